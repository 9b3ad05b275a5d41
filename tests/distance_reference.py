"""Independent NumPy float64 statement of the signed geom distance (include/mjpl_hip.h: mjpl_distances*).

d(g1, g2) is the exact Euclidean signed distance of the two solids: the gap width when they are disjoint, minus
the penetration depth (shortest separating translation) when they overlap.  A plane is a half-space: d is the
signed height of the geom's lowest point.  Margins are not subtracted.

Every non-plane pair is reduced to core distance minus radii (sphere = point, capsule = segment, box = box):
  * disjoint cores: the minimum over every feature pair that can hold the closest points (end points, the
    interior critical point of two lines, box vertices and edges, a point clamped into a box);
  * overlapping cores: the least overlap of the two projected intervals over the separating axes, taken in the
    world frame (box face normals, normalised cross products of edge directions).
Poses come from the CPU oracle's forward kinematics (oracle.pyoracle: fk).  Everything is vectorised over
configurations, per pair type; nothing of the product's routines is used.
"""
import numpy as np

PLANE, SPHERE, CAPSULE, BOX = 0, 2, 3, 6
_SKIP_CROSS = 1e-12  # squared sine below which an edge-pair axis is left out (parallel edges)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def pt_seg(p, a, b):
    """Distance from points p to segments [a, b] (broadcast over leading axes)."""
    d = b - a
    dd = _dot(d, d)
    t = np.where(dd > 0, _dot(p - a, d) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return _norm(p - (a + t[..., None] * d))


def seg_seg(p1, q1, p2, q2):
    """Distance between segments [p1, q1] and [p2, q2]: an end point against the other segment (4 cases), or
    the critical point of the two lines when it lies inside both segments."""
    best = np.minimum(np.minimum(pt_seg(p1, p2, q2), pt_seg(q1, p2, q2)),
                      np.minimum(pt_seg(p2, p1, q1), pt_seg(q2, p1, q1)))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, b, e = _dot(d1, d1), _dot(d1, d2), _dot(d2, d2)
    c, f = _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > 1e-14 * a * e
    safe = np.where(ok, den, 1.0)
    s = (b * f - c * e) / safe
    t = (a * f - b * c) / safe
    inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    di = _norm(p1 + s[..., None] * d1 - (p2 + t[..., None] * d2))
    return np.where(inside, np.minimum(best, di), best)


def box_corners(pos, mat, size):
    """[..., 8, 3] world corners; corner c has sign + on axis k iff bit k of c is set."""
    R = mat.reshape(mat.shape[:-1] + (3, 3))
    signs = np.array([[1 if (c >> k) & 1 else -1 for k in range(3)] for c in range(8)], float)
    local = signs * size[..., None, :]
    return pos[..., None, :] + np.einsum("...ij,...cj->...ci", R, local)


_EDGES = [(c, c | (1 << k)) for c in range(8) for k in range(3) if not (c >> k) & 1]  # 12 corner pairs


def box_edges(pos, mat, size):
    cs = box_corners(pos, mat, size)
    a = np.stack([cs[..., i, :] for i, _ in _EDGES], axis=-2)
    b = np.stack([cs[..., j, :] for _, j in _EDGES], axis=-2)
    return a, b  # [..., 12, 3] each


def pt_box(p, pos, mat, size):
    """Distance from world points p [..., 3] to the box (0 inside)."""
    R = mat.reshape(mat.shape[:-1] + (3, 3))
    loc = np.einsum("...ji,...j->...i", R, p - pos)
    return _norm(loc - np.clip(loc, -size, size))


def _interval_box(axis, pos, mat, size):
    R = mat.reshape(mat.shape[:-1] + (3, 3))
    c = _dot(axis, pos)
    rad = np.sum(size * np.abs(np.einsum("...ji,...j->...i", R, axis)), axis=-1)
    return c - rad, c + rad


def _overlap(lo1, hi1, lo2, hi2):
    return np.minimum(hi1 - lo2, hi2 - lo1)


def _unit_or_none(v):
    n2 = _dot(v, v)
    ok = n2 >= _SKIP_CROSS
    return v / np.sqrt(np.where(ok, n2, 1.0))[..., None], ok


def _sat_depth(axes_oks, intervals):
    """least overlap over axes (ok ones only); separated iff some overlap < 0"""
    depth = np.full(intervals(axes_oks[0][0])[0].shape, np.inf)
    sep = np.zeros(depth.shape, bool)
    for ax, ok in axes_oks:
        lo1, hi1, lo2, hi2 = intervals(ax)
        o = _overlap(lo1, hi1, lo2, hi2)
        depth = np.where(ok, np.minimum(depth, o), depth)
        sep |= ok & (o < 0)
    return depth, sep


def point_box(c, pos, mat, size):
    """Signed distance of the point c to the box (negative inside: minus the distance to the nearest face)."""
    R = mat.reshape(mat.shape[:-1] + (3, 3))
    loc = np.einsum("...ji,...j->...i", R, c - pos)
    out = _norm(loc - np.clip(loc, -size, size))
    inside_depth = np.min(size - np.abs(loc), axis=-1)
    return np.where(np.all(np.abs(loc) <= size, axis=-1), -inside_depth, out)


def segment_box(a, b, pos, mat, size):
    """Signed distance of the segment [a, b] to the box."""
    R = mat.reshape(mat.shape[:-1] + (3, 3))
    u = b - a
    axes = [(R[..., :, k], np.ones(a.shape[:-1], bool)) for k in range(3)]
    lu = _norm(u)
    for k in range(3):
        cr = np.cross(u, R[..., :, k])
        n2 = _dot(cr, cr)
        ok = n2 > _SKIP_CROSS * lu * lu
        axes.append((cr / np.sqrt(np.where(ok, n2, 1.0))[..., None], ok))

    def intervals(ax):
        pa, pb = _dot(ax, a), _dot(ax, b)
        lo2, hi2 = _interval_box(ax, pos, mat, size)
        return np.minimum(pa, pb), np.maximum(pa, pb), lo2, hi2

    depth, sep = _sat_depth(axes, intervals)
    ea, eb = box_edges(pos, mat, size)
    dis = np.minimum(pt_box(a, pos, mat, size), pt_box(b, pos, mat, size))
    dis = np.minimum(dis, np.min(seg_seg(a[..., None, :], b[..., None, :], ea, eb), axis=-1))
    return np.where(sep, dis, -depth)


def box_box(pos1, mat1, size1, pos2, mat2, size2):
    R1 = mat1.reshape(mat1.shape[:-1] + (3, 3))
    R2 = mat2.reshape(mat2.shape[:-1] + (3, 3))
    ones = np.ones(pos1.shape[:-1], bool)
    axes = [(R1[..., :, k], ones) for k in range(3)] + [(R2[..., :, k], ones) for k in range(3)]
    for i in range(3):
        for j in range(3):
            axes.append(_unit_or_none(np.cross(R1[..., :, i], R2[..., :, j])))

    def intervals(ax):
        lo1, hi1 = _interval_box(ax, pos1, mat1, size1)
        lo2, hi2 = _interval_box(ax, pos2, mat2, size2)
        return lo1, hi1, lo2, hi2

    depth, sep = _sat_depth(axes, intervals)
    c1, c2 = box_corners(pos1, mat1, size1), box_corners(pos2, mat2, size2)
    dis = np.minimum(np.min(pt_box(c1, pos2[..., None, :], mat2[..., None, :], size2[..., None, :]), axis=-1),
                     np.min(pt_box(c2, pos1[..., None, :], mat1[..., None, :], size1[..., None, :]), axis=-1))
    a1, b1 = box_edges(pos1, mat1, size1)
    a2, b2 = box_edges(pos2, mat2, size2)
    ee = seg_seg(a1[..., :, None, :], b1[..., :, None, :], a2[..., None, :, :], b2[..., None, :, :])
    dis = np.minimum(dis, np.min(ee.reshape(ee.shape[:-2] + (144,)), axis=-1))
    return np.where(sep, dis, -depth)


def _core(t, pos, mat, size):
    """sphere -> (pos, pos); capsule -> its segment's end points"""
    if t == SPHERE:
        return pos, pos
    ax = mat[..., [2, 5, 8]] * size[..., 1:2]
    return pos - ax, pos + ax


def geom_distance(t1, pos1, mat1, size1, t2, pos2, mat2, size2):
    """Signed distance of two geoms; pos [..., 3], mat [..., 9] (row-major), size [..., 3]."""
    pos1, mat1, size1, pos2, mat2, size2 = (np.asarray(x, float) for x in (pos1, mat1, size1, pos2, mat2, size2))
    if t1 == PLANE and t2 == PLANE:
        raise ValueError("plane-plane has no distance")
    if t2 == PLANE:
        t1, pos1, mat1, size1, t2, pos2, mat2, size2 = t2, pos2, mat2, size2, t1, pos1, mat1, size1
    if t1 == PLANE:
        n = mat1[..., [2, 5, 8]]
        if t2 == BOX:
            return np.min(_dot(box_corners(pos2, mat2, size2) - pos1[..., None, :], n[..., None, :]), axis=-1)
        a, b = _core(t2, pos2, mat2, size2)
        return np.minimum(_dot(a - pos1, n), _dot(b - pos1, n)) - size2[..., 0]
    if t1 == BOX and t2 == BOX:
        return box_box(pos1, mat1, size1, pos2, mat2, size2)
    if t1 == BOX:
        t1, pos1, mat1, size1, t2, pos2, mat2, size2 = t2, pos2, mat2, size2, t1, pos1, mat1, size1
    if t2 == BOX:
        a, b = _core(t1, pos1, mat1, size1)
        if t1 == SPHERE:
            return point_box(a, pos2, mat2, size2) - size1[..., 0]
        return segment_box(a, b, pos2, mat2, size2) - size1[..., 0]
    a1, b1 = _core(t1, pos1, mat1, size1)
    a2, b2 = _core(t2, pos2, mat2, size2)
    return seg_seg(a1, b1, a2, b2) - size1[..., 0] - size2[..., 0]


def pair_distances(model, geom_xpos, geom_xmat, pairs):
    """[N, ngeom, 3] / [N, ngeom, 9] world poses and candidate pairs [P, 2] -> D [N, P]."""
    gt = np.asarray(model.geom_type)
    gs = np.asarray(model.geom_size, float).reshape(-1, 3)
    n = geom_xpos.shape[0]
    D = np.zeros((n, len(pairs)))
    for p, (g1, g2) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        D[:, p] = geom_distance(int(gt[g1]), geom_xpos[:, g1], geom_xmat[:, g1], np.broadcast_to(gs[g1], (n, 3)),
                                int(gt[g2]), geom_xpos[:, g2], geom_xmat[:, g2], np.broadcast_to(gs[g2], (n, 3)))
    return D


def reference_distances(model, Q, pairs):
    """D [N, P] at the full-nq configurations Q [N, nq], poses from the oracle's forward kinematics."""
    from oracle import pyoracle
    k = pyoracle.Oracle(model).fk(np.asarray(Q, float))
    return pair_distances(model, k["geom_xpos"], k["geom_xmat"], pairs)


def pair_margins(model, pairs):
    m = np.asarray(model.geom_margin, float)
    pairs = np.asarray(pairs).reshape(-1, 2)
    return np.maximum(m[pairs[:, 0]], m[pairs[:, 1]])


def clearance_from(D, margins, allowed):
    """(C, pair) from D [N, P]: min over non-allowed pairs of D - margin, lowest index on ties."""
    keep = np.flatnonzero(~np.asarray(allowed, bool))
    n = D.shape[0]
    if len(keep) == 0:
        return None, np.full(n, -1, np.int32)
    V = D[:, keep] - margins[keep]
    arg = np.argmin(V, axis=1)  # (the first minimum)
    return V[np.arange(n), arg], keep[arg].astype(np.int32)
