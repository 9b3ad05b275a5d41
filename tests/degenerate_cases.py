"""Seeded pose families where the distance, clearance and witness routines have their branches -- touching,
aligned and coincident poses -- for the pod models of tests/pose_pods.py, and their expected values.  Shared by
tests/test_degenerate_cases_host.py (no GPU) and tests/test_gpu_degenerate_poses.py.

Every set has N rows; a row has one TARGET pair (one of the G x G pairs of the two pods, or one of the G pairs of
the plane model), placed deliberately; the other pairs of the row come along as ordinary poses.

  T  touching: random attitudes, geom 2 on a ray from geom 1; the ray parameter s* at which the target pair just
     touches by bisection of narrowphase_cases.gap in longdouble; the row takes s* + delta, delta in the classes of
     narrowphase_cases (apart, deep, six bands +-10^U[-9, -3]).
  A  aligned: a tilt of 0 (a tenth of the rows) or 10^U[-9, -3] about a random axis away from exact alignment of
     two features, and a gap of 10^U[-9, -1] beyond touching (found by the same bisection, along the set's ray).
  C  coincident cores: the cores of the target pair meet.

Expected values: poses are the CPU oracle's fk(Q); the target pair, where its cores are more than CORE_APART apart,
takes narrowphase_cases.gap in longdouble (box-box: narrowphase_cases.box_box_dist wherever the overlap predicate
says disjoint); every other entry takes tests/distance_reference.py.
"""
import functools
import hashlib

import numpy as np

import distance_reference as ref
import narrowphase_cases as nc
import pose_pods as pods

LD = nc.LD
PLANE, SPHERE, CAPSULE, BOX = nc.PLANE, nc.SPHERE, nc.CAPSULE, nc.BOX
N = 1024
G = 2
RECIPE = 1
CORE_APART = 1e-6
GRAD_OK, GRAD_DEGENERATE = 0, 2  # include/mjpl_hip.h: MJPL_GRAD_*
PLANE_POS = np.array([0.1, -0.2, -0.3])
PLANE_QUAT = np.array([0.9, 0.2, -0.3, 0.1]) / np.linalg.norm([0.9, 0.2, -0.3, 0.1])

_I = np.eye(3)
_C1 = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])  # z -> x, x -> y, y -> z
_C2 = _C1.T                                          # z -> y
_Z90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
_Z_TO = [_C1, _C2, _I]                               # _Z_TO[k] takes the z axis to axis k
_PERMS = np.stack([_I, _C1, _C2, _Z90])


# ------------------------------------------------------------------ draws
def _rng(name):
    return np.random.default_rng([RECIPE] + [ord(c) for c in name])


def _rand_rot(rng, n):
    return nc.quat_mat64(rng.normal(size=(n, 4)))


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _axis_rot(ax, ang):
    """Rodrigues: rotations by ang [n] about the unit axes ax [n, 3]; exactly the identity where ang == 0"""
    K = np.zeros((len(ang), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def _tilt(rng, n):
    """(dR [n, 3, 3], angle [n], band [n]): band 0 = no tilt (a tenth), band 1 + k = angle in [10^-(9-k), 10^-(8-k))"""
    ex = rng.uniform(-9, -3, n)
    exact = rng.uniform(size=n) < 0.1
    ang = np.where(exact, 0.0, 10.0 ** ex)
    band = np.where(exact, 0, 1 + np.minimum(np.floor(ex + 9).astype(int), 5))
    return _axis_rot(_unit(rng, n), ang), ang, band


def _gap(rng, n):
    return 10.0 ** rng.uniform(-9, -1, n)


def _sizes(rng, t):
    return nc._sizes(rng, t, G) if t != PLANE else np.zeros((1, 3))


def _bound(t, s):
    return nc._bound(t, s)


def _touch(t1, p1, R1, S1, t2, base2, u, R2, S2):
    """s* [n] (float64): geom 2 at base2 + s u just touches geom 1, by bisection in longdouble on poses composed in
    longdouble.  The pair overlaps at s = 0 and is apart far out; both shapes are convex.  (The NumPy statement
    finds where to look first, which spares most of the longdouble evaluations: the bracket it proposes is checked
    in longdouble, and the bisection starts from 0 and far out where that fails.)"""
    P1, r1, s1, B, U, r2, s2 = (x.astype(LD) for x in (p1, R1, S1, base2, u, R2, S2))

    def g(s):
        return nc.gap(t1, P1, r1, s1, t2, B + s[:, None] * U, r2, s2)

    n = len(p1)
    far = _bound(t1, S1) + _bound(t2, S2) + np.linalg.norm(base2 - p1, axis=1) + 1.0
    if t1 == PLANE:
        far = far / 0.3
    a, b = np.zeros(n), far.copy()
    m1, m2 = R1.reshape(n, 9), R2.reshape(n, 9)
    for _ in range(0 if t1 == BOX else 48):  # (boxes: the longdouble predicate is the cheaper one)
        mid = (a + b) / 2
        inside = ref.geom_distance(t1, p1, m1, S1, t2, base2 + mid[:, None] * u, m2, S2) <= 0
        a, b = np.where(inside, mid, a), np.where(inside, b, mid)
    lo, hi = np.maximum(a - 1e-10, 0.0).astype(LD), (b + 1e-10).astype(LD)
    good = np.asarray((g(lo) <= 0) & (g(hi) > 0)) & (t1 != BOX)
    lo, hi = np.where(good, lo, LD(0)), np.where(good, hi, far.astype(LD))
    assert np.all(g(lo) <= 0) and np.all(g(hi) > 0)
    for _ in range(40 if good.all() else 72):
        mid = (lo + hi) / 2
        inside = g(mid) <= 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    return ((lo + hi) / 2).astype(np.float64)


def _new(name, family, t1, t2, sizes1, sizes2, ta, tb, p1, R1, p2, R2, **labels):
    n = len(p2)
    cs = dict(name=name, family=family, t1=t1, t2=t2, sizes1=sizes1, sizes2=sizes2, tgt_a=ta, tgt_b=tb,
              p1=p1, R1=R1, p2=p2, R2=R2,
              cls=np.full(n, -1), sign=np.zeros(n, bool), tilt=np.full(n, np.nan), tilt_band=np.full(n, -1),
              gap=np.full(n, np.nan), kind=np.zeros(n, int), aligned=np.zeros(n, bool),
              want_status=np.full(n, -1), closed=np.full(n, np.nan))
    cs.update(labels)
    if t1 == PLANE:
        cs["Q"] = pods.configs(None, None, p2, R2)
    else:
        cs["Q"] = pods.configs(p1, R1, p2, R2)
    return cs


def _targets(rng, t1, n):
    return (rng.integers(0, G, n) if t1 != PLANE else np.zeros(n, int)), rng.integers(0, G, n)


def _plane_frame(n):
    R = nc.quat_mat64(PLANE_QUAT[None])[0]
    return np.repeat(PLANE_POS[None], n, 0), np.repeat(R[None], n, 0)


# ------------------------------------------------------------------ T: touching
def _touching(t1, t2):
    name = f"T {nc.NAMES[t1]}-{nc.NAMES[t2]}"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, t1), _sizes(rng, t2)
    ta, tb = _targets(rng, t1, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    if t1 == PLANE:
        p1, R1 = _plane_frame(n)
    else:
        p1, R1 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    R2 = _rand_rot(rng, n)
    u = _unit(rng, n)
    if t1 == PLANE:  # leave the plane on its upper side, not too flat (narrowphase_cases.draw)
        nrm = R1[:, :, 2]
        d = np.sum(u * nrm, axis=1, keepdims=True)
        u = u - d * nrm + np.abs(d) * nrm + 0.3 * nrm
        u /= np.linalg.norm(u, axis=1, keepdims=True)
    cls = rng.integers(0, 8, n)
    sign = rng.integers(0, 2, n).astype(bool)  # bands: True = apart side
    mag = 10.0 ** (-(9 - (cls.astype(float) - nc.BAND0)) + rng.uniform(0, 1, n))
    delta = np.where(cls == nc.APART, rng.uniform(0.01, 0.3, n), np.where(sign, mag, -mag))
    frac = rng.uniform(0, 0.9, n)
    sstar = _touch(t1, p1, R1, S1, t2, p1, u, R2, S2)
    s = np.maximum(np.where(cls == nc.DEEP, sstar * frac, sstar + delta), 0.0)
    return _new(name, "T", t1, t2, sizes1, sizes2, ta, tb, p1, R1, p1 + s[:, None] * u, R2, cls=cls, sign=sign, s=s)


# ------------------------------------------------------------------ A: aligned
def _finish_aligned(name, t1, t2, sizes1, sizes2, ta, tb, p1, R1, base2, u, R2, rng, ang, band, **labels):
    """geom 2 from base2 along u to touching, then the gap beyond"""
    n = len(p1)
    gap = _gap(rng, n)
    sstar = _touch(t1, p1, R1, sizes1[ta], t2, base2, u, R2, sizes2[tb])
    p2 = base2 + (sstar + gap)[:, None] * u
    return _new(name, "A", t1, t2, sizes1, sizes2, ta, tb, p1, R1, p2, R2, tilt=ang, tilt_band=band, gap=gap, **labels)


def _a_capsules():
    """capsule || capsule, as narrowphase_cases.draw makes its nearly parallel ones: the tilted attitude, a ray"""
    name = "A capsule || capsule"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, CAPSULE), _sizes(rng, CAPSULE)
    ta, tb = _targets(rng, CAPSULE, n)
    p1, R1 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    dR, ang, band = _tilt(rng, n)
    R2 = dR @ R1
    u = _unit(rng, n)
    return _finish_aligned(name, CAPSULE, CAPSULE, sizes1, sizes2, ta, tb, p1, R1, p1, u, R2, rng, ang, band,
                           aligned=ang == 0)


def _a_capsule_edge():
    """capsule axis || box edge k, the capsule beside that edge: it leaves the edge along a direction of the outward
    quadrant, shifted along the edge by up to the sum of the half lengths"""
    name = "A capsule || box edge"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, CAPSULE), _sizes(rng, BOX)
    ta, tb = _targets(rng, CAPSULE, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    p1, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    dR, ang, band = _tilt(rng, n)
    k = np.where(ang == 0, rng.integers(0, 3, n) // 2 * 2, rng.integers(0, 3, n))  # (no tilt: z or x)
    R1 = dR @ R2 @ np.stack(_Z_TO)[k]
    i, j = (k + 1) % 3, (k + 2) % 3
    rows = np.arange(n)
    sg = rng.choice([-1.0, 1.0], (n, 2))
    phi = rng.uniform(0, np.pi / 2, n)
    phi = np.where(rng.uniform(size=n) < 0.2, rng.integers(0, 2, n) * (np.pi / 2), phi)  # (some straight off a face)
    edge = np.zeros((n, 3))   # a point of the edge, box frame
    edge[rows, i], edge[rows, j] = sg[:, 0] * S2[rows, i], sg[:, 1] * S2[rows, j]
    edge[rows, k] = rng.uniform(-1, 1, n) * (S2[rows, k] + 0.9 * S1[:, 1])
    out = np.zeros((n, 3))    # the way out, box frame
    out[rows, i], out[rows, j] = sg[:, 0] * np.cos(phi), sg[:, 1] * np.sin(phi)
    # the capsule stays: the box centre is where the capsule's centre sits on the edge, then backs away
    base2 = p1 - np.einsum("nij,nj->ni", R2, edge)
    u = -np.einsum("nij,nj->ni", R2, out)
    return _finish_aligned(name, CAPSULE, BOX, sizes1, sizes2, ta, tb, p1, R1, base2, u, R2, rng, ang, band,
                           aligned=(ang == 0) & (k == 2), kind=k)


def _a_capsule_face():
    """capsule axis || box face, the capsule lying over that face"""
    name = "A capsule || box face"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, CAPSULE), _sizes(rng, BOX)
    ta, tb = _targets(rng, CAPSULE, n)
    S2 = sizes2[tb]
    p1, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    dR, ang, band = _tilt(rng, n)
    rows = np.arange(n)
    # the face normal e_f; the axis in the face: no tilt: the box's own z axis (f = x or y), else any direction of it
    f = np.where(ang == 0, rng.integers(0, 2, n), rng.integers(0, 3, n))
    theta = np.where(ang == 0, 0.0, rng.uniform(0, 2 * np.pi, n))
    ef = np.zeros((n, 3))
    ef[rows, f] = 1.0
    spin = _axis_rot(ef, theta)                      # about the face normal
    first = np.where(ang == 0, 2, (f + 1) % 3)       # the axis at theta = 0
    R1 = dR @ R2 @ spin @ np.stack(_Z_TO)[first]
    sg = rng.choice([-1.0, 1.0], n)
    lat = rng.uniform(-1, 1, (n, 3)) * S2
    lat[rows, f] = 0.0
    base2 = p1 - np.einsum("nij,nj->ni", R2, lat)
    u = -np.einsum("nij,nj->ni", R2, ef * sg[:, None])
    return _finish_aligned(name, CAPSULE, BOX, sizes1, sizes2, ta, tb, p1, R1, base2, u, R2, rng, ang, band,
                           aligned=ang == 0, kind=f)


def _a_boxes():
    """box || box: the same attitude or a 90 degree axis permutation of it.  kind 0: face to face, the lateral
    offsets up to the sum of the half extents; kind 1: leaving through a corner direction along which two axes
    separate almost together, which takes the closest features to parallel edges"""
    name = "A box || box"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, BOX), _sizes(rng, BOX)
    ta, tb = _targets(rng, BOX, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    p1, R1 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    dR, ang, band = _tilt(rng, n)
    perm = np.where((ang == 0) & (rng.uniform(size=n) < 0.5), 0, rng.integers(0, 4, n))  # (no tilt: half identical)
    R2 = dR @ R1 @ _PERMS[perm]
    S2in1 = np.einsum("nij,nj->ni", np.abs(_PERMS[perm]), S2)  # box 2's half extents along box 1's axes
    reach = S1 + S2in1
    rows = np.arange(n)
    kind = rng.integers(0, 2, n)
    k = rng.integers(0, 3, n)
    sg = rng.choice([-1.0, 1.0], (n, 3))
    off = rng.uniform(-1, 1, (n, 3)) * reach
    off[rows, k] = 0.0
    out = np.zeros((n, 3))
    out[rows, k] = sg[rows, k]
    # kind 1: no offset on axis i either, and the way out reaches both faces nearly together
    i = (k + 1) % 3
    jit = 1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, -0.5, n)
    corner = np.zeros((n, 3))
    corner[rows, k] = sg[rows, k] * reach[rows, k]
    corner[rows, i] = sg[rows, i] * reach[rows, i] * jit
    corner /= np.linalg.norm(corner, axis=1, keepdims=True)
    off1 = off.copy()
    off1[rows, i] = 0.0
    off = np.where(kind[:, None] == 1, off1, off)
    out = np.where(kind[:, None] == 1, corner, out)
    base2 = p1 + np.einsum("nij,nj->ni", R1, off)
    u = np.einsum("nij,nj->ni", R1, out)
    return _finish_aligned(name, BOX, BOX, sizes1, sizes2, ta, tb, p1, R1, base2, u, R2, rng, ang, band,
                           aligned=(ang == 0) & (perm == 0), kind=kind, perm=perm)


def _a_plane_box():
    """plane || box face: the four lowest corners tie"""
    name = "A plane || box face"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, PLANE), _sizes(rng, BOX)
    ta, tb = _targets(rng, PLANE, n)
    p1, R1 = _plane_frame(n)
    dR, ang, band = _tilt(rng, n)
    perm = rng.integers(0, 4, n)
    flip = np.where(rng.uniform(size=n) < 0.5, 0.0, np.pi)   # either of the two faces down
    R2 = dR @ R1 @ _axis_rot(np.repeat([[1.0, 0, 0]], n, 0), flip) @ _PERMS[perm]
    lat = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)
    base2 = p1 + np.einsum("nij,nj->ni", R1, lat) - 1.0 * R1[:, :, 2]
    return _finish_aligned(name, PLANE, BOX, sizes1, sizes2, ta, tb, p1, R1, base2, R1[:, :, 2].copy(), R2, rng, ang, band,
                           kind=perm)


def _a_plane_capsule():
    """plane || capsule axis: both end points tie"""
    name = "A plane || capsule axis"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, PLANE), _sizes(rng, CAPSULE)
    ta, tb = _targets(rng, PLANE, n)
    p1, R1 = _plane_frame(n)
    dR, ang, band = _tilt(rng, n)
    theta = rng.uniform(0, 2 * np.pi, n)
    R2 = dR @ R1 @ _axis_rot(np.repeat([[0.0, 0, 1]], n, 0), theta) @ _C1
    lat = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)
    base2 = p1 + np.einsum("nij,nj->ni", R1, lat) - 1.0 * R1[:, :, 2]
    return _finish_aligned(name, PLANE, CAPSULE, sizes1, sizes2, ta, tb, p1, R1, base2, R1[:, :, 2].copy(), R2, rng, ang,
                           band)


def _a_sphere_voronoi():
    """The Voronoi boundaries of pt_box_d2.  kind 0: the sphere's centre on the extension of a box face plane (beyond
    the box along another axis); kind 1: on a box edge line, beyond the edge's end.  What a tilt is to the other sets
    is here the centre's distance (metres) from that plane or line."""
    name = "A sphere on box Voronoi boundaries"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, SPHERE), _sizes(rng, BOX)
    ta, tb = _targets(rng, SPHERE, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    p2, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    R1 = _rand_rot(rng, n)
    _, ang, band = _tilt(rng, n)
    dev = ang * rng.choice([-1.0, 1.0], n)
    dev2 = ang * rng.choice([-1.0, 1.0], n)
    gap = _gap(rng, n)
    kind = rng.integers(0, 2, n)
    k = rng.integers(0, 3, n)
    i, j = (k + 1) % 3, (k + 2) % 3
    rows = np.arange(n)
    sg = rng.choice([-1.0, 1.0], (n, 3))
    c = np.zeros((n, 3))  # the centre, box frame
    # kind 0: coordinate k on the face plane, i beyond the box by the radius and the gap, j anywhere near
    c[rows, k] = sg[rows, k] * S2[rows, k] + dev
    c[rows, i] = sg[rows, i] * (S2[rows, i] + S1[:, 0] + gap)
    c[rows, j] = rng.uniform(-1.2, 1.2, n) * S2[rows, j]
    # kind 1: coordinates i and j on the edge line, k beyond the end
    c1 = np.zeros((n, 3))
    c1[rows, i] = sg[rows, i] * S2[rows, i] + dev
    c1[rows, j] = sg[rows, j] * S2[rows, j] + dev2
    c1[rows, k] = sg[rows, k] * (S2[rows, k] + S1[:, 0] + gap)
    c = np.where(kind[:, None] == 1, c1, c)
    p1 = p2 + np.einsum("nij,nj->ni", R2, c)
    return _new(name, "A", SPHERE, BOX, sizes1, sizes2, ta, tb, p1, R1, p2, R2, tilt=ang, tilt_band=band, gap=gap, kind=kind)


# ------------------------------------------------------------------ C: coincident cores
def _c_spheres():
    name = "C concentric spheres"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, SPHERE), _sizes(rng, SPHERE)
    ta, tb = _targets(rng, SPHERE, n)
    p1 = rng.uniform(-0.5, 0.5, (n, 3))
    return _new(name, "C", SPHERE, SPHERE, sizes1, sizes2, ta, tb, p1, _rand_rot(rng, n), p1.copy(), _rand_rot(rng, n),
                want_status=np.full(n, GRAD_DEGENERATE))


def _c_sphere_on_axis():
    name = "C sphere centre on capsule axis"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, SPHERE), _sizes(rng, CAPSULE)
    ta, tb = _targets(rng, SPHERE, n)
    p2, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    kind = rng.integers(0, 3, n)  # 0: inside the segment, 1: its end point, 2: its middle
    t = np.where(kind == 0, rng.uniform(-1, 1, n), np.where(kind == 1, rng.choice([-1.0, 1.0], n), 0.0))
    p1 = p2 + (t * sizes2[tb, 1])[:, None] * R2[:, :, 2]
    return _new(name, "C", SPHERE, CAPSULE, sizes1, sizes2, ta, tb, p1, _rand_rot(rng, n), p2, R2, kind=kind)


def _c_capsules_crossing():
    name = "C capsule axes crossing"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, CAPSULE), _sizes(rng, CAPSULE)
    ta, tb = _targets(rng, CAPSULE, n)
    p1, R1, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n), _rand_rot(rng, n)
    kind = (rng.uniform(size=n) < 0.15).astype(int)  # 1: at an end point of capsule 1
    a = np.where(kind == 1, rng.choice([-1.0, 1.0], n), rng.uniform(-0.95, 0.95, n)) * sizes1[ta, 1]
    b = rng.uniform(-0.95, 0.95, n) * sizes2[tb, 1]
    p2 = p1 + a[:, None] * R1[:, :, 2] - b[:, None] * R2[:, :, 2]
    return _new(name, "C", CAPSULE, CAPSULE, sizes1, sizes2, ta, tb, p1, R1, p2, R2, kind=kind,
                want_status=np.full(n, GRAD_DEGENERATE))


def _c_sphere_on_face():
    """kind 0: the centre exactly on a box face; 1: at the box centre; 2 / 3: 10^U[-12, -9] inside / outside the face"""
    name = "C sphere centre on box face"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, SPHERE), _sizes(rng, BOX)
    ta, tb = _targets(rng, SPHERE, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    p2, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    kind = rng.integers(0, 4, n)
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    eps = 10.0 ** rng.uniform(-12, -9, n)
    c = rng.uniform(-0.9, 0.9, (n, 3)) * S2
    c[rows, k] = rng.choice([-1.0, 1.0], n) * (S2[rows, k] + np.where(kind == 2, -eps, np.where(kind == 3, eps, 0.0)))
    c = np.where(kind[:, None] == 1, 0.0, c)
    p1 = p2 + np.einsum("nij,nj->ni", R2, c)
    p1 = np.where(kind[:, None] == 1, p2, p1)
    return _new(name, "C", SPHERE, BOX, sizes1, sizes2, ta, tb, p1, _rand_rot(rng, n), p2, R2, kind=kind,
                want_status=np.where(kind == 1, GRAD_OK, -1),
                closed=np.where(kind == 1, -S2.min(axis=1) - S1[:, 0], np.nan))


def _c_capsule_through_box():
    """The capsule's centre at the box centre.  kind 0: any attitude; kind 1: the axis along box axis k, where the
    depth has a closed form: the radius plus the lesser half extent across the axis, or, when that is less, the way out
    along the axis (half extent plus half length)"""
    name = "C capsule through box centre"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, CAPSULE), _sizes(rng, BOX)
    ta, tb = _targets(rng, CAPSULE, n)
    S1, S2 = sizes1[ta], sizes2[tb]
    p2, R2 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    kind = rng.integers(0, 2, n)
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    R1 = np.where(kind[:, None, None] == 1, R2 @ np.stack(_Z_TO)[k], _rand_rot(rng, n))
    across = np.minimum(S2[rows, (k + 1) % 3], S2[rows, (k + 2) % 3])
    depth = np.minimum(across, S2[rows, k] + S1[:, 1])
    return _new(name, "C", CAPSULE, BOX, sizes1, sizes2, ta, tb, p2.copy(), R1, p2, R2, kind=kind,
                aligned=(kind == 1) & (k == 2), want_status=np.full(n, GRAD_OK),
                closed=np.where(kind == 1, -depth - S1[:, 0], np.nan))


def _c_boxes():
    """Boxes with a common centre.  kind 0: any attitudes; 1: the same attitude; 2: tilted by 10^U[-9, -3]"""
    name = "C boxes with a common centre"
    rng = _rng(name)
    n = N
    sizes1, sizes2 = _sizes(rng, BOX), _sizes(rng, BOX)
    ta, tb = _targets(rng, BOX, n)
    p1, R1 = rng.uniform(-0.5, 0.5, (n, 3)), _rand_rot(rng, n)
    kind = rng.integers(0, 3, n)
    ang = np.where(kind == 2, 10.0 ** rng.uniform(-9, -3, n), 0.0)
    R2 = np.where(kind[:, None, None] == 0, _rand_rot(rng, n), _axis_rot(_unit(rng, n), ang) @ R1)
    return _new(name, "C", BOX, BOX, sizes1, sizes2, ta, tb, p1, R1, p1.copy(), R2, kind=kind, aligned=kind == 1, tilt=ang)


_MAKERS = {f"T {nc.NAMES[a]}-{nc.NAMES[b]}": functools.partial(_touching, a, b) for a, b in nc.PAIRS}
_MAKERS.update({
    "A capsule || capsule": _a_capsules, "A capsule || box edge": _a_capsule_edge, "A capsule || box face": _a_capsule_face,
    "A box || box": _a_boxes, "A plane || box face": _a_plane_box, "A plane || capsule axis": _a_plane_capsule,
    "A sphere on box Voronoi boundaries": _a_sphere_voronoi,
    "C concentric spheres": _c_spheres, "C sphere centre on capsule axis": _c_sphere_on_axis,
    "C capsule axes crossing": _c_capsules_crossing, "C sphere centre on box face": _c_sphere_on_face,
    "C capsule through box centre": _c_capsule_through_box, "C boxes with a common centre": _c_boxes})
SETS = list(_MAKERS)


@functools.lru_cache(maxsize=None)
def case_set(name):
    """The set `name`: made once, shared and left unchanged"""
    cs = _MAKERS[name]()
    assert cs["name"] == name and len(cs["Q"]) == N
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


@functools.lru_cache(maxsize=None)
def model_of(name):
    cs = case_set(name)
    if cs["t1"] == PLANE:
        return pods.plane_pod_model(PLANE_POS, PLANE_QUAT, cs["t2"], cs["sizes2"])
    return pods.two_pod_model(cs["t1"], cs["sizes1"], cs["t2"], cs["sizes2"])


def digest(cs) -> str:
    return hashlib.sha256(np.ascontiguousarray(cs["Q"], dtype="<f8").tobytes()).hexdigest()[:16]


# ------------------------------------------------------------------ expected values
_RAD = {PLANE: lambda s: 0 * s[:, 0], SPHERE: lambda s: s[:, 0], CAPSULE: lambda s: s[:, 0], BOX: lambda s: 0 * s[:, 0]}


@functools.lru_cache(maxsize=None)
def poses(name):
    k = pods.fk(model_of(name), case_set(name)["Q"])
    for v in k.values():
        v.setflags(write=False)
    return k


def _ld_pose(k, g, rows=None):
    n = len(g)
    i = np.arange(n) if rows is None else rows
    return k["geom_xpos"][i, g].astype(LD), k["geom_xmat"][i, g].reshape(n, 3, 3).astype(LD)


def ld_gap(name, g1, g2, distance=True, rows=None):
    """(gap [N] longdouble, core gap [N] longdouble) of the geoms g1 [N], g2 [N] (types in PAIRS order) at the
    oracle's poses (of the given rows, default all): narrowphase_cases.gap.  Boxes: box_box_dist where the overlap
    predicate says disjoint (only with `distance`; else +1), -1 and core gap 0 where it says overlapping.  A plane
    pair has no core gap: inf."""
    cs, m, k = case_set(name), model_of(name), poses(name)
    t1, t2 = cs["t1"], cs["t2"]
    gs = np.asarray(m.geom_size, float).reshape(-1, 3)
    p1, R1 = _ld_pose(k, g1, rows)
    p2, R2 = _ld_pose(k, g2, rows)
    s1, s2 = gs[g1].astype(LD), gs[g2].astype(LD)
    gap = nc.gap(t1, p1, R1, s1, t2, p2, R2, s2)
    if t1 == BOX:
        apart = np.asarray(gap > 0)
        if distance and apart.any():
            gap = np.array(gap, LD)
            gap[apart] = nc.box_box_dist(p1[apart], R1[apart], s1[apart], p2[apart], R2[apart], s2[apart])
        return gap, np.where(apart, gap, LD(0))
    if t1 == PLANE:
        return gap, np.full(len(g1), np.inf, LD)
    return gap, gap + _RAD[t1](s1) + _RAD[t2](s2)


@functools.lru_cache(maxsize=None)
def target_ld(name):
    """(gap, core gap) in longdouble of every row's target pair"""
    cs, m = case_set(name), model_of(name)
    ga, gb = pods.pod_geoms(m)
    return ld_gap(name, ga[cs["tgt_a"]], gb[cs["tgt_b"]])


def host_pairs(name):
    """The product set in a's-major order, smaller type first: what the host test walks without an engine"""
    ga, gb = pods.pod_geoms(model_of(name))
    pairs = np.array([(x, y) for x in ga for y in gb], np.int32)
    ia = np.repeat(np.arange(len(ga)), len(gb))
    ib = np.tile(np.arange(len(gb)), len(ga))
    return pairs, ia, ib


def expected(name, pairs, ia, ib):
    """E [N, P] for the candidate table `pairs` (ia / ib: pose_pods.pair_table) and what goes with it: the NumPy
    statement everywhere, the longdouble statement on the target pair where its cores are apart"""
    cs, m, k = case_set(name), model_of(name), poses(name)
    Eref = ref.pair_distances(m, k["geom_xpos"], k["geom_xmat"], pairs)
    col = np.array([int(np.flatnonzero((ia == a) & (ib == b))[0]) for a, b in zip(cs["tgt_a"], cs["tgt_b"])])
    gap, core = target_ld(name)
    # (a box is its own core: box_box_dist holds for any disjoint boxes, so they count as apart at every gap)
    use = np.asarray(core > (0.0 if cs["t1"] == BOX else CORE_APART))
    E = Eref.copy()
    rows = np.arange(len(E))
    E[rows[use], col[use]] = gap[use].astype(np.float64)
    # core gaps of every entry: the target's in longdouble, the others' from the NumPy statement
    gs = np.asarray(m.geom_size, float).reshape(-1, 3)
    rad = _RAD[cs["t1"]](gs[pairs[:, 0]]) + _RAD[cs["t2"]](gs[pairs[:, 1]])
    coregap = np.maximum(Eref + rad[None, :], 0.0)
    if cs["t1"] == PLANE:
        coregap[:] = np.inf
    coregap[rows, col] = np.asarray(core, np.float64)
    return dict(E=E, Eref=Eref, col=col, use=use, gap=gap, core=core, coregap=coregap)


def verdicts(name, pairs, Eref):
    """touching (gap <= 0) by the longdouble predicates, [N, P].  Entries that the NumPy statement Eref puts more than
    CORE_APART from touching take its sign: the two statements agree within 1e-12 (tests/test_degenerate_cases_host.py),
    so the longdouble evaluation is spent on the rows where it can differ."""
    out = Eref <= 0
    for p, (g1, g2) in enumerate(pairs):
        r = np.flatnonzero(np.abs(Eref[:, p]) <= CORE_APART)
        if len(r):
            gap, _ = ld_gap(name, np.full(len(r), g1), np.full(len(r), g2), distance=False, rows=r)
            out[r, p] = np.asarray(gap <= 0)
    return out
