"""Any pose pair through the engine: two six-joint pods (or a tilted static plane and one pod) whose tip geoms
can be put at any world pose by the configuration alone.  Shared by tests/degenerate_cases.py,
tests/test_degenerate_cases_host.py and tests/test_gpu_degenerate_poses.py.

The pod is the `_pod` of tests/test_gpu_filter_adversarial.py with every offset zero: six one-joint bodies from the
world (slides x, y, z, then hinges x, y, z), all body positions 0, joint ranges +-10, and G geoms of one type with
different sizes on the tip body at local pose identity.  A tip geom's centre is then the three slide values and its
frame Rx(a) Ry(b) Rz(c) of the three hinge values.
"""
import numpy as np

from mjpl_amd.model import ModelBuilder

PLANE, SPHERE, CAPSULE, BOX = 0, 2, 3, 6
TYPE_NAME = {PLANE: "plane", SPHERE: "sphere", CAPSULE: "capsule", BOX: "box"}
_NSIZE = {SPHERE: 1, CAPSULE: 2, BOX: 3}
RANGE = 10.0


def _pod(mb, name, gtype, sizes):
    parent = "world"
    axes = [("slide", (1, 0, 0)), ("slide", (0, 1, 0)), ("slide", (0, 0, 1)),
            ("hinge", (1, 0, 0)), ("hinge", (0, 1, 0)), ("hinge", (0, 0, 1))]
    for k, (jt, ax) in enumerate(axes):
        body = f"{name}{k}"
        mb.add_body(body, parent=parent, pos=(0, 0, 0))
        mb.add_joint(body, f"{name}_j{k}", jt, axis=ax, range=(-RANGE, RANGE))
        parent = body
    for i, s in enumerate(np.atleast_2d(np.asarray(sizes, float))):
        mb.add_geom(parent, TYPE_NAME[gtype], tuple(s[:_NSIZE[gtype]]), name=f"{name}_g{i}")


def two_pod_model(type_a, sizes_a, type_b, sizes_b):
    """Pods a and b with the geoms sizes_a [Ga, 3] of type_a and sizes_b [Gb, 3] of type_b: Ga x Gb candidate pairs,
    12 configuration columns (a's slides and hinges, then b's)."""
    mb = ModelBuilder()
    _pod(mb, "a", type_a, sizes_a)
    _pod(mb, "b", type_b, sizes_b)
    return mb.compile()


def plane_pod_model(plane_pos, plane_quat, type_b, sizes_b):
    """A plane on the world at the given pose (planes only occur as the static partner) and pod b: Gb candidate
    pairs, 6 configuration columns."""
    mb = ModelBuilder()
    mb.add_geom("world", "plane", (0, 0, 0.1), pos=tuple(plane_pos), quat=tuple(plane_quat), name="a_g0")
    _pod(mb, "b", type_b, sizes_b)
    return mb.compile()


def pod_geoms(model):
    """(geom ids of a, geom ids of b), each in the order of the sizes handed to the model's maker"""
    out = []
    for name in "ab":
        ids, i = [], 0
        while True:
            try:
                ids.append(int(model.geom(f"{name}_g{i}").id))
            except (KeyError, ValueError, IndexError):
                break
            i += 1
        out.append(np.array(ids))
    return out[0], out[1]


def rot_xyz(ang):
    """Rx(a) Ry(b) Rz(c) [N, 3, 3] of the hinge values ang [N, 3]"""
    a, b, c = np.asarray(ang).T
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.stack([np.stack([cb * cc, -cb * sc, sb], 1),
                     np.stack([ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb], 1),
                     np.stack([sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb], 1)], 1)


def euler_xyz(R):
    """Hinge values [N, 3] with Rx(a) Ry(b) Rz(c) = R [N, 3, 3] (away from cos b = 0)"""
    R = np.asarray(R, float)
    b = np.arctan2(R[:, 0, 2], np.hypot(R[:, 0, 0], R[:, 0, 1]))
    a = np.arctan2(-R[:, 1, 2], R[:, 2, 2])
    c = np.arctan2(-R[:, 0, 1], R[:, 0, 0])
    return np.stack([a, b, c], 1)


def configs(p1, R1, p2, R2):
    """Q [N, 12] that puts pod a's tip at (p1, R1) and pod b's at (p2, R2); Q [N, 6] for the plane model
    (p1 = R1 = None).  Rows whose two matrices are the same bits get the same three hinge values."""
    qb = np.concatenate([np.asarray(p2, float), euler_xyz(R2)], 1)
    if p1 is None:
        return qb
    Q = np.concatenate([np.asarray(p1, float), euler_xyz(R1), qb], 1)
    assert np.abs(Q).max() < RANGE
    return Q


def fk(model, Q):
    """The CPU oracle's forward kinematics: what every expected value is computed from"""
    from oracle import pyoracle
    return pyoracle.Oracle(model).fk(np.asarray(Q, float))


def product_pairs(model):
    """The candidate pairs the model must have, as a set of (smaller id, larger id): every geom of a with every
    geom of b"""
    ga, gb = pod_geoms(model)
    return {(min(int(x), int(y)), max(int(x), int(y))) for x in ga for y in gb}


def pair_table(engine, model):
    """Engine.contact_pairs() of a pod model -> (pairs [P, 2], ia [P], ib [P]): ia / ib = which of a's / b's geoms the
    row holds.  Asserts that the table is exactly the product set: the model compiler's pruning passes must not have
    dropped a pair, and none is allowed."""
    pairs, allowed = engine.contact_pairs()
    ga, gb = pod_geoms(model)
    have = [(min(int(x), int(y)), max(int(x), int(y))) for x, y in pairs]
    assert len(set(have)) == len(have) and set(have) == product_pairs(model), (have, sorted(product_pairs(model)))
    assert not allowed.any()
    gt = np.asarray(model.geom_type)
    assert np.all(gt[pairs[:, 0]] <= gt[pairs[:, 1]])
    ia, ib = np.zeros(len(pairs), int), np.zeros(len(pairs), int)
    for p, (x, y) in enumerate(pairs):
        xa = x if x in ga else y
        yb = y if xa == x else x
        ia[p], ib[p] = int(np.flatnonzero(ga == xa)[0]), int(np.flatnonzero(gb == yb)[0])
    return pairs, ia, ib
