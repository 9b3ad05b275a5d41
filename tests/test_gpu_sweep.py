"""Certified edge checks on the GPU (include/mjpl_hip.h: mjpl_sweep_*): closed forms on hand-built scenes, the bubble
measurement against the NumPy statement (tests/sweep_reference.py) fed by Engine.distances, the loop against the NumPy
loop fed by Engine.sweep_measure, soundness of FREE and HIT against Engine.clearance and check_edges on the same
batches, shapes across the wave and the 64-edge chunk, both layouts and forms, argument errors, run-to-run identity.

The closed-form wall scene: the edge 0.8 -> 1.0 of a ball (r 0.01) through a wall 2 mm thick at x = 0.9.  Waypoints
0.05 apart on that edge are 0.85, 0.90, 0.95: the second one sits in the wall, so a sampled check at step 0.05 sees
the wall.  The point -- a sampled check that calls the edge valid while the sweep reports the hit -- is made at step
0.06 (waypoints 0.86, 0.92, 0.98; the ball touches for x in [0.889, 0.911])."""
import ctypes as C
import functools

import numpy as np
import pytest

import sweep_reference as sref
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import CertifiedIntervals, ClearanceConstraint, CollisionConstraint
from mjpl_amd.model import ModelBuilder
from test_sweep_host import MODELS as HOST_MODELS

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
FREE, HIT, UNDECIDED, NONFINITE, RANGE = (eng_mod.SWEEP_FREE, eng_mod.SWEEP_HIT, eng_mod.SWEEP_UNDECIDED,
                                          eng_mod.SWEEP_NONFINITE, eng_mod.SWEEP_RANGE)
NAMES = ("status", "t_hit", "clear_lb", "pair", "nodes", "depth")
DECISION = 1e-6  # (c): edges whose decision margins stay above this at every node are compared
EDGES, MAX_DEPTH, SEED = 192, 6, 5


def margins_of(e):
    pairs, allowed = e.contact_pairs()
    m = np.asarray(e.model.geom_margin, float)
    return pairs, allowed, np.maximum(m[pairs[:, 0]], m[pairs[:, 1]])


# ---- (a) closed forms
def wall_scene():
    mb = ModelBuilder()
    mb.add_body("ball", pos=(0, 0, 1))
    mb.add_joint("ball", "ball_slide_x", "slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("ball", "sphere", (0.01,))
    mb.add_geom("world", "box", (0.001, 0.5, 0.5), pos=(0.9, 0, 1), name="wall")
    return mb.compile()


def test_thin_wall_between_two_waypoints():
    e = eng_mod.Engine(wall_scene())
    kw = dict(cap=0.1, lo=[-2.0], hi=[2.0])
    assert e.check_edges(np.array([[0.8]]), np.array([[1.0]]), 0.06)[0] == 1  # the sampled check steps over the wall
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[0.8]]), np.array([[1.0]]), **kw)
    assert st[0] == HIT and t[0] == 0.5 and pair[0] == 0 and nodes[0] == 3 and depth[0] == 0 and np.isnan(lb[0])
    # free at the root: distance 0.049 at 0.84, the ball travels 0.04 either way
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[0.8]]), np.array([[0.88]]), **kw)
    assert st[0] == FREE and nodes[0] == 3 and depth[0] == 0 and pair[0] == -1 and np.isnan(t[0])
    assert abs(lb[0] - 0.009) <= 1e-12
    # a point
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[0.8]]), np.array([[0.8]]), **kw)
    assert st[0] == FREE and nodes[0] == 3 and depth[0] == 0 and abs(lb[0] - 0.089) <= 1e-12
    # max_depth 0: the root of 0.5 -> 0.88 sees the cap 0.1 and travels 0.19
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[0.5]]), np.array([[0.88]]), max_depth=0, **kw)
    assert st[0] == UNDECIDED and nodes[0] == 3 and depth[0] == 0 and np.isnan(lb[0]) and np.isnan(t[0]) and pair[0] == -1
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[0.5]]), np.array([[0.88]]), **kw)
    assert st[0] == FREE and 0 < lb[0] <= 0.009 + 1e-12 and depth[0] >= 1 and nodes[0] > 3
    # d_min: 0.8 -> 0.88 ends 0.009 from the wall
    st = e.sweep_edges(np.array([[0.8]]), np.array([[0.88]]), 0.01, **kw)[0]
    assert st[0] == HIT
    # the measurement itself: a box of half-width 0.04 around 0.84
    slack, sp, gap, gp = e.sweep_measure(np.array([[0.84]]), np.array([[0.04]]), 0.1)
    assert abs(slack[0] - 0.009) <= 1e-12 and abs(gap[0] - 0.049) <= 1e-12 and sp[0] == 0 and gp[0] == 0


def arm_scene():
    """A sphere (r 0.05) 0.5 out on a hinge about z; static spheres (r 0.02) at (0.6, 0, 0) and (r 0.04) at (0, 0.58, 0)."""
    mb = ModelBuilder()
    mb.add_body("arm")
    mb.add_joint("arm", "swing", "hinge", axis=(0, 0, 1), range=(-3, 3))
    mb.add_geom("arm", "sphere", (0.05,), pos=(0.5, 0, 0))
    mb.add_geom("world", "sphere", (0.02,), pos=(0.6, 0, 0))
    mb.add_geom("world", "sphere", (0.04,), pos=(0, 0.58, 0))
    return mb.compile()


def test_sphere_on_a_hinge_arm_passing_small_spheres():
    e = eng_mod.Engine(arm_scene())
    pairs, _ = e.contact_pairs()
    W = e.sweep_levers()
    assert W.shape == (2, 1) and np.all(np.abs(W - 0.55) <= 1e-15)  # |geom_pos| + rbound
    d1 = lambda th: np.sqrt(0.25 + 0.36 - 0.6 * np.cos(th)) - 0.07
    # -0.2 -> 0.2 passes the first sphere at 0.03: the root and depth 1 are not certified, depth 2 is
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[-0.2]]), np.array([[0.2]]), cap=0.2)
    assert st[0] == FREE and nodes[0] == 3 + 2 + 4 and depth[0] == 2
    assert abs(lb[0] - (d1(0.05) - 0.05 * 0.55)) <= 1e-12
    # the second sphere is touched around pi / 2: at the root ...
    h = np.pi / 2
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[h - 0.4]]), np.array([[h + 0.4]]), cap=0.2)
    big = int(np.flatnonzero(np.asarray(e.model.geom_size).reshape(-1, 3)[:, 0] == 0.04)[0])  # the r 0.04 sphere's pair
    second = int(np.flatnonzero((pairs == big).any(axis=1))[0])
    assert st[0] == HIT and t[0] == 0.5 and nodes[0] == 3 and depth[0] == 0 and pair[0] == second
    # ... and at depth 1, t = 3/4 (the root, at pi / 2 - 0.1, is 6.4 mm clear)
    st, t, lb, pair, nodes, depth = e.sweep_edges(np.array([[h - 0.4]]), np.array([[h + 0.2]]), cap=0.2)
    assert st[0] == HIT and t[0] == 0.75 and nodes[0] == 5 and depth[0] == 1 and pair[0] == second


# ---- the batches of (b), (c), (d): the models of the host test, Franka with pads in place of two_dof_ball
def gpu_models():
    out = [x for x in HOST_MODELS if x[0] != "two_dof_ball"]
    mp = scenes.franka_p(True, True)
    qidx = scenes.planning_index(mp, scenes.FRANKA_ARM_JOINTS).astype(np.int32)
    rng = np.asarray(mp.jnt_range, float)[qidx]
    out.insert(2, ("franka_p+16obs+pads, arm", mp, (), qidx, mp.keyframe("home").qpos.copy(), rng[:, 0].copy(), rng[:, 1].copy()))
    return out


MODELS = gpu_models()
IDS = [x[0] for x in MODELS]


def sweep_batch(lo, hi, n=EDGES, seed=SEED):
    """n edges inside [lo, hi]: half of length 0.05, half of length up to 2 (before clipping)."""
    rng = np.random.default_rng(seed)
    qa = rng.uniform(lo, hi, size=(n, len(lo)))
    d = rng.normal(size=qa.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = np.where(np.arange(n) % 2 == 0, 0.05, rng.uniform(0.05, 2.0, size=n))
    return qa, np.clip(qa + length[:, None] * d, lo, hi)


@functools.lru_cache(maxsize=None)
def engine_of(k):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = eng_mod.Engine(m, allowed)
    e.set_planning(qidx, base)
    return e


def cap_of(e, d_min):
    return d_min + e.sweep_margin_max() + 0.25


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_measure_equals_the_numpy_statement(k):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    e.sweep_bounds(lo, hi)
    pairs, flags, margins = margins_of(e)
    W = e.sweep_levers(lo, hi)
    QA, QB = sweep_batch(lo, hi, 130)
    rng = np.random.default_rng(3)
    HD = np.abs(QB - QA) * rng.uniform(0, 0.5, size=(len(QA), 1))
    HD[::7] = 0.0
    HD[1::7, 0] = 0.0
    cap = cap_of(e, 0.0)
    want = sref.bubble(e.distances(QA), margins, flags, W, HD, cap)
    got = e.sweep_measure(QA, HD, cap)
    worst = max(float(np.max(np.abs(got[0] - want[0]))), float(np.max(np.abs(got[2] - want[2]))))
    print(f"{name}: largest |slack or gap - NumPy| = {worst:.3e}")
    assert worst <= 1e-9
    # gap is mjpl_clearance at distmax = cap, byte for byte, whatever HD; and with HD = 0 slack is gap
    clear, cpair = e.clearance(QA, cap)
    assert got[2].tobytes() == clear.tobytes() and got[3].tobytes() == cpair.tobytes()
    z = e.sweep_measure(QA, np.zeros_like(QA), cap)
    assert z[2].tobytes() == clear.tobytes() and z[0].tobytes() == clear.tobytes() and z[1].tobytes() == cpair.tobytes()
    # SoA and the device form
    s = e.sweep_measure(np.ascontiguousarray(QA.T), np.ascontiguousarray(HD.T), cap, eng_mod.SOA)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(s, got))


@functools.lru_cache(maxsize=None)
def swept(k, d_min):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    QA, QB = sweep_batch(lo, hi)
    cap = cap_of(e, d_min)
    got = e.sweep_edges(QA, QB, d_min, cap=cap, max_depth=MAX_DEPTH, lo=lo, hi=hi)
    return QA, QB, cap, got


@pytest.mark.parametrize("d_min", [0.0, 0.01])
@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_edges_equal_the_numpy_loop(k, d_min):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    QA, QB, cap, got = swept(k, d_min)
    want = sref.sweep_edges(lambda Q, HD: e.sweep_measure(Q, HD, cap), QA, QB, d_min, MAX_DEPTH, lo, hi)
    cmp = want["margin"] > DECISION
    out = int((~cmp).sum())
    st = got[0]
    print(f"{name}, d_min {d_min}: {out} of {len(cmp)} edges left out; FREE {int((st == FREE).sum())}, HIT "
          f"{int((st == HIT).sum())}, UNDECIDED {int((st == UNDECIDED).sum())}; nodes per edge {got[4].mean():.1f}")
    assert out <= 0.05 * len(cmp)
    for name_, a in zip(NAMES, got):
        b = want[name_]
        if name_ == "clear_lb":
            assert a[cmp].tobytes() == b[cmp].tobytes(), name_
        else:
            assert np.array_equal(a[cmp], b[cmp], equal_nan=True), name_


@pytest.mark.parametrize("d_min", [0.0, 0.01])
@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_free_edges_are_free_and_hits_are_hits(k, d_min):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    QA, QB, cap, (st, t_hit, lb, pair, nodes, depth) = swept(k, d_min)
    free, hit = np.flatnonzero(st == FREE), np.flatnonzero(st == HIT)
    assert len(free) + len(hit) > 0
    if len(free):
        t = np.linspace(0.0, 1.0, 257)
        rows = QA[free][:, None, :] + t[None, :, None] * (QB[free] - QA[free])[:, None, :]
        clear = e.clearance(rows.reshape(-1, rows.shape[-1]), cap)[0].reshape(len(free), len(t))
        assert np.all(clear >= d_min)
        assert np.all(clear >= lb[free][:, None] - 1e-9)
        assert np.all(lb[free] > 0) and np.all(lb[free] <= cap)
        assert e.check_edges(QA[free], QB[free], 0.01).all()
    if len(hit):
        at = QA[hit] + t_hit[hit][:, None] * (QB[hit] - QA[hit])
        at[t_hit[hit] == 1.0] = QB[hit][t_hit[hit] == 1.0]  # (the end point's node is QB itself)
        clear, cp = e.clearance(at, cap)
        assert np.all((clear <= 0) | (clear < d_min))
        assert np.array_equal(cp, pair[hit])


# ---- (e) shapes and arguments
@pytest.mark.parametrize("E", [1, 63, 65, 200])
def test_shapes_layouts_and_forms(E):
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    QA, QB = sweep_batch(lo, hi, E, seed=9)
    kw = dict(cap=cap_of(e, 0.0), max_depth=16, lo=lo, hi=hi)  # (max_depth 16: chunks of 64 edges)
    got = e.sweep_edges(QA, QB, **kw)
    again = e.sweep_edges(QA, QB, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two identical calls, identical bytes"
    soa = e.sweep_edges(np.ascontiguousarray(QA.T), np.ascontiguousarray(QB.T), layout=eng_mod.SOA, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, soa))
    # every edge alone gives what it gives in the batch (chunks and packing change nothing)
    for i in (0, E - 1):
        one = e.sweep_edges(QA[i:i + 1], QB[i:i + 1], **kw)
        assert all(a.tobytes() == b[i:i + 1].tobytes() for a, b in zip(one, got))
    # the device form
    nplan = QA.shape[1]
    dA, dB = e.alloc(QA.nbytes).upload(QA), e.alloc(QB.nbytes).upload(QB)
    outs = [e.alloc(E * (4 if n in ("status", "pair", "nodes", "depth") else 8)) for n in NAMES]
    e.sweep_edges_dev(dA.ptr, dB.ptr, E, eng_mod.AOS, 0.0, *[o.ptr for o in outs], **kw)
    for n, o, a in zip(NAMES, outs, got):
        assert o.download(a.dtype, E).tobytes() == a.tobytes(), n
    for b in (dA, dB, *outs):
        b.free()
    assert nplan == len(lo)


def test_nonfinite_and_range_edges():
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    QA, QB = sweep_batch(lo, hi, 8, seed=2)
    ref = e.sweep_edges(QA, QB, lo=lo, hi=hi)
    A, B = QA.copy(), QB.copy()
    A[1, 2] = np.nan
    B[3, 0] = np.inf
    B[5, 1] = hi[1] + 1e-3
    A[6, 0] = lo[0] - 1e-3
    st, t, lb, pair, nodes, depth = e.sweep_edges(A, B, lo=lo, hi=hi)
    assert list(st[[1, 3, 5, 6]]) == [NONFINITE, NONFINITE, RANGE, RANGE]
    for i in (1, 3, 5, 6):
        assert np.isnan(t[i]) and np.isnan(lb[i]) and pair[i] == -1 and nodes[i] == 0 and depth[i] == 0
    for i in (0, 2, 4, 7):  # the others as without them
        assert all(a[i:i + 1].tobytes() == b[i:i + 1].tobytes() for a, b in zip((st, t, lb, pair, nodes, depth), ref))
    # without bounds the same edges are measured
    assert list(e.sweep_edges(A[[5, 6]], B[[5, 6]])[0]) != [RANGE, RANGE]
    # a non-finite row of the measurement
    Q = QA[:2].copy()
    Q[1, 0] = np.nan
    slack, sp, gap, gp = e.sweep_measure(Q, np.zeros_like(Q), 0.3)
    assert np.isnan(slack[1]) and np.isnan(gap[1]) and sp[1] == -1 and gp[1] == -1 and np.isfinite(slack[0])


def test_argument_refusals():
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    QA, QB = sweep_batch(lo, hi, 4, seed=2)
    mm = e.sweep_margin_max()
    bad = [dict(d_min=-1e-3), dict(d_min=float("nan")), dict(cap=float("nan")), dict(cap=mm), dict(d_min=0.1, cap=0.1 + mm),
           dict(cap=float("inf")), dict(max_depth=-1), dict(max_depth=17), dict(lo=np.full(len(lo), np.nan)),
           dict(lo=hi + 1.0, hi=hi)]
    for kw in bad:
        with pytest.raises(eng_mod.MjplError) as ei:
            e.sweep_edges(QA, QB, **kw)
        assert ei.value.code == E_ARG, kw
    for kw in (dict(cap=0.0), dict(cap=float("nan")), dict(cap=float("inf"))):
        with pytest.raises(eng_mod.MjplError) as ei:
            e.sweep_measure(QA, np.zeros_like(QA), **kw)
        assert ei.value.code == E_ARG, kw
    with pytest.raises(eng_mod.MjplError):
        e.sweep_bounds(lo=hi + 1.0, hi=hi)
    F, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    desc, keep = e.sweep_desc()
    st, i32, f64 = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4)
    p = lambda a, T: a.ctypes.data_as(T)
    args = [p(st, I), p(f64, F), p(f64, F), p(i32, I), p(i32, I), p(i32, I)]
    assert e.lib.mjpl_sweep_edges(e.h, None, p(QA, F), p(QB, F), 4, eng_mod.AOS, *args) == E_ARG
    assert e.lib.mjpl_sweep_edges(e.h, C.byref(desc), p(QA, F), None, 4, eng_mod.AOS, *args) == E_ARG
    assert e.lib.mjpl_sweep_edges(e.h, C.byref(desc), p(QA, F), p(QB, F), 4, 7, *args) == E_ARG
    assert e.lib.mjpl_sweep_edges(e.h, C.byref(desc), p(QA, F), p(QB, F), 4, eng_mod.AOS, None, *args[1:]) == E_ARG
    assert e.lib.mjpl_sweep_edges(e.h, C.byref(desc), p(QA, F), p(QB, F), 0, eng_mod.AOS, *([None] * 6)) == 0


# ---- the constraints and the adapter
def test_constraints_and_the_adapter():
    m = wall_scene()
    cc = CollisionConstraint(m)
    a, b = np.array([0.8]), np.array([1.0])
    r = cc.certified_interval(a, b, cap=0.1, lo=[-2.0], hi=[2.0])
    assert r.status == HIT and r.t_hit == 0.5 and r.pair == tuple(int(g) for g in cc.engine.contact_pairs()[0][0])
    assert cc.valid_interval(a, b, 0.06)  # sampled: steps over the wall
    ci = CertifiedIntervals(cc, cap=0.1, lo=[-2.0], hi=[2.0])
    assert not ci.valid_interval(a, b, 0.06) and ci.valid_interval(a, np.array([0.88]), 0.06)
    assert list(ci.valid_intervals(np.array([[0.8], [0.8]]), np.array([[1.0], [0.88]]), 0.06)) == [False, True]
    with pytest.raises(ValueError):
        ci.valid_interval(a, b, 0.0)
    cl = ClearanceConstraint(cc, 0.01, lower=[-2.0], upper=[2.0])
    assert cl.certified_interval(a, np.array([0.88]), cap=0.1).status == HIT  # ends 0.009 from the wall
    assert cl.certified_interval(a, np.array([0.87]), cap=0.1).status == FREE
    assert not CertifiedIntervals(cl, cap=0.1).valid_interval(a, np.array([0.88]), 0.05)
    st = cc.certified_edges_planning(np.array([[0.8]]), np.array([[0.88]]), cap=0.1, lo=[-2.0], hi=[2.0])[0]
    assert st[0] == FREE
