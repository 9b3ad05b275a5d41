"""Push-out on the GPU (include/mjpl_hip.h: mjpl_push_out*; ClearanceConstraint): closed forms on hand-built scenes,
the status rule, clear and pair against mjpl_clearance bit for bit, the NumPy statement of tests/push_reference.py fed
by the engine's own near pairs, shapes across the wave, the block and the 2^16-row chunk, the entry points' forms and
argument errors, run-to-run identity, and the constraint in apply_constraints and in RRT."""
import ctypes as C
import functools

import numpy as np
import pytest

import distance_reference as ref
import push_reference as pref
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import (ClearanceConstraint, CollisionConstraint, JointLimitConstraint, apply_constraints,
                                 obeys_constraints)
from mjpl_amd.planning import RRT
from helpers import uniform_configs
from test_gpu_clearance_grad import g, one_pair, quat
from test_gpu_models import random_model
from test_gpu_near_pairs import two_walls
from test_push_out_host import PUSH_DMIN, PUSH_K, PUSH_ROWS, PUSH_SEED, PUSH_SHARE

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
OK, STUCK, DEGENERATE, NONFINITE = eng_mod.PUSH_OK, eng_mod.PUSH_STUCK, eng_mod.PUSH_DEGENERATE, eng_mod.PUSH_NONFINITE
OVERSHOOT, DAMPING, MAX_ITER = 1e-3, 1e-4, 16  # the defaults
F, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
NAMES = ("Q_out", "clear", "pair", "iters", "status")

# 6(e), 7: |Q_out - the NumPy statement fed by engine.near_pairs| over the rows whose decision margin stays above
# DECISION at every iteration.  Measured at the first run on an MI355X: MEASURED_E, the largest over the seven models
# and the 65 537-row case (Franka-P + obstacles; the others 1.2e-11 and below); the bound is 100 times that, 3.157e-9,
# and no more than 1e-6.
DECISION = 1e-6
MEASURED_E = 3.157e-11
TOL_E = min(100 * MEASURED_E, 1e-6)
TOL_FIRST_STEP = 1e-9  # one step against the statement: the project's bound for NumPy statements


def push(e, Q, d_min, **kw):
    return e.push_out(np.atleast_2d(np.asarray(Q, float)), d_min, **kw)


# ---- 1. closed form, one step
def test_sphere_on_slide_facing_box_one_step():
    for sgn in (1.0, -1.0):
        m = one_pair(g("box", (0.2, 0.2, 0.2)), g("sphere", (0.1,), (0.5, 0, 0)), axis=(sgn, 0, 0))
        e = eng_mod.Engine(m)
        Qo, clear, pair, iters, st = push(e, [[0.0]], 0.3)
        want = sgn * (0.1 + OVERSHOOT) / (1 + DAMPING)
        assert abs(Qo[0, 0] - want) <= 1e-12
        assert st[0] == OK and iters[0] == 1 and pair[0] == 0 and clear[0] >= 0.3
    # the bound stops the push: the last iterate is the bound itself
    m = one_pair(g("box", (0.2, 0.2, 0.2)), g("sphere", (0.1,), (0.5, 0, 0)), axis=(1.0, 0, 0))
    e = eng_mod.Engine(m)
    Qo, clear, pair, iters, st = push(e, [[0.0]], 0.3, hi=[0.05])
    assert Qo[0, 0] == 0.05 and st[0] == STUCK and iters[0] == MAX_ITER and clear[0] < 0.3


# ---- 2. two walls (faces at -1 and +1, sphere r = 0.1)
def test_two_walls():
    e = eng_mod.Engine(two_walls())
    Q = np.array([[0.0]])
    Qo, clear, pair, iters, st = push(e, Q, 0.5)
    assert Qo.tobytes() == Q.tobytes() and iters[0] == 0 and st[0] == OK
    # one step of 0.4 + overshoot: step_max must admit it (the default 0.2 would cut it in two)
    Qo, clear, pair, iters, st = push(e, [[0.8]], 0.5, step_max=1.0)
    assert abs(Qo[0, 0] - (0.8 - (0.4 + OVERSHOOT) / (1 + DAMPING))) <= 1e-12
    assert iters[0] == 1 and st[0] == OK
    # no configuration is 0.95 from both walls.  Without overshoot the damping leaves the pushed wall a little short,
    # both walls stay violated and the iteration settles between them
    Qo, clear, pair, iters, st = push(e, [[0.3]], 0.95, overshoot=0.0)
    assert st[0] == STUCK and iters[0] == MAX_ITER and abs(Qo[0, 0]) <= 1e-6 and clear[0] < 0.95
    # ... with the default overshoot every step satisfies one wall, which then takes no part in the next: the row
    # alternates between the two answers, 0.05 + overshoot from the middle, and ends as it stands
    Qo, clear, pair, iters, st = push(e, [[0.3]], 0.95)
    assert st[0] == STUCK and iters[0] == MAX_ITER and abs(abs(Qo[0, 0]) - 0.051) <= 1e-4 and clear[0] < 0.95


# ---- 3. capsule on a hinge above a plane
def test_capsule_on_hinge_above_plane():
    m = one_pair(g("plane", (1, 1, 0.1)), g("capsule", (0.05, 0.2), q=quat((0, 1, 0), np.pi / 2)),
                 jtype="hinge", axis=(0, 1, 0), body_pos=(0, 0, 0.5))
    e = eng_mod.Engine(m)
    Qo, clear, pair, iters, st = push(e, [[1.2]], 0.35)
    want = 0.45 - 0.2 * abs(np.sin(Qo[0, 0]))
    assert st[0] == OK and want >= 0.35 and 1 <= iters[0] <= 8
    # clear is mjpl_clearance at distmax D* = 0.35, so it reads the cap; the uncapped clearance is the closed form
    assert abs(clear[0] - min(want, 0.35)) <= 1e-12
    assert abs(e.clearance(Qo)[0][0] - want) <= 1e-12


# ---- 4. concentric spheres: no normal, no step
def test_concentric_spheres_are_degenerate():
    m = one_pair(g("sphere", (0.1,)), g("sphere", (0.1,)))
    e = eng_mod.Engine(m)
    Q = np.array([[0.0]])
    Qo, clear, pair, iters, st = push(e, Q, 0.05)
    assert st[0] == DEGENERATE and Qo.tobytes() == Q.tobytes() and iters[0] == 0 and clear[0] < 0.05


# ---- 6. models
def _model_cases():
    yield "franka_p", scenes.franka_p(obstacles=True), (), PUSH_DMIN, PUSH_ROWS
    yield "franka_pads", scenes.franka_p(obstacles=True, pads=True), (), PUSH_DMIN, 96
    yield "ur5e", scenes.ur5e(), (), PUSH_DMIN, 96
    for seed in range(4):
        m, allowed = random_model(seed)
        yield f"random{seed}", m, tuple(allowed), 0.01, 96


MODELS = {c[0]: c for c in _model_cases()}


@functools.lru_cache(maxsize=None)
def model_setup(label):
    """(model, engine, Q, margins, allowed flags, d_min, D*): made once per model"""
    _, m, allowed, d_min, rows = MODELS[label]
    e = eng_mod.Engine(m, list(allowed))
    if label.startswith("franka"):
        Q = uniform_configs(m, rows, seed=PUSH_SEED)
    else:
        Q = np.random.default_rng(PUSH_SEED).uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(rows, m.nq))
    pairs, flags = e.contact_pairs()
    margins = ref.pair_margins(m, pairs)
    dstar = d_min + (margins[~flags].max() if (~flags).any() else 0.0)
    Q.setflags(write=False)
    return m, e, Q, margins, flags, d_min, dstar


@functools.lru_cache(maxsize=None)
def model_run(label):
    """push_out with the defaults: made once per model, shared and left unchanged"""
    m, e, Q, margins, flags, d_min, dstar = model_setup(label)
    out = e.push_out(Q, d_min)
    for a in out:
        a.setflags(write=False)
    return out


def check_abc(e, Q, out, d_min, dstar):
    """(a) clear and pair are mjpl_clearance(Q_out, D*); (b) OK <=> clear >= d_min; (c) rows that hold are untouched"""
    Qo, clear, pair, iters, st = out
    C_, cp = e.clearance(Qo, dstar)
    assert clear.tobytes() == C_.tobytes() and pair.tobytes() == cp.tobytes()
    assert np.array_equal(st == OK, clear >= d_min)
    assert np.all(st != NONFINITE) and np.all((iters >= 0) & (iters <= MAX_ITER))
    start = e.clearance(Q, dstar)[0]
    holds = start >= d_min
    assert Qo[holds].tobytes() == Q[holds].tobytes() and np.all(iters[holds] == 0) and np.all(st[holds] == OK)
    return ~holds


def near_of(e, dstar, K):
    def near(S):
        count, pair, dist, grad, _ft, _n, status = e.near_pairs(S, dstar, K)
        return count, pair, dist, grad, status
    return near


def check_e(label, e, Q, Qo, needing, margins, d_min, dstar, **kw):
    """(e) Q_out against the NumPy statement fed by engine.near_pairs, on the rows with a clear decision margin"""
    want, _it, _deg, decision, _w = pref.push_out(near_of(e, dstar, PUSH_K), Q, margins, d_min, **kw)
    kept = needing & np.all(decision > DECISION, axis=1)
    left_out = int((needing & ~kept).sum())
    err = float(np.abs(Qo[kept] - want[kept]).max()) if kept.any() else 0.0
    print(f"{label}: needing {int(needing.sum())}, left out {left_out}, |Q_out - statement| = {err:.3e}")
    assert left_out <= 0.1 * needing.sum(), (label, left_out, int(needing.sum()))
    return err


@pytest.mark.parametrize("label", list(MODELS))
def test_models(label):
    m, e, Q, margins, flags, d_min, dstar = model_setup(label)
    out = model_run(label)
    needing = check_abc(e, Q, out, d_min, dstar)
    if label == "franka_p":
        conv = (out[4] == OK) & needing
        print(f"franka_p: converged {int(conv.sum())} of {int(needing.sum())}, most steps {int(out[3][conv].max())}")
        assert conv.sum() >= PUSH_SHARE * needing.sum(), (int(conv.sum()), int(needing.sum()))
    err = check_e(label, e, Q, out[0], needing, margins, d_min, dstar)
    assert err <= TOL_E, f"{label}: |Q_out - statement| = {err:.3e}"
    # a first step alone
    first = e.push_out(Q, d_min, max_iter=1)
    assert np.all(first[3] <= 1)
    want, *_ = pref.push_out(near_of(e, dstar, PUSH_K), Q, margins, d_min, max_iter=1)
    err1 = float(np.abs(first[0] - want).max())
    print(f"{label}: first step |Q_out - statement| = {err1:.3e}")
    assert err1 <= TOL_FIRST_STEP, f"{label}: first step off by {err1:.3e}"


# ---- 5. non-finite rows among finite ones
def test_nonfinite_rows():
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    want = model_run("franka_p")
    Qb = Q.copy()
    Qb[3, 2], Qb[77, 0] = np.nan, np.inf
    got = e.push_out(Qb, d_min)
    bad = np.zeros(len(Q), bool)
    bad[[3, 77]] = True
    assert np.all(got[4][bad] == NONFINITE) and got[0][bad].tobytes() == Qb[bad].tobytes()
    assert np.isnan(got[1][bad]).all() and np.all(got[2][bad] == -1) and np.all(got[3][bad] == 0)
    # their neighbours equal a run without them
    alone = e.push_out(Qb[~bad], d_min)
    for a, b, c in zip(got, alone, want):
        assert a[~bad].tobytes() == b.tobytes() and a[~bad].tobytes() == c[~bad].tobytes()


# ---- 7. shapes
@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_rows_do_not_depend_on_the_batch(n):
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    want = model_run("franka_p")
    Qn = uniform_configs(m, n, seed=PUSH_SEED)
    k = min(n, PUSH_ROWS)
    assert np.array_equal(Qn[:k], Q[:k])  # (uniform_configs draws row by row)
    got = e.push_out(Qn, d_min)
    for name, a, b in zip(NAMES, got, want):
        assert a[:k].tobytes() == b[:k].tobytes(), name
    check_abc(e, Qn, got, d_min, dstar)


def test_two_chunks_of_the_two_wall_scene():
    m = two_walls()
    e = eng_mod.Engine(m)
    n, d_min = 65537, 0.3
    Q = np.random.default_rng(11).uniform(-0.85, 0.85, size=(n, 1))
    out = e.push_out(Q, d_min)
    assert np.all(out[4] == OK)
    margins = ref.pair_margins(m, e.contact_pairs()[0])
    needing = check_abc(e, Q, out, d_min, d_min + margins.max())
    assert 0.2 < needing.mean() < 0.4
    err = check_e("two walls", e, Q, out[0], needing, margins, d_min, d_min + margins.max())
    assert err <= TOL_E, f"two walls: |Q_out - statement| = {err:.3e}"
    # the row of the second chunk equals a call of its own
    alone = e.push_out(Q[65536:], d_min)
    for a, b in zip(out, alone):
        assert a[65536:].tobytes() == b.tobytes()


# ---- 8. entry points
SENT_F, SENT_I = -12345.678, 777


def raw_call(e, Q, d_min, layout=eng_mod.AOS, fn=None, **params):
    """mjpl_push_out on host arrays pre-filled with a sentinel -> (rc, arrays in NAMES order)"""
    Q = np.ascontiguousarray(Q, float)
    n = Q.shape[0] if layout == eng_mod.AOS else Q.shape[1]
    out = [np.full(Q.shape, SENT_F), np.full(n, SENT_F), np.full(n, SENT_I, np.int32), np.full(n, SENT_I, np.int32),
           np.full(n, SENT_I, np.int32)]
    desc, keep = e.push_desc(d_min, **params)
    p = [a.ctypes.data_as(I if a.dtype == np.int32 else F) for a in out]
    rc = (fn or e.lib.mjpl_push_out)(e.h, C.byref(desc), Q.ctypes.data_as(F), n, layout, *p)
    del keep
    return rc, out


def dev_call(e, Q, n, layout, d_min, **params):
    Q = np.ascontiguousarray(Q, float)
    dQ = e.alloc(max(Q.nbytes, 8)).upload(Q)
    shapes = [(Q.shape, np.float64), ((n,), np.float64), ((n,), np.int32), ((n,), np.int32), ((n,), np.int32)]
    bufs = [e.alloc(max(int(np.prod(s)) * np.dtype(t).itemsize, 8)) for s, t in shapes]
    e.push_out_dev(dQ.ptr, n, layout, d_min, *[b.ptr for b in bufs], **params)
    out = [b.download(t, int(np.prod(s))).reshape(s) for b, (s, t) in zip(bufs, shapes)]
    for b in [dQ, *bufs]:
        b.free()
    return out


def test_layouts_and_forms_agree():
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    want = model_run("franka_p")
    rc, aos = raw_call(e, Q, d_min)
    assert rc == 0
    rc, soa = raw_call(e, Q.T, d_min, eng_mod.SOA)
    assert rc == 0
    dev_aos = dev_call(e, Q, len(Q), eng_mod.AOS, d_min)
    dev_soa = dev_call(e, Q.T, len(Q), eng_mod.SOA, d_min)
    assert soa[0].shape == (m.nq, len(Q))
    for k, name in enumerate(NAMES):
        for got in (aos, dev_aos):
            assert got[k].tobytes() == want[k].tobytes(), name
        for got in (soa, dev_soa):
            assert (got[k].T if k == 0 else got[k]).tobytes() == want[k].tobytes(), name


def test_planning_columns_against_the_full_run():
    """Seven arm columns against the full-nq run with the fingers pinned by the bounds.  The full run solves 9 x 9
    normal equations and clamps afterwards, so the two runs follow the same iteration only on rows where no violated
    pair's distance moves with a finger (its gradient is exactly 0 in both finger columns, at every iteration): the
    NumPy statement on the full run's near pairs picks those rows, and on them the arm columns agree."""
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    arm = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    fingers = np.setdiff1d(np.arange(m.nq), arm)
    assert len(arm) == 7 and np.all(Q[:, fingers] == Q[0, fingers])
    lo, hi = np.full(m.nq, -np.inf), np.full(m.nq, np.inf)
    lo[fingers] = hi[fingers] = Q[0, fingers]
    c = CollisionConstraint(m)
    cl = ClearanceConstraint(c, d_min, lower=lo, upper=hi)
    full = cl.apply_batch(Q)
    assert np.all(full[0][:, fingers] == Q[:, fingers])
    check_abc(c.engine, Q, full, d_min, dstar)
    _want, _it, _deg, decision, watched = pref.push_out(near_of(c.engine, dstar, PUSH_K), Q, margins, d_min, lo=lo, hi=hi,
                                                        watch=fingers)
    c.set_planning(arm, Q[0])
    part = cl.apply_planning(np.ascontiguousarray(Q[:, arm]))
    Qf = Q.copy()
    Qf[:, arm] = part[0]
    c._ensure_full()
    assert c.engine.clearance(Qf, dstar)[0].tobytes() == part[1].tobytes()  # (the planning run measured the same rows)
    needing = full[3] > 0
    rows = needing & ~watched & np.all(decision > DECISION, axis=1)
    print(f"needing {int(needing.sum())}, rows no finger takes part in: {int((needing & ~watched).sum())}, compared {int(rows.sum())}")
    assert rows.sum() >= 0.25 * needing.sum()
    err = float(np.abs(full[0][rows][:, arm] - part[0][rows]).max())
    print(f"|arm columns, full - planning| = {err:.3e}")
    assert err <= TOL_E and np.array_equal(full[4][rows], part[4][rows])


def test_argument_errors():
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    Q4 = Q[:4]
    rc, good = raw_call(e, Q4, d_min)
    assert rc == 0

    def untouched(out):
        return all(np.all(a == (SENT_I if a.dtype == np.int32 else SENT_F)) for a in out)

    nan = float("nan")
    for params in (dict(d_min=0.0), dict(d_min=-1.0), dict(d_min=nan), dict(overshoot=-1e-9), dict(overshoot=nan),
                   dict(damping=0.0), dict(damping=-1.0), dict(damping=nan), dict(step_max=0.0), dict(step_max=nan),
                   dict(max_iter=0), dict(max_pairs=0), dict(max_pairs=-2),
                   dict(lo=np.full(m.nq, 0.5), hi=np.full(m.nq, 0.4)), dict(lo=np.full(m.nq, nan)),
                   dict(hi=np.full(m.nq, nan))):
        params = dict(params)
        rc, out = raw_call(e, Q4, params.pop("d_min", d_min), **params)
        assert rc == E_ARG and untouched(out), params
    rc, out = raw_call(e, Q4, d_min, fn=lambda h, d, q, n, lay, *a: e.lib.mjpl_push_out(h, d, q, n, 7, *a))
    assert rc == E_ARG and untouched(out)  # unknown layout
    rc, out = raw_call(e, Q4, d_min, fn=lambda h, d, q, n, *a: e.lib.mjpl_push_out(h, d, q, -1, *a))
    assert rc == E_ARG and untouched(out)
    rc, out = raw_call(e, Q4, d_min, fn=lambda h, d, *a: e.lib.mjpl_push_out(h, None, *a))
    assert rc == E_ARG and untouched(out)  # no descriptor
    for k in range(5):  # every output is required

        def drop(h, d, q, n, lay, *a, k=k):
            a = list(a)
            a[k] = None
            return e.lib.mjpl_push_out(h, d, q, n, lay, *a)

        rc, out = raw_call(e, Q4, d_min, fn=drop)
        assert rc == E_ARG and untouched(out), NAMES[k]
    desc, _keep = e.push_desc(d_min)
    assert e.lib.mjpl_push_out(e.h, C.byref(desc), Q4.ctypes.data_as(F), 0, eng_mod.AOS, None, None, None, None, None) == 0
    assert e.lib.mjpl_push_out_dev(e.h, C.byref(desc), None, 4, eng_mod.AOS, None, None, None, None, None) == E_ARG
    with pytest.raises(eng_mod.MjplError) as ei:
        e.push_out(Q4, -0.5)
    assert ei.value.code == E_ARG
    # equal bounds are a bound, not an error
    rc, out = raw_call(e, Q4, d_min, lo=Q4[0], hi=Q4[0])
    assert rc == 0


def test_one_slot_per_row():
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    count, pair, dist, *_rest = e.near_pairs(Q, dstar, 32)
    viol = (pair >= 0) & (dist - margins[np.maximum(pair, 0)] < d_min)
    assert (viol.sum(axis=1) > 1).sum() >= 10  # rows with more than one violated pair
    out = e.push_out(Q, d_min, max_pairs=1)
    check_abc(e, Q, out, d_min, dstar)


# ---- 9. the packed order of the active rows is not part of the result
def test_two_identical_calls_return_identical_bytes():
    m, e, Q, margins, flags, d_min, dstar = model_setup("franka_p")
    Q = uniform_configs(m, 4096, seed=PUSH_SEED + 1)
    a = e.push_out(Q, d_min)
    b = e.push_out(Q, d_min)
    for name, x, y in zip(NAMES, a, b):
        assert x.tobytes() == y.tobytes(), name
    assert (a[3] > 1).sum() > 256  # (many rows went through the packing more than once)


# ---- 10. the constraint
def test_clearance_constraint_object_rule_and_composition():
    m = two_walls()
    c = CollisionConstraint(m)
    with pytest.raises(ValueError):
        ClearanceConstraint(c, 0.0)
    with pytest.raises(ValueError):
        ClearanceConstraint(c, float("nan"))
    cl = ClearanceConstraint(c, 0.5)
    assert cl.engine is c.engine and cl.projects
    q = np.array([0.1])
    assert cl.valid_config(q) and cl.apply(q, q) is q
    q = np.array([0.7])
    assert not cl.valid_config(q)
    p = cl.apply(q, q)
    assert p is not q and p is not None and cl.valid_config(p) and q[0] == 0.7
    assert ClearanceConstraint(c, 0.95).apply(q, q) is None  # no configuration is 0.95 from both walls
    assert np.array_equal(cl.valid_configs(np.array([[0.1], [0.7], [-0.45]])), [True, False, False])
    with pytest.raises(ValueError):
        cl.valid_config(np.zeros(2))
    with pytest.raises(ValueError):
        cl.apply_batch(np.zeros((3, 2)))
    out = cl.apply_batch(np.array([[0.1], [0.7]]))
    assert out[0].shape == (2, 1) and out[4].tolist() == [OK, OK] and out[3][0] == 0 and out[3][1] >= 1
    # with the joint limits: a configuration that obeys both
    jl = JointLimitConstraint(m)
    got = apply_constraints(q, q, [jl, cl])
    assert got is not None and obeys_constraints(got, [jl, cl]) and got[0] < 0.4 + 1e-9


def test_rrt_keeps_the_clearance():
    m = scenes.two_dof_ball()
    c = CollisionConstraint(m)
    cl = ClearanceConstraint(c, 0.1)
    constraints = [JointLimitConstraint(m), cl]
    planner = RRT(m, ["ball_slide_x", "ball_slide_y"], constraints, max_planning_time=20.0, epsilon=0.1, seed=5)
    q_init, q_goal = np.array([-0.2, 0.0]), np.array([1.2, 0.0])  # either side of the wall
    path = planner.plan_to_config(q_init, q_goal)
    assert len(path) >= 3 and np.array_equal(path[0], q_init) and np.array_equal(path[-1], q_goal)
    clear = c.clearance_batch(np.stack(path), cl.distmax)[0]
    assert np.all(clear >= 0.1), clear.min()
