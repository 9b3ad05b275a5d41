"""mjpl_plan_paths_constrained* (mjpl_amd/csrc/mjpl_cplan.h) against their NumPy statement (tests/cplan_reference.py),
bit for bit with the engine's own checks and the handle's own projection as the verdicts, and plan_paths_constrained on
top of them.  Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import cplan_cases as cases
import cplan_reference as ref
from mjpl_amd import (CollisionConstraint, HipToppTrajectoryGenerator, JointLimitConstraint, PoseConstraint, engine,
                      generate_constrained_trajectories, plan_paths_constrained, scenes, site_pose)
from mjpl_amd.lie import SE3

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK_BYTES = 256 << 20
FIELDS = ("P", "n_out", "status", "rounds_used", "edges", "tree_nodes")
E_ARG = -1
FRANKA = dict(epsilon=0.1, step_dist=0.05, nodes=256)
BALL = dict(step_dist=cases.BALL_STEP, **cases.BALL_PARAMS)


class Scene:
    """An engine on its planning columns, a PoseConstraint of that engine, the problems and the sampling box."""

    def __init__(self, e, pose, qidx, base, QI, QG, lo, hi):
        self.e, self.pose, self.qidx, self.base, self.QI, self.QG, self.lo, self.hi = e, pose, np.asarray(qidx), base, QI, QG, lo, hi

    def full(self, Q):
        F = np.tile(self.base, (len(Q), 1))
        F[:, self.qidx] = Q
        return F

    def pose_valid(self, Q):
        return self.pose.valid_configs(self.full(Q))

    def project(self, A, X):
        Y, ok, _ = self.pose.apply_batch(self.full(A), self.full(X))
        other = np.setdiff1d(np.arange(len(self.base)), self.qidx)
        same = (Y[:, other].view(np.uint64) == self.base[other].view(np.uint64)).all(axis=1)
        return np.ascontiguousarray(Y[:, self.qidx]), ok & same

    def verdicts(self, step_dist, calls=None):
        def edges(QA, QB):
            if calls is not None:
                calls.append(len(QA))
            return self.e.check_edges(QA, QB, step_dist).astype(bool)
        return (lambda Q: self.e.check_configs(Q).astype(bool)), edges, self.project, self.pose_valid

    def run(self, QI=None, QG=None, pose=None, **kw):
        QI, QG = (self.QI if QI is None else QI), (self.QG if QG is None else QG)
        step_dist, epsilon = kw.pop("step_dist"), kw.pop("epsilon")
        return dict(zip(FIELDS, self.e.plan_paths_constrained(pose or self.pose, QI, QG, self.lo, self.hi, step_dist, epsilon, **kw)))

    def reference(self, calls=None, QI=None, QG=None, **kw):
        QI, QG = (self.QI if QI is None else QI), (self.QG if QG is None else QG)
        step_dist = kw.pop("step_dist")
        return ref.plan_paths_constrained(QI, QG, self.lo, self.hi, *self.verdicts(step_dist, calls), **kw)


def franka_pose(e, model, base):
    return PoseConstraint(model, "ee_site", site_pose(model, base, "ee_site", engine=e), roll=(-0.1, 0.1), pitch=(-0.1, 0.1),
                          q_step=0.1, engine=e)


@pytest.fixture(scope="module")
def franka():
    """The headline scene over the 7 arm columns, the end effector within 0.1 rad of upright in roll and pitch, and 24
    seeded pairs on that manifold: uniform draws projected with q_step = inf, kept where both ends are collision-valid
    and pose-valid.  Problem 5 has q_goal == q_init."""
    model, qidx, base, lo, hi = cases.franka_planning()
    e = engine.Engine(model, device=0)
    pose = franka_pose(e, model, base)
    e.set_planning(qidx, base)
    s = Scene(e, pose, qidx, base, None, None, lo, hi)
    rng = np.random.default_rng(23)
    pose.q_step = np.inf
    rows = np.zeros((0, len(qidx)))
    while len(rows) < 48:
        X = rng.uniform(lo, hi, size=(96, len(qidx)))
        Y, ok = s.project(X, X)
        ok &= (Y >= lo).all(axis=1) & (Y <= hi).all(axis=1)
        Y = Y[ok]
        rows = np.concatenate([rows, Y[e.check_configs(Y).astype(bool) & s.pose_valid(Y)]])
    pose.q_step = 0.1
    s.QI, s.QG = rows[:24].copy(), rows[24:48].copy()
    s.QG[5] = s.QI[5]
    yield s
    e.close()


@pytest.fixture(scope="module")
def ball():
    c = CollisionConstraint(scenes.two_dof_ball())
    c._ensure_full()
    pose = PoseConstraint(c.model, "ball_site", SE3.identity(), y_translation=cases.BALL_BAND, tolerance=cases.BALL_TOL,
                          q_step=cases.BALL_QSTEP, engine=c.engine)
    QI, QG = cases.ball_ends()
    s = Scene(c.engine, pose, np.arange(2), np.asarray(c.model.qpos0, float).copy(), QI, QG, cases.BALL_LO, cases.BALL_HI)
    s.collision = c
    yield s
    c.engine.close()


def same_bits(got, want, what=""):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        a, b = (x[f].view(np.uint64) if f == "P" else x[f] for x in (got, want))
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} {f}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


def check_against_statement(s, what, **kw):
    calls = []
    want = s.reference(calls, **kw)
    got = s.run(**kw)
    print(f"{what}: status counts {np.bincount(got['status'], minlength=6)}, rounds used {got['rounds_used'].tolist()}, "
          f"rows {got['n_out'].tolist()}, edges {got['edges'].sum()}, largest tree {got['tree_nodes'].max()}")
    same_bits(got, want, what)
    # one edge launch per round at most: the library validated exactly the statement's edges
    assert s.e.get_option("plan_last_edges") == sum(calls) == got["edges"].sum()
    assert s.e.get_option("plan_last_chunks") == 1
    return got, want


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
@pytest.mark.parametrize("chain", [1, 8])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("rounds", [1, 32])
def test_bits_of_the_statement_ball(ball, rounds, K, chain, seed):
    kw = {**BALL, **dict(rounds=rounds, candidates=K, chain=chain, seed=seed)}
    check_against_statement(ball, f"ball rounds={rounds} K={K} chain={chain}", **kw)


@pytest.mark.parametrize("chain", [1, 5])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("rounds", [1, 4])
def test_bits_of_the_statement_franka(franka, rounds, K, chain):
    got, _ = check_against_statement(franka, f"franka rounds={rounds} K={K} chain={chain}", rounds=rounds, candidates=K, chain=chain,
                                     seed=3, **FRANKA)
    # q_goal == q_init: round 0's bridge is the closing edge alone
    assert got["status"][5] == engine.PLAN_SOLVED and got["rounds_used"][5] == 1 and got["n_out"][5] == 2
    assert got["P"][5, 0].tobytes() == franka.QI[5].tobytes() and got["P"][5, 1].tobytes() == franka.QG[5].tobytes()


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
def test_statuses_on_the_ball(ball, seed):
    # rounds = 32, the value of tests/test_cplan_host.py: no reason to raise it unless the real projection needs more
    got = ball.run(rounds=32, seed=seed, **BALL)
    print("status", got["status"], "rounds", got["rounds_used"], "rows", got["n_out"])
    assert tuple(got["status"]) == cases.BALL_STATUS
    assert not got["tree_nodes"][[3, 6]].any() and not got["edges"][[3, 6]].any()


def test_invariants_of_solved_paths(ball, franka):
    for s, kw, q_step in ((ball, dict(rounds=32, seed=0, **BALL), cases.BALL_QSTEP),
                          (franka, dict(rounds=12, candidates=16, chain=8, seed=1, **FRANKA), 0.1)):
        want = s.reference(**kw)
        same_bits(s.run(**kw), want, "invariants")
        _, edges, _, pose_valid = s.verdicts(kw["step_dist"])
        cases.check_invariants(s.QI, s.QG, want, edges, pose_valid, kw["epsilon"], q_step, 256)
        assert (want["status"] == ref.SOLVED).sum() >= 2
    got = ball.run(rounds=32, seed=0, **BALL)
    over = [b for b in range(len(ball.QI)) if got["status"][b] == engine.PLAN_SOLVED and
            (got["P"][b, :got["n_out"][b], 1] > 0.6).any() and (got["P"][b, :got["n_out"][b], 0] < 0.4).any() and
            (got["P"][b, :got["n_out"][b], 0] > 0.8).any()]
    assert over  # over the wall, inside the band


def test_long_and_nodes(ball):
    got, _ = check_against_statement(ball, "max_rows=16", rounds=32, seed=0, max_rows=16, **BALL)
    assert got["status"][4] == engine.PLAN_LONG and got["n_out"][4] == 0 and not got["P"][4].any()
    assert got["status"][1] == engine.PLAN_SOLVED and got["n_out"][1] == 13 and got["P"].shape[1] == 16
    got, _ = check_against_statement(ball, "nodes=12", rounds=32, seed=0, **{**BALL, "nodes": 12})
    assert engine.PLAN_NODES in got["status"] and got["tree_nodes"].max() <= 12


def test_full_chain_budget(ball):
    got, want = check_against_statement(ball, "nodes=12 chain=32", rounds=32, seed=0, **{**BALL, "nodes": 12, "chain": 32})
    assert got["tree_nodes"].max() == 12  # the links stop at nodes - n_g
    assert all(len(t[0]) <= 12 and len(t[2]) <= 12 for t in want["trees"] if t is not None)


def test_chunks_change_no_bit(franka):
    e = franka.e
    assert e.get_option("plan_chunk_bytes") == DEFAULT_CHUNK_BYTES
    kw = dict(rounds=4, candidates=7, chain=5, seed=7, **FRANKA)
    one = franka.run(**kw)
    assert e.get_option("plan_last_chunks") == 1
    edges = e.get_option("plan_last_edges")
    try:
        for nbytes, least in ((1, 24), (300_000, 3)):
            e.set_option("plan_chunk_bytes", nbytes)
            got = franka.run(**kw)
            chunks = int(e.get_option("plan_last_chunks"))
            print(f"plan_chunk_bytes {nbytes}: {chunks} chunks")
            assert least <= chunks <= 24 and (chunks == 24) == (nbytes == 1)
            same_bits(got, one, f"chunk bytes {nbytes}")
            assert e.get_option("plan_last_edges") == edges
    finally:
        e.set_option("plan_chunk_bytes", DEFAULT_CHUNK_BYTES)


def test_nan_problem_changes_no_other(franka):
    kw = dict(rounds=4, candidates=7, chain=5, seed=1, **FRANKA)
    clean = franka.run(**kw)
    b = 11  # (a problem in the middle of the batch)
    bad = franka.QG.copy()
    bad[b, 2] = np.nan
    got = franka.run(QG=bad, **kw)
    assert got["status"][b] == engine.PLAN_NONFINITE and got["n_out"][b] == 0 and got["edges"][b] == 0 and got["rounds_used"][b] == 0
    assert not got["P"][b].any() and not got["tree_nodes"][b].any()
    others = np.arange(len(franka.QI)) != b
    for f in FIELDS:
        assert np.array_equal(got[f][others].view(np.uint8), clean[f][others].view(np.uint8)), f
    inf = franka.QI.copy()
    inf[3, 0] = np.inf
    assert franka.run(QI=inf, **{**kw, "rounds": 1})["status"][3] == engine.PLAN_NONFINITE


def test_host_and_device_forms_agree(franka):
    e, QI, QG, lo, hi = franka.e, franka.QI, franka.QG, franka.lo, franka.hi
    B = len(QI)
    kw = dict(rounds=4, candidates=7, chain=5, seed=3, **FRANKA)
    host = franka.run(**kw)
    dkw = {k: v for k, v in kw.items() if k not in ("step_dist", "epsilon")}
    dQI, dQG = e.alloc(QI.nbytes).upload(QI), e.alloc(QG.nbytes).upload(QG)
    bufs = {f: e.alloc(max(host[f].nbytes, 8)) for f in FIELDS}
    e.plan_paths_constrained_dev(franka.pose, dQI.ptr, dQG.ptr, B, lo, hi, kw["step_dist"], kw["epsilon"], bufs["P"].ptr, bufs["n_out"].ptr,
                                 bufs["status"].ptr, bufs["rounds_used"].ptr, bufs["edges"].ptr, bufs["tree_nodes"].ptr, **dkw)
    got = {f: bufs[f].download(host[f].dtype, host[f].size).reshape(host[f].shape) for f in FIELDS}
    same_bits(got, host, "device form")
    # without the optional outputs
    for f in ("P", "n_out", "status"):
        bufs[f].upload(np.full_like(host[f], 7))
    e.plan_paths_constrained_dev(franka.pose, dQI.ptr, dQG.ptr, B, lo, hi, kw["step_dist"], kw["epsilon"], bufs["P"].ptr, bufs["n_out"].ptr,
                                 bufs["status"].ptr, **dkw)
    for f in ("P", "n_out", "status"):
        assert np.array_equal(bufs[f].download(host[f].dtype, host[f].size).reshape(host[f].shape), host[f]), f
    for buf in (dQI, dQG, *bufs.values()):
        buf.free()


def test_generated_chain_and_interpreting_kernels_agree(franka):
    if not franka.pose._proj.spec_loaded():
        pytest.skip("the engine's library has no generated projection for this chain")
    e = franka.e
    kw = dict(rounds=4, candidates=7, chain=5, seed=5, **FRANKA)
    generated = franka.run(**kw)
    e.set_option("pose_spec", 0)
    try:
        plain = franka_pose(e, e.model, franka.base)
        assert not plain._proj.spec_loaded()
        same_bits(franka.run(pose=plain, **kw), generated, "interpreting handle")
    finally:
        e.set_option("pose_spec", 1)


def test_refused_arguments(franka, ball):
    e, QI, QG, lo, hi = franka.e, franka.QI, franka.QG, franka.lo, franka.hi
    B = len(QI)
    lib, F64P, I32P = e.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P, n_out, status = np.zeros((B, 8, QI.shape[1])), np.zeros(B, np.int32), np.zeros(B, np.int32)
    nan = float("nan")
    good = (0.1, 0.05, 0, 2, 4, 64, 3, 8, 0)

    def desc(**kw):
        names = [f[0] for f in engine.CplanDesc._fields_]
        return engine.CplanDesc(*[kw.get(n, v) for n, v in zip(names, good)])

    def call(d=None, h=franka.pose._proj.h, QI=QI, QG=QG, B=B, lo=lo, hi=hi, P=P, n_out=n_out, status=status, dev=False):
        d = desc() if d is None else d
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        fn = lib.mjpl_plan_paths_constrained_dev if dev else lib.mjpl_plan_paths_constrained
        return fn(h, C.byref(d), p(QI, F64P), p(QG, F64P), B, p(lo, F64P), p(hi, F64P), p(P, F64P), p(n_out, I32P), p(status, I32P),
                  None, None, None)
    assert call() == 0  # (rounds_used, edges, tree_nodes: NULL is allowed)
    for kw in (dict(QI=None), dict(QG=None), dict(lo=None), dict(hi=None), dict(P=None), dict(n_out=None), dict(status=None), dict(B=-1),
               dict(h=None)):
        assert call(**kw) == E_ARG, kw
    assert lib.mjpl_plan_paths_constrained(franka.pose._proj.h, None, None, None, 0, None, None, None, None, None, None, None, None) == E_ARG
    for kw in (dict(epsilon=0.0), dict(epsilon=nan), dict(step_dist=0.0), dict(step_dist=nan), dict(rounds=0), dict(rounds=4097),
               dict(candidates=0), dict(candidates=65), dict(nodes=1), dict(nodes=65537), dict(chain=0), dict(chain=33), dict(max_rows=1)):
        assert call(d=desc(**kw)) == E_ARG, kw
        assert call(d=desc(**kw), QI=None, QG=None, B=0, P=None, n_out=None, status=None, dev=True) == E_ARG, kw
    for c, v in ((0, nan), (3, float("inf"))):
        box = lo.copy()
        box[c] = v
        assert call(lo=box) == E_ARG and call(hi=box) == E_ARG
    box = lo.copy()
    box[2] = hi[2] + 1.0
    assert call(lo=box) == E_ARG
    # B = 0 launches nothing
    assert call(QI=None, QG=None, B=0, P=None, n_out=None, status=None) == 0
    assert e.get_option("plan_last_chunks") == 0 and e.get_option("plan_last_edges") == 0
    # more planning columns than the projection takes
    wide = scenes.ModelBuilder()
    for k in range(17):
        wide.add_body(f"b{k}", pos=(0.5 * k, 0, 1), parent=f"b{k - 1}" if k else "world")
        wide.add_joint(f"b{k}", f"j{k}", "slide", axis=(1, 0, 0), range=(-1, 1))
        wide.add_geom(f"b{k}", "sphere", (0.05,))
    wide.add_site("b16", "tip")
    wm = wide.compile()
    we = engine.Engine(wm, device=0)
    wpose = PoseConstraint(wm, "tip", SE3.identity(), z_translation=(0.5, 1.5), engine=we)
    q = np.zeros((1, 17))
    with pytest.raises(ValueError):
        we.plan_paths_constrained(wpose, q, q, -np.ones(17), np.ones(17), 0.05, 0.1)
    out = (np.zeros((1, 8, 17)), np.zeros(1, np.int32), np.zeros(1, np.int32))
    one = -np.ones(17)
    assert lib.mjpl_plan_paths_constrained(wpose._proj.h, C.byref(desc()), q.ctypes.data_as(F64P), q.ctypes.data_as(F64P), 1,
                                           one.ctypes.data_as(F64P), (-one).ctypes.data_as(F64P), out[0].ctypes.data_as(F64P),
                                           out[1].ctypes.data_as(I32P), out[2].ctypes.data_as(I32P), None, None, None) == E_ARG
    we.close()
    # the Python surface: a pose constraint of another engine, and plan_paths' own cases
    c, a, b = ball.collision, np.array([0.0, 0.7]), np.array([1.2, 0.7])
    box = dict(lo=cases.BALL_LO, hi=cases.BALL_HI)
    other = PoseConstraint(c.model, "ball_site", SE3.identity(), y_translation=cases.BALL_BAND, q_step=cases.BALL_QSTEP)
    with pytest.raises(ValueError):
        plan_paths_constrained([a], [b], c, other, cases.BALL_STEP, epsilon=0.1, **box)
    with pytest.raises(ValueError):
        c.engine.plan_paths_constrained(other, a[None], b[None], cases.BALL_LO, cases.BALL_HI, cases.BALL_STEP, 0.1)
    other.engine.close()
    assert plan_paths_constrained([], [], c, ball.pose, cases.BALL_STEP, epsilon=0.1) == []
    assert plan_paths_constrained([], [], c, ball.pose, cases.BALL_STEP, epsilon=0.1, return_info=True) == ([], [])
    for qi, qg, kw in (([a], [b, b], {}), ([np.zeros(3)], [np.zeros(3)], {}), ([a], [np.array([2.5, 0.7])], {}), ([a], [b], dict(rounds=0)),
                       ([a], [b], dict(candidates=65)), ([a], [b], dict(nodes=1)), ([a], [b], dict(epsilon=0.0)), ([a], [b], dict(chain=0)),
                       ([a], [b], dict(chain=33)), ([a], [b], dict(max_rows=1)), ([a], [b], dict(lo=[0.5, -2.0])),
                       ([a], [b], dict(lo=[-2.0], hi=[2.0])), ([a], [b], dict(hi=[np.inf, 2.0]))):
        with pytest.raises(ValueError):
            plan_paths_constrained(qi, qg, c, ball.pose, cases.BALL_STEP, **{**dict(epsilon=0.1), **box, **kw})
    with pytest.raises(ValueError):
        plan_paths_constrained([a], [b], c, ball.pose, 0.0, epsilon=0.1)


def test_plan_and_parameterise_on_the_ball_scene(ball):
    c, pose, model = ball.collision, ball.pose, ball.collision.model
    q_inits, q_goals = ([np.array(p[k], float) for p in cases.BALL_PROBLEMS] for k in (0, 1))
    paths, info = plan_paths_constrained(q_inits, q_goals, c, pose, cases.BALL_STEP, rounds=32, lo=cases.BALL_LO, hi=cases.BALL_HI,
                                         return_info=True, **cases.BALL_PARAMS)
    print([(i["status"], i["rounds_used"], i["edges"], i["nodes"]) for i in info])
    assert [i["status"] for i in info] == ["solved", "solved", "solved", "invalid_end", "solved", "solved", "invalid_end"]
    assert paths[3] is None and paths[6] is None and info[3]["nodes"] == (0, 0)
    solved = [0, 1, 2, 4, 5]
    for b in solved:
        path = paths[b]
        assert path[0] is q_inits[b] and path[-1] is q_goals[b] and all(q.shape == (model.nq,) for q in path)
        assert pose.valid_configs(np.stack(path)).all()
    # the same call is the statement's result
    got = ball.run(rounds=32, seed=0, **BALL)
    for b in solved:
        assert np.array_equal(np.stack(paths[b]), got["P"][b, :got["n_out"][b]])
    # long paths are reported by name
    _, info16 = plan_paths_constrained(q_inits, q_goals, c, pose, cases.BALL_STEP, rounds=32, max_rows=16, lo=cases.BALL_LO,
                                       hi=cases.BALL_HI, return_info=True, **cases.BALL_PARAMS)
    assert info16[4]["status"] == "long"
    # ... and feeds the stage after it
    constraints = [pose, JointLimitConstraint(model), c]
    gen = HipToppTrajectoryGenerator(0.01, np.full(model.nq, 1.0), np.full(model.nq, 2.0), engine=c.engine)
    trajs = generate_constrained_trajectories([paths[b] for b in solved], gen, constraints, max_rounds=64)
    for b, t in zip(solved, trajs):
        assert t is not None, b
        Q = np.stack(t.positions)
        assert all(k.valid_configs(Q).all() for k in constraints), b
        assert np.allclose(Q[-1], q_goals[b], atol=1e-9)
