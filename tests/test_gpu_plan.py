"""mjpl_plan_paths* (mjpl_amd/csrc/mjpl_plan.h) against their NumPy statement (tests/plan_reference.py), bit for bit
with the engine's own checks as the verdicts, and plan_paths on top of them.  Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import plan_cases as cases
import plan_reference as ref
from mjpl_amd import CollisionConstraint, HipToppTrajectoryGenerator, engine, plan_paths, scenes, smooth_paths

pytestmark = pytest.mark.gpu

STEP = 0.05
EPS = 1.0
DEFAULT_CHUNK_BYTES = 256 << 20
FIELDS = ("P", "n_out", "status", "rounds_used", "edges", "tree_nodes")
E_ARG = -1


@pytest.fixture(scope="module")
def franka():
    """(engine on the headline scene's planning columns, QI, QG, lo, hi) of 37 seeded pairs of valid configurations;
    problem 5 has q_goal == q_init."""
    model, qidx, base, lo, hi = cases.franka_planning()
    e = engine.Engine(model, device=0)
    e.set_planning(qidx, base)
    QI, QG = cases.random_ends(lo, hi, lambda Q: e.check_configs(Q).astype(bool), 37, seed=11)
    yield e, QI, QG, lo, hi
    e.close()


@pytest.fixture(scope="module")
def ball():
    c = CollisionConstraint(scenes.two_dof_ball())
    yield c
    c.engine.close()


def run(e, QI, QG, lo, hi, **kw):
    return dict(zip(FIELDS, e.plan_paths(QI, QG, lo, hi, STEP, EPS, **kw)))


def same_bits(got, want, what=""):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        a, b = (x[f].view(np.uint64) if f == "P" else x[f] for x in (got, want))
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} {f}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


def reference(e, QI, QG, lo, hi, calls=None, **kw):
    def edges(QA, QB):
        if calls is not None:
            calls.append(len(QA))
        return e.check_edges(QA, QB, STEP).astype(bool)
    return ref.plan_paths(QI, QG, lo, hi, lambda Q: e.check_configs(Q).astype(bool), edges, EPS, **kw)


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("rounds", [1, 6])
@pytest.mark.parametrize("K", [1, 7, 64])
def test_bits_of_the_statement(franka, K, rounds, seed):
    e, QI, QG, lo, hi = franka
    calls = []
    want = reference(e, QI, QG, lo, hi, calls, rounds=rounds, candidates=K, nodes=512, seed=seed)
    got = run(e, QI, QG, lo, hi, rounds=rounds, candidates=K, nodes=512, seed=seed)
    print(f"K {K} rounds {rounds}: status counts {np.bincount(got['status'], minlength=5)}, rounds used {got['rounds_used'].tolist()}, "
          f"edges {got['edges'].sum()}, largest tree {got['tree_nodes'].max()}")
    same_bits(got, want, f"K={K} rounds={rounds}")
    # one edge launch for the direct edges and one per round: the library validated exactly the statement's edges
    assert e.get_option("plan_last_edges") == sum(calls) == got["edges"].sum()
    assert e.get_option("plan_last_rounds") == len(calls) - 1 <= rounds and e.get_option("plan_last_chunks") == 1
    assert got["status"][5] == engine.PLAN_SOLVED and got["rounds_used"][5] == 0
    if K == 64 and rounds == 6:  # the block edges of the nearest scan and of the ballot append
        assert got["tree_nodes"].max() > 128
        solved = got["status"] == engine.PLAN_SOLVED
        assert (solved & (got["rounds_used"] > 0)).any()


def test_full_trees_bits(franka):
    e, QI, QG, lo, hi = franka
    want = reference(e, QI, QG, lo, hi, rounds=6, candidates=64, nodes=40, seed=1)
    got = run(e, QI, QG, lo, hi, rounds=6, candidates=64, nodes=40, seed=1)
    same_bits(got, want, "nodes=40")
    assert engine.PLAN_NODES in got["status"] and got["tree_nodes"].max() == 40


def test_solved_paths_pass_check_edges(franka):
    e, QI, QG, lo, hi = franka
    got = run(e, QI, QG, lo, hi, rounds=6, candidates=16, nodes=512, seed=2)
    solved = np.flatnonzero(got["status"] == engine.PLAN_SOLVED)
    assert (got["rounds_used"][solved] == 0).any() and (got["rounds_used"][solved] > 0).any()
    assert (got["n_out"][got["status"] != engine.PLAN_SOLVED] == 0).all()
    QA = np.concatenate([got["P"][b, :got["n_out"][b] - 1] for b in solved])
    QB = np.concatenate([got["P"][b, 1:got["n_out"][b]] for b in solved])
    assert e.check_edges(QA, QB, STEP).all()
    for b in solved:
        n = got["n_out"][b]
        assert 2 <= n <= got["rounds_used"][b] + 2
        assert got["P"][b, 0].tobytes() == QI[b].tobytes() and got["P"][b, n - 1].tobytes() == QG[b].tobytes()


def test_chunks_change_no_bit(franka):
    e, QI, QG, lo, hi = franka
    assert e.get_option("plan_chunk_bytes") == DEFAULT_CHUNK_BYTES
    kw = dict(rounds=6, candidates=64, nodes=512, seed=7)
    one = run(e, QI, QG, lo, hi, **kw)
    assert e.get_option("plan_last_chunks") == 1
    edges, rounds = e.get_option("plan_last_edges"), e.get_option("plan_last_rounds")
    try:
        for nbytes, least in ((1, 37), (300_000, 5)):
            e.set_option("plan_chunk_bytes", nbytes)
            got = run(e, QI, QG, lo, hi, **kw)
            chunks = int(e.get_option("plan_last_chunks"))
            print(f"plan_chunk_bytes {nbytes}: {chunks} chunks")
            assert least <= chunks <= 37 and (chunks == 37) == (nbytes == 1)
            same_bits(got, one, f"chunk bytes {nbytes}")
            assert e.get_option("plan_last_edges") == edges and e.get_option("plan_last_rounds") >= rounds
        for name in ("plan_last_chunks", "plan_last_rounds", "plan_last_edges"):
            with pytest.raises(engine.MjplError):
                e.set_option(name, 1)
    finally:
        e.set_option("plan_chunk_bytes", DEFAULT_CHUNK_BYTES)


def test_nan_problem_changes_no_other(franka):
    e, QI, QG, lo, hi = franka
    kw = dict(rounds=4, candidates=16, nodes=512, seed=1)
    clean = run(e, QI, QG, lo, hi, **kw)
    b = 17  # (a problem in the middle of the batch)
    bad = QG.copy()
    bad[b, 2] = np.nan
    got = run(e, QI, bad, lo, hi, **kw)
    assert got["status"][b] == engine.PLAN_NONFINITE and got["n_out"][b] == 0 and got["edges"][b] == 0 and got["rounds_used"][b] == 0
    assert not got["P"][b].any() and not got["tree_nodes"][b].any()
    others = np.arange(len(QI)) != b
    for f in FIELDS:
        assert np.array_equal(got[f][others].view(np.uint8), clean[f][others].view(np.uint8)), f
    inf = QI.copy()
    inf[3, 0] = np.inf
    assert run(e, inf, QG, lo, hi, rounds=1)["status"][3] == engine.PLAN_NONFINITE


def test_host_and_device_forms_agree(franka):
    e, QI, QG, lo, hi = franka
    B = len(QI)
    kw = dict(rounds=4, candidates=7, nodes=512, seed=3)
    host = run(e, QI, QG, lo, hi, **kw)
    dQI, dQG = e.alloc(QI.nbytes).upload(QI), e.alloc(QG.nbytes).upload(QG)
    bufs = {f: e.alloc(max(host[f].nbytes, 8)) for f in FIELDS}
    e.plan_paths_dev(dQI.ptr, dQG.ptr, B, lo, hi, STEP, EPS, bufs["P"].ptr, bufs["n_out"].ptr, bufs["status"].ptr, bufs["rounds_used"].ptr,
                     bufs["edges"].ptr, bufs["tree_nodes"].ptr, **kw)
    got = {f: bufs[f].download(host[f].dtype, host[f].size).reshape(host[f].shape) for f in FIELDS}
    same_bits(got, host, "device form")
    # without the optional outputs
    for f in ("P", "n_out", "status"):
        bufs[f].upload(np.full_like(host[f], 7))
    e.plan_paths_dev(dQI.ptr, dQG.ptr, B, lo, hi, STEP, EPS, bufs["P"].ptr, bufs["n_out"].ptr, bufs["status"].ptr, **kw)
    for f in ("P", "n_out", "status"):
        assert np.array_equal(bufs[f].download(host[f].dtype, host[f].size).reshape(host[f].shape), host[f]), f
    lib, F64P, I32P = e.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P, n_out, status = np.zeros_like(host["P"]), np.zeros(B, np.int32), np.zeros(B, np.int32)
    desc = engine.Engine.plan_desc(STEP, EPS, **kw)
    assert lib.mjpl_plan_paths(e.h, C.byref(desc), QI.ctypes.data_as(F64P), QG.ctypes.data_as(F64P), B, lo.ctypes.data_as(F64P),
                               hi.ctypes.data_as(F64P), P.ctypes.data_as(F64P), n_out.ctypes.data_as(I32P), status.ctypes.data_as(I32P),
                               None, None, None) == 0
    assert np.array_equal(P.view(np.uint64), host["P"].view(np.uint64)) and np.array_equal(n_out, host["n_out"]) and np.array_equal(status, host["status"])
    for buf in (dQI, dQG, *bufs.values()):
        buf.free()


def test_refused_arguments(franka, ball):
    e, QI, QG, lo, hi = franka
    B = len(QI)
    lib, F64P, I32P = e.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P, n_out, status = np.zeros((B, 4, QI.shape[1])), np.zeros(B, np.int32), np.zeros(B, np.int32)
    nan = float("nan")

    def call(desc=None, QI=QI, QG=QG, B=B, lo=lo, hi=hi, P=P, n_out=n_out, status=status, dev=False):
        desc = engine.PlanDesc(EPS, STEP, 0, 2, 8, 64, 0) if desc is None else desc
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        fn = lib.mjpl_plan_paths_dev if dev else lib.mjpl_plan_paths
        return fn(e.h, C.byref(desc), p(QI, F64P), p(QG, F64P), B, p(lo, F64P), p(hi, F64P), p(P, F64P), p(n_out, I32P), p(status, I32P),
                  None, None, None)
    assert call() == 0  # (rounds_used, edges, tree_nodes: NULL is allowed)
    for kw in (dict(QI=None), dict(QG=None), dict(lo=None), dict(hi=None), dict(P=None), dict(n_out=None), dict(status=None), dict(B=-1)):
        assert call(**kw) == E_ARG, kw
    assert lib.mjpl_plan_paths(e.h, None, None, None, 0, None, None, None, None, None, None, None, None) == E_ARG
    for bad in (engine.PlanDesc(0.0, STEP, 0, 2, 8, 64, 0), engine.PlanDesc(nan, STEP, 0, 2, 8, 64, 0), engine.PlanDesc(EPS, 0.0, 0, 2, 8, 64, 0),
                engine.PlanDesc(EPS, nan, 0, 2, 8, 64, 0), engine.PlanDesc(EPS, STEP, 0, 0, 8, 64, 0), engine.PlanDesc(EPS, STEP, 0, 4097, 8, 64, 0),
                engine.PlanDesc(EPS, STEP, 0, 2, 0, 64, 0), engine.PlanDesc(EPS, STEP, 0, 2, 65, 64, 0), engine.PlanDesc(EPS, STEP, 0, 2, 8, 1, 0),
                engine.PlanDesc(EPS, STEP, 0, 2, 8, 65537, 0)):
        assert call(desc=bad) == E_ARG
        assert call(desc=bad, QI=None, QG=None, B=0, P=None, n_out=None, status=None, dev=True) == E_ARG
    for c, v in ((0, nan), (3, float("inf"))):
        box = lo.copy()
        box[c] = v
        assert call(lo=box) == E_ARG and call(hi=box) == E_ARG
    box = lo.copy()
    box[2] = hi[2] + 1.0
    assert call(lo=box) == E_ARG and b"lo" in lib.mjpl_last_error()
    # B = 0 launches nothing
    assert call(QI=None, QG=None, B=0, P=None, n_out=None, status=None) == 0
    assert e.get_option("plan_last_chunks") == 0 and e.get_option("plan_last_edges") == 0
    empty = e.plan_paths(np.zeros((0, QI.shape[1])), np.zeros((0, QI.shape[1])), lo, hi, STEP, EPS, rounds=3)
    assert empty[0].shape == (0, 5, QI.shape[1]) and all(len(a) == 0 for a in empty)
    # the Python surface
    a, b = np.array([0.0, 0.0]), np.array([-1.0, 1.0])
    box = dict(lo=cases.BALL_LO, hi=cases.BALL_HI)
    assert plan_paths([], [], ball, STEP, epsilon=0.5) == [] and plan_paths([], [], ball, STEP, epsilon=0.5, return_info=True) == ([], [])
    for qi, qg, kw in (([a], [b, b], {}), ([np.zeros(3)], [np.zeros(3)], {}), ([a], [np.array([2.5, 0.0])], {}), ([a], [b], dict(rounds=0)),
                       ([a], [b], dict(candidates=65)), ([a], [b], dict(nodes=1)), ([a], [b], dict(epsilon=0.0)),
                       ([a], [b], dict(lo=[0.5, -2.0])), ([a], [b], dict(lo=[-2.0], hi=[2.0])), ([a], [b], dict(hi=[np.inf, 2.0]))):
        with pytest.raises(ValueError):
            plan_paths(qi, qg, ball, STEP, **{**dict(epsilon=0.5), **box, **kw})
    with pytest.raises(ValueError):
        plan_paths([a], [b], ball, 0.0, epsilon=0.5)
    with pytest.raises(ValueError):
        e.plan_paths(QI[:, :3], QG[:, :3], lo, hi, STEP, EPS)
    with pytest.raises(ValueError):
        e.plan_paths(QI, QG[:-1], lo, hi, STEP, EPS)
    with pytest.raises(ValueError):
        e.plan_paths(QI, QG, lo[:-1], hi[:-1], STEP, EPS)


def test_plan_smooth_parameterise_on_the_ball_scene(ball):
    model = ball.model
    q_inits, q_goals = ([np.array(p[k], float) for p in cases.BALL_PROBLEMS] for k in (0, 1))
    step = cases.BALL_STEP
    paths, info = plan_paths(q_inits, q_goals, ball, step, epsilon=0.5, nodes=512, lo=cases.BALL_LO, hi=cases.BALL_HI, return_info=True)
    print([(i["status"], i["rounds_used"], i["edges"], i["nodes"]) for i in info])
    assert [i["status"] for i in info] == ["solved", "solved", "solved", "invalid_end", "solved", "solved"]
    assert paths[3] is None and info[1]["rounds_used"] == 0 and len(paths[1]) == 2 and info[1]["nodes"] == (0, 0)
    across = [0, 2, 4, 5]
    for b in across:
        path = paths[b]
        assert path[0] is q_inits[b] and path[-1] is q_goals[b] and all(q.shape == (model.nq,) for q in path)
        assert info[b]["rounds_used"] > 0 and 3 <= len(path) <= info[b]["rounds_used"] + 2
        Q = np.stack(path)
        assert ball.valid_edges_planning(Q[:-1], Q[1:], step).all()
        assert np.abs(Q[:, 1]).max() > 0.5  # round an end of the wall
    # the same call is the statement's result
    QI, QG = cases.ball_ends()
    want = ref.plan_paths(QI, QG, cases.BALL_LO, cases.BALL_HI, lambda Q: ball.engine.check_configs(Q).astype(bool),
                          lambda A, Bq: ball.valid_edges_planning(A, Bq, step), 0.5, rounds=32, candidates=16, nodes=512, seed=0)
    got = dict(zip(FIELDS, ball.engine.plan_paths(QI, QG, cases.BALL_LO, cases.BALL_HI, step, 0.5, nodes=512)))
    same_bits(got, want, "ball")
    # ... and feeds the stages after it
    planned = [paths[b] for b in across]
    short = smooth_paths(planned, ball, step)
    for path, s in zip(planned, short):
        assert s[0] is path[0] and s[-1] is path[-1] and len(s) <= len(path)
    gen = HipToppTrajectoryGenerator(0.01, np.full(model.nq, 2.0), np.full(model.nq, 4.0), engine=ball.engine)
    trajs = gen.generate_trajectories(short)
    assert len(trajs) == len(short) and all(t is not None for t in trajs)
    for t, s in zip(trajs, short):
        assert np.allclose(t.positions[-1], s[-1], atol=1e-9)
