"""mjpl_roadmap_build* / mjpl_roadmap_query* (mjpl_amd/csrc/mjpl_roadmap.h) against their NumPy statement
(tests/roadmap_reference.py), bit for bit with the engine's own checks as the verdicts, and Roadmap on top of them.
Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import plan_cases
import roadmap_cases as cases
import roadmap_reference as ref
from mjpl_amd import CollisionConstraint, HipToppTrajectoryGenerator, Roadmap, engine, scenes, smooth_paths

pytestmark = pytest.mark.gpu

STEP = cases.FRANKA_STEP
DEFAULT_CHUNK_BYTES = 256 << 20
DEFAULT_LDS_NODES = 18432
GRAPH = ("node_valid", "row_off", "adj", "w")
ANSWER = ("P", "n_out", "status", "cost")
E_ARG = -1


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(got, want, fields, what=""):
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape, want[f].shape)
        bad = np.argwhere(bits(got[f]) != bits(want[f]))
        assert len(bad) == 0, f"{what} {f}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


@pytest.fixture(scope="module")
def franka():
    """The engine on the headline scene's planning columns, the shared inputs, and per (k, radius) the statement's graph
    under the engine's own verdicts (computed once, shared, never changed)."""
    model, qidx, base, lo, hi = plan_cases.franka_planning()
    e = engine.Engine(model, device=0)
    e.set_planning(qidx, base)
    vc = lambda Q: e.check_configs(Q).astype(bool)  # noqa: E731
    ve = lambda QA, QB: e.check_edges(QA, QB, STEP).astype(bool)  # noqa: E731
    Q, QI, QG = cases.franka_inputs(lo, hi, vc)
    graphs = {(k, r): ref.build(Q, vc, ve, r, k) for k, r in cases.FRANKA_BUILDS}
    yield dict(e=e, vc=vc, ve=ve, Q=Q, QI=QI, QG=QG, graphs=graphs)
    e.close()


@pytest.fixture(scope="module")
def ball():
    c = CollisionConstraint(scenes.two_dof_ball())
    yield c
    c.engine.close()


def build(e, Q, radius, k, step=STEP):
    return dict(zip(GRAPH, e.roadmap_build(Q, radius, step, k)))


def query(e, Q, g, QI, QG, radius, connections, max_rows, step=STEP):
    return dict(zip(ANSWER, e.roadmap_query(Q, g["node_valid"], g["row_off"], g["adj"], g["w"], QI, QG, radius, step, connections, max_rows)))


@pytest.mark.parametrize("k, radius", cases.FRANKA_BUILDS)
def test_build_bits_of_the_statement(franka, k, radius):
    e, Q = franka["e"], franka["Q"]
    want = franka["graphs"][(k, radius)]
    got = build(e, Q, radius, k)
    print(f"k {k} radius {radius}: {len(want['pairs'])} candidates, {want['pair_valid'].sum()} valid, {got['row_off'][-1]} entries")
    same_bits(got, want, GRAPH, f"k={k}")
    cases.check_graph(Q, dict(got, radius=radius), k)
    assert e.get_option("roadmap_last_edges") == len(want["pairs"]) and e.get_option("roadmap_last_chunks") == 1
    assert e.get_option("roadmap_last_sweeps") == 0
    ok = got["node_valid"].astype(bool)
    assert not ok[list(cases.ROW_INVALID)].any() and not ok[cases.ROW_NAN] and ok.sum() == cases.FRANKA_N - 3
    assert want["pair_valid"].any() and not want["pair_valid"].all()


@pytest.mark.parametrize("connections, max_rows", [(1, 256), (4, 256), (32, 256), (4, 3)])
@pytest.mark.parametrize("k, radius", cases.FRANKA_BUILDS)
def test_query_bits_of_the_statement(franka, k, radius, connections, max_rows):
    e, Q, QI, QG = franka["e"], franka["Q"], franka["QI"], franka["QG"]
    g = franka["graphs"][(k, radius)]
    want = ref.query(Q, g, QI, QG, franka["vc"], franka["ve"], radius, connections, max_rows)
    got = query(e, Q, g, QI, QG, radius, connections, max_rows)
    print(f"k {k} connections {connections} max_rows {max_rows}: status counts {np.bincount(got['status'], minlength=5)}, "
          f"rows up to {got['n_out'].max()}, sweeps {e.get_option('roadmap_last_sweeps')}")
    same_bits(got, want, ANSWER, f"k={k} connections={connections} max_rows={max_rows}")
    assert e.get_option("roadmap_last_edges") == want["edges"] and e.get_option("roadmap_last_chunks") == 1
    assert e.get_option("roadmap_last_sweeps") >= want["searched"].sum()
    cases.check_paths(Q, QI, QG, got, franka["ve"])
    assert got["status"][cases.PROB_SAME] == engine.ROADMAP_SOLVED and got["n_out"][cases.PROB_SAME] == 2
    assert got["status"][cases.PROB_NAN] == engine.ROADMAP_NONFINITE and got["status"][cases.PROB_INVALID] == engine.ROADMAP_INVALID_END
    assert got["n_out"][cases.PROB_FAR] in (0, 2)
    if (k, max_rows) == (5, 3):
        assert engine.ROADMAP_LONG in got["status"] and (got["n_out"] <= 3).all()
    if (k, connections, max_rows) == (5, 4, 256):
        assert (got["n_out"] > 2).any() and engine.ROADMAP_NO_PATH in got["status"]


@pytest.mark.parametrize("name", ["split", "around"])
def test_ball_grids_bits(ball, name):
    e = ball.engine
    ball._ensure_full()
    vc = lambda Q: e.check_configs(Q).astype(bool)  # noqa: E731
    ve = lambda QA, QB: e.check_edges(QA, QB, cases.BALL_STEP).astype(bool)  # noqa: E731
    Q, radius = cases.ball_grid(name)
    QI, QG = cases.ball_queries(name)
    want = ref.build(Q, vc, ve, radius, 5)
    got = build(e, Q, radius, 5, cases.BALL_STEP)
    same_bits(got, want, GRAPH, name)
    label = ref.components(got["row_off"], got["adj"], got["node_valid"])
    assert len(np.unique(label[label >= 0])) == (2 if name == "split" else 1)
    for connections in (1, 4):
        ans = ref.query(Q, want, QI, QG, vc, ve, radius, connections, 64)
        res = query(e, Q, got, QI, QG, radius, connections, 64, cases.BALL_STEP)
        same_bits(res, ans, ANSWER, f"{name} connections={connections}")
        cases.check_paths(Q, QI, QG, res, ve)
    print(name, "status", res["status"], "rows", res["n_out"])
    assert res["status"][3] == engine.ROADMAP_INVALID_END and res["n_out"][1] == 2
    if name == "split":
        assert (res["status"][[0, 2, 4]] == engine.ROADMAP_NO_PATH).all()
    else:
        assert (res["n_out"][[0, 2, 4, 5]] > 2).all()


def test_empty_and_single(franka):
    e, Q, QI, QG = franka["e"], franka["Q"], franka["QI"], franka["QG"]
    d = Q.shape[1]
    g0 = build(e, np.zeros((0, d)), 3.0, 5)
    assert len(g0["node_valid"]) == 0 and g0["row_off"].tolist() == [0] and len(g0["adj"]) == len(g0["w"]) == 0
    assert e.get_option("roadmap_last_edges") == 0 and e.get_option("roadmap_last_chunks") == 0
    # N = 0: only the direct edges can solve anything
    res = query(e, np.zeros((0, d)), g0, QI, QG, 3.0, 4, 8)
    want = ref.query(np.zeros((0, d)), g0, QI, QG, franka["vc"], franka["ve"], 3.0, 4, 8)
    same_bits(res, want, ANSWER, "N=0")
    assert set(res["status"]) == {engine.ROADMAP_SOLVED, engine.ROADMAP_NO_PATH, engine.ROADMAP_NONFINITE, engine.ROADMAP_INVALID_END}
    free = Q[[0]]
    g1 = build(e, free, 3.0, 5)
    assert g1["node_valid"].tolist() == [1] and g1["row_off"].tolist() == [0, 0] and (g1["adj"] == -1).all() and not g1["w"].any()
    same_bits(g1, ref.build(free, franka["vc"], franka["ve"], 3.0, 5), GRAPH, "N=1")
    same_bits(query(e, free, g1, QI, QG, 3.0, 4, 8), ref.query(free, g1, QI, QG, franka["vc"], franka["ve"], 3.0, 4, 8), ANSWER, "N=1")
    # B = 0
    res = query(e, Q, franka["graphs"][(5, 3.0)], np.zeros((0, d)), np.zeros((0, d)), 3.0, 4, 8)
    assert res["P"].shape == (0, 8, d) and all(len(res[f]) == 0 for f in ANSWER)
    assert e.get_option("roadmap_last_edges") == 0 and e.get_option("roadmap_last_chunks") == 0


def test_chunks_and_the_workspace_path_change_no_bit(franka):
    e, Q, QI, QG = franka["e"], franka["Q"], franka["QI"], franka["QG"]
    k, radius = 5, 3.0
    want = franka["graphs"][(k, radius)]
    assert e.get_option("roadmap_chunk_bytes") == DEFAULT_CHUNK_BYTES and e.get_option("roadmap_lds_nodes") == DEFAULT_LDS_NODES
    one = query(e, Q, want, QI, QG, radius, 4, 256)
    edges, sweeps = e.get_option("roadmap_last_edges"), e.get_option("roadmap_last_sweeps")
    E = len(want["pairs"])
    per_edge = 2 * Q.shape[1] * 8 + 1
    try:
        for nbytes, chunks in ((1, E), (100 * per_edge, -(-E // 100))):
            e.set_option("roadmap_chunk_bytes", nbytes)
            got = build(e, Q, radius, k)
            print(f"roadmap_chunk_bytes {nbytes}: {int(e.get_option('roadmap_last_chunks'))} edge launches")
            assert e.get_option("roadmap_last_chunks") == chunks and e.get_option("roadmap_last_edges") == E
            same_bits(got, want, GRAPH, f"chunk bytes {nbytes}")
        # the distances in the chunk's workspace instead of LDS: one problem per launch, then five
        e.set_option("roadmap_lds_nodes", 0)
        for nbytes, chunks in ((1, len(QI)), (5 * len(Q) * 8, -(-len(QI) // 5)), (DEFAULT_CHUNK_BYTES, 1)):
            e.set_option("roadmap_chunk_bytes", nbytes)
            got = query(e, Q, want, QI, QG, radius, 4, 256)
            assert e.get_option("roadmap_last_chunks") == chunks
            assert e.get_option("roadmap_last_edges") == edges and e.get_option("roadmap_last_sweeps") >= 1
            same_bits(got, one, ANSWER, f"workspace, chunk bytes {nbytes}")
        print(f"sweeps {sweeps} in LDS, {e.get_option('roadmap_last_sweeps')} in the workspace")
        for name in ("roadmap_last_edges", "roadmap_last_chunks", "roadmap_last_sweeps"):
            with pytest.raises(engine.MjplError):
                e.set_option(name, 1)
        with pytest.raises(engine.MjplError):
            e.set_option("roadmap_lds_nodes", DEFAULT_LDS_NODES + 1)
    finally:
        e.set_option("roadmap_chunk_bytes", DEFAULT_CHUNK_BYTES)
        e.set_option("roadmap_lds_nodes", DEFAULT_LDS_NODES)


def test_host_and_device_forms_agree(franka):
    e, Q, QI, QG = franka["e"], franka["Q"], franka["QI"], franka["QG"]
    k, radius = 5, 3.0
    N, B, d = len(Q), len(QI), Q.shape[1]
    host = build(e, Q, radius, k)
    dQ = e.alloc(Q.nbytes).upload(Q)
    gb = {f: e.alloc(max(host[f].nbytes, 8)) for f in GRAPH}
    e.roadmap_build_dev(dQ.ptr, N, radius, STEP, gb["node_valid"].ptr, gb["row_off"].ptr, gb["adj"].ptr, gb["w"].ptr, k=k)
    got = {f: gb[f].download(host[f].dtype, host[f].size) for f in GRAPH}
    same_bits(got, host, GRAPH, "device build")
    ans = query(e, Q, host, QI, QG, radius, 4, 16)
    dQI, dQG = e.alloc(QI.nbytes).upload(QI), e.alloc(QG.nbytes).upload(QG)
    ab = {f: e.alloc(max(ans[f].nbytes, 8)) for f in ANSWER}
    for with_cost in (True, False):
        for f in ANSWER:
            ab[f].upload(np.full_like(ans[f], 7))
        e.roadmap_query_dev(dQ.ptr, N, gb["node_valid"].ptr, gb["row_off"].ptr, gb["adj"].ptr, gb["w"].ptr, dQI.ptr, dQG.ptr, B, radius, STEP,
                            ab["P"].ptr, ab["n_out"].ptr, ab["status"].ptr, ab["cost"].ptr if with_cost else None, connections=4, max_rows=16)
        res = {f: ab[f].download(ans[f].dtype, ans[f].size).reshape(ans[f].shape) for f in ANSWER}
        same_bits(res, ans, ANSWER if with_cost else ANSWER[:3], "device query")
    for buf in (dQ, dQI, dQG, *gb.values(), *ab.values()):
        buf.free()


def test_refused_arguments(franka):
    e, Q, QI, QG = franka["e"], franka["Q"], franka["QI"], franka["QG"]
    g = franka["graphs"][(5, 3.0)]
    lib, F64P, I32P, U8P = e.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    N, B, d = len(Q), len(QI), Q.shape[1]
    nan, inf = float("nan"), float("inf")
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    out = dict(node_valid=np.zeros(N, np.uint8), row_off=np.zeros(N + 1, np.int32), adj=np.zeros(2 * N * 5, np.int32), w=np.zeros(2 * N * 5))

    def call_build(desc=None, Q=Q, N=N, dev=False, **kw):
        desc = engine.RoadmapDesc(3.0, STEP, 5, 0) if desc is None else desc
        o = {**out, **kw}
        fn = lib.mjpl_roadmap_build_dev if dev else lib.mjpl_roadmap_build
        return fn(e.h, C.byref(desc), p(Q, F64P), N, p(o["node_valid"], U8P), p(o["row_off"], I32P), p(o["adj"], I32P), p(o["w"], F64P))
    assert call_build() == 0
    for kw in (dict(Q=None), dict(node_valid=None), dict(row_off=None), dict(adj=None), dict(w=None), dict(N=-1), dict(N=(1 << 20) + 1)):
        assert call_build(**kw) == E_ARG, kw
    assert lib.mjpl_roadmap_build(e.h, None, None, 0, None, None, None, None) == E_ARG
    for bad in (engine.RoadmapDesc(0.0, STEP, 5, 0), engine.RoadmapDesc(nan, STEP, 5, 0), engine.RoadmapDesc(inf, STEP, 5, 0),
                engine.RoadmapDesc(3.0, 0.0, 5, 0), engine.RoadmapDesc(3.0, nan, 5, 0), engine.RoadmapDesc(3.0, inf, 5, 0),
                engine.RoadmapDesc(3.0, STEP, 0, 0), engine.RoadmapDesc(3.0, STEP, 33, 0)):
        assert call_build(desc=bad) == E_ARG
        assert call_build(desc=bad, Q=None, N=0, dev=True) == E_ARG
    assert call_build(Q=None, N=0, node_valid=None, row_off=None, adj=None, w=None) == 0  # N = 0 launches nothing
    ans = dict(P=np.zeros((B, 4, d)), n_out=np.zeros(B, np.int32), status=np.zeros(B, np.int32))

    def call_query(desc=None, QI=QI, QG=QG, B=B, N=N, dev=False, **kw):
        desc = engine.RoadmapQueryDesc(3.0, STEP, 4, 4) if desc is None else desc
        a = {**dict(Q=Q, **g), **ans, **kw}
        fn = lib.mjpl_roadmap_query_dev if dev else lib.mjpl_roadmap_query
        return fn(e.h, C.byref(desc), p(a["Q"], F64P), N, p(a["node_valid"], U8P), p(a["row_off"], I32P), p(a["adj"], I32P), p(a["w"], F64P),
                  p(QI, F64P), p(QG, F64P), B, p(a["P"], F64P), p(a["n_out"], I32P), p(a["status"], I32P), None)
    assert call_query() == 0  # (cost: NULL is allowed)
    for kw in (dict(Q=None), dict(node_valid=None), dict(row_off=None), dict(adj=None), dict(w=None), dict(QI=None), dict(QG=None), dict(P=None),
               dict(n_out=None), dict(status=None), dict(B=-1), dict(N=-1)):
        assert call_query(**kw) == E_ARG, kw
    for bad in (engine.RoadmapQueryDesc(0.0, STEP, 4, 4), engine.RoadmapQueryDesc(nan, STEP, 4, 4), engine.RoadmapQueryDesc(3.0, 0.0, 4, 4),
                engine.RoadmapQueryDesc(3.0, inf, 4, 4), engine.RoadmapQueryDesc(3.0, STEP, 0, 4), engine.RoadmapQueryDesc(3.0, STEP, 33, 4),
                engine.RoadmapQueryDesc(3.0, STEP, 4, 1)):
        assert call_query(desc=bad) == E_ARG
        assert call_query(desc=bad, QI=None, QG=None, B=0, P=None, n_out=None, status=None, dev=True) == E_ARG
    assert call_query(QI=None, QG=None, B=0, P=None, n_out=None, status=None) == 0  # B = 0 launches nothing
    with pytest.raises(ValueError):
        e.roadmap_build(Q[:, :3], 3.0, STEP)
    with pytest.raises(ValueError):
        e.roadmap_query(Q, g["node_valid"], g["row_off"][:-1], g["adj"], g["w"], QI, QG, 3.0, STEP)
    with pytest.raises(ValueError):
        e.roadmap_query(Q, g["node_valid"], g["row_off"], g["adj"], g["w"], QI, QG[:-1], 3.0, STEP)


def test_roadmap_smooth_parameterise_on_the_ball_scene(ball):
    model = ball.model
    step = cases.BALL_STEP
    rm = Roadmap(ball, step, radius=0.5, k=8).build_uniform(400, lo=[-2.0, -2.0], hi=[2.0, 2.0], seed=3)
    assert rm.nodes.shape == (400, 2) and rm.node_valid.all() and rm.row_off[-1] > 0
    assert ball.valid_configs(rm.nodes).all()
    pairs, lengths = rm.edges()
    assert len(pairs) == rm.row_off[-1] // 2 and (pairs[:, 0] < pairs[:, 1]).all() and (lengths <= 0.5).all() and (lengths > 0).all()
    assert np.array_equal(rm.components(), ref.components(rm.row_off, rm.adj, rm.node_valid))
    q_inits, q_goals = ([np.array(pr[i], float) for pr in plan_cases.BALL_PROBLEMS] for i in (0, 1))
    paths = rm.query(q_inits, q_goals)
    P, n_out, status, cost = rm.query_status(q_inits, q_goals)
    print("status", status, "rows", n_out, "cost", cost)
    assert status[3] == engine.ROADMAP_INVALID_END and paths[3] is None and n_out[1] == 2 and len(paths[1]) == 2
    across = [0, 2, 4, 5]
    assert (status[across] == engine.ROADMAP_SOLVED).all()
    for b in across:
        path = paths[b]
        assert path[0] is q_inits[b] and path[-1] is q_goals[b] and all(q.shape == (model.nq,) for q in path) and len(path) == n_out[b] > 2
        W = np.stack(path)
        assert ball.valid_edges_planning(W[:-1], W[1:], step).all()
        assert np.abs(W[:, 1]).max() > 0.5  # round an end of the wall
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
    assert rm.query([], []) == []
