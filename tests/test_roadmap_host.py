"""Roadmap planning without a GPU: the ABI of mjpl_roadmap_build* / mjpl_roadmap_query*, and the NumPy statement of
both algorithms (tests/roadmap_reference.py) held to its own invariants -- on random graphs, on grids full of ties, and
under the CPU oracle's checks on the very inputs tests/test_gpu_roadmap.py runs (which shows here that they exercise
every final status)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plan_cases
import roadmap_cases as cases
import roadmap_reference as ref
import mjpl_amd
from mjpl_amd import build, engine, scenes
from mjpl_amd.planning import Roadmap
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name in ("mjpl_roadmap_build", "mjpl_roadmap_build_dev", "mjpl_roadmap_query", "mjpl_roadmap_query_dev"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in engine.ABI, name
    values = dict(SOLVED=0, NO_PATH=1, NONFINITE=2, INVALID_END=3, LONG=4)
    for name, value in values.items():
        assert re.search(rf"#define\s+MJPL_ROADMAP_{name}\s+{value}\b", code), name
        assert getattr(engine, f"ROADMAP_{name}") == getattr(ref, name) == value
    assert C.sizeof(engine.RoadmapDesc) == 24 and C.sizeof(engine.RoadmapQueryDesc) == 24
    assert [f[0] for f in engine.RoadmapDesc._fields_] == ["radius", "step_dist", "k", "reserved"]
    assert [f[0] for f in engine.RoadmapQueryDesc._fields_] == ["radius", "step_dist", "connections", "max_rows"]
    assert re.search(r"double radius, step_dist;\s*int32_t k, reserved;\s*}\s*mjpl_roadmap_desc;", code)
    assert re.search(r"double radius, step_dist;\s*int32_t connections, max_rows;\s*}\s*mjpl_roadmap_query_desc;", code)
    assert engine.ROADMAP_MAX_K == ref.MAX_K == 32
    assert "Roadmap" in mjpl_amd.__all__ and "Roadmap" in mjpl_amd.planning.__all__
    assert mjpl_amd.Roadmap is mjpl_amd.planning.Roadmap is Roadmap
    names = engine.option_names()
    writable = engine.option_names(writable_only=True)
    for name in ("roadmap_chunk_bytes", "roadmap_lds_nodes"):
        assert name in names and name in writable, name
    for name in ("roadmap_last_edges", "roadmap_last_chunks", "roadmap_last_sweeps"):
        assert name in names and name not in writable, name


class _NoEngine:
    """A collision constraint whose engine must not be reached."""
    class model:
        nq = 2
        jnt_range = np.array([[-1.0, 1.0], [-1.0, 1.0]])

    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name})")


def test_bad_parameters_are_value_errors_before_any_engine():
    nan, inf = float("nan"), float("inf")
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(step_dist=0.0), dict(step_dist=nan),
               dict(step_dist=inf), dict(k=0), dict(k=33)):
        with pytest.raises(ValueError):
            engine.Engine.roadmap_desc(**{**dict(radius=1.0, step_dist=0.1), **kw})
        with pytest.raises(ValueError):
            Roadmap(_NoEngine(), **{**dict(radius=1.0, step_dist=0.1), **kw})
    for kw in (dict(radius=0.0), dict(step_dist=-0.1), dict(connections=0), dict(connections=33), dict(max_rows=1), dict(max_rows=-4)):
        with pytest.raises(ValueError):
            engine.Engine.roadmap_query_desc(**{**dict(radius=1.0, step_dist=0.1), **kw})
    d = engine.Engine.roadmap_desc(2.5, 0.01)
    assert (d.radius, d.step_dist, d.k, d.reserved) == (2.5, 0.01, 8, 0)
    q = engine.Engine.roadmap_query_desc(2.5, 0.01)
    assert (q.radius, q.step_dist, q.connections, q.max_rows) == (2.5, 0.01, 8, 256)
    r = Roadmap(_NoEngine(), 0.1, 1.0, k=32)
    assert len(r.nodes) == 0 and r.row_off.tolist() == [0] and len(r.edges()[0]) == 0 and len(r.components()) == 0
    a = np.zeros(2)
    for args, kw in ((([a], [a, a]), {}), (([np.zeros(3)], [np.zeros(3)]), {}), (([a], [a]), dict(connections=0)), (([a], [a]), dict(max_rows=1))):
        with pytest.raises(ValueError):
            r.query(*args, **kw)
    with pytest.raises(ValueError):
        r.build(np.zeros((4, 3)))
    for kw in (dict(n=-1), dict(n=4, lo=[0.0]), dict(n=4, lo=[0.0, 0.0], hi=[np.inf, 1.0]), dict(n=4, lo=[2.0, 0.0], hi=[1.0, 1.0])):
        with pytest.raises(ValueError):
            r.build_uniform(**kw)


# ---- the search: Dijkstra on a heap against Jacobi iteration, bit for bit
def random_graph(rng, N, radius, degree):
    """A symmetric CSR over N nodes: weights between 2^-20 radius and radius, a share of them drawn from a short list
    (exact ties) and a share at the two extremes."""
    pairs = set()
    for i in range(N):
        for j in rng.choice(N, size=degree, replace=False):
            if i != j:
                pairs.add((min(i, int(j)), max(i, int(j))))
    pairs = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    kind = rng.integers(0, 4, len(pairs))
    short = radius * np.array([0.25, 0.5, 0.125, 1.0, 2.0 ** -20])
    wt = np.where(kind == 0, short[rng.integers(0, len(short), len(pairs))],
                  np.where(kind == 1, radius * 2.0 ** -rng.uniform(0.0, 20.0, len(pairs)), radius * rng.uniform(2.0 ** -20, 1.0, len(pairs))))
    directed = np.concatenate([pairs, pairs[:, ::-1]])
    ww = np.concatenate([wt, wt])
    order = np.lexsort((directed[:, 1], directed[:, 0]))
    directed, ww = directed[order], ww[order]
    row_off = np.searchsorted(directed[:, 0], np.arange(N + 1)).astype(np.int32)
    return row_off, directed[:, 1].astype(np.int32), ww


@pytest.mark.parametrize("N, degree, seed", [(1, 1, 0), (40, 2, 1), (150, 3, 2), (150, 6, 3)])
def test_dijkstra_is_the_fixed_point(N, degree, seed):
    rng = np.random.default_rng(seed)
    radius = 1.75
    row_off, adj, w = random_graph(rng, N, radius, min(degree, N))
    assert N == 1 or (w.min() >= radius * 2.0 ** -20 and w.max() <= radius and len(np.unique(w)) < 0.9 * len(w) / 2)
    for trial in range(4):
        init = np.full(N, np.inf)
        starts = rng.choice(N, size=min(N, 1 + trial), replace=False)
        init[starts] = radius * rng.choice([0.5, 0.25, 1.0], size=len(starts))  # (ties between the starts too)
        dist = ref.dijkstra(row_off, adj, w, init)
        assert np.array_equal(dist.view(np.uint64), ref.jacobi(row_off, adj, w, init).view(np.uint64))
        assert (dist <= init).all()
        for g in np.flatnonzero(np.isfinite(dist)):
            chain = ref.walk_back(row_off, adj, w, init, dist, g)  # (asserts that it ends within N steps)
            assert 1 <= len(chain) <= N and init[chain[-1]] == dist[chain[-1]]
            assert (np.diff(dist[chain]) < 0).all()  # strictly decreasing: every weight is felt
            total = init[chain[-1]]
            for a, b in zip(chain[::-1][:-1], chain[::-1][1:]):
                p = row_off[b] + int(np.flatnonzero(adj[row_off[b]:row_off[b + 1]] == a)[0])
                total = total + w[p]
            assert total == dist[g]


# ---- the tie rule on an integer grid
def test_neighbours_tie_to_the_lowest_index():
    side = 9
    Q = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2).astype(float)
    ok = np.ones(len(Q), bool)
    centre = 4 * side + 4
    for k, want in ((1, [centre - side]), (3, [centre - side, centre - 1, centre + 1]),
                    (6, [centre - side, centre - 1, centre + 1, centre + side, centre - side - 1, centre - side + 1])):
        idx, dd = ref.nearest_k(Q, ok, Q[centre], k, 4.0, 4.0 * 2.0 ** -40, skip=centre)
        assert idx.tolist() == want and (np.diff(dd) >= 0).all()
    graph = ref.build(Q, lambda X: np.ones(len(X), bool), lambda A, B: np.ones(len(A), bool), 1.5, 3)
    cases.check_graph(Q, dict(graph, radius=1.5), 3)
    # knn is not symmetric: the corner's third neighbour is the diagonal one, whose own three are all closer
    assert side + 1 in graph["adj"][graph["row_off"][0]:graph["row_off"][1]]
    assert (ref.components(graph["row_off"], graph["adj"], graph["node_valid"]) == 0).all()
    # coincident nodes stay apart, and an invalid node is nobody's neighbour
    Q2 = np.concatenate([Q, Q[[centre]], Q[[0]]])
    ok2 = lambda X: ~((X == Q[0]).all(axis=1))  # noqa: E731
    g2 = ref.build(Q2, ok2, lambda A, B: np.ones(len(A), bool), 1.5, 8)
    cases.check_graph(Q2, dict(g2, radius=1.5), 8)
    dup = len(Q)
    assert not g2["node_valid"][0] and not g2["node_valid"][dup + 1]
    assert g2["adj"][g2["row_off"][centre]:g2["row_off"][centre + 1]].tolist() == g2["adj"][g2["row_off"][dup]:g2["row_off"][dup + 1]].tolist()
    assert dup not in g2["adj"][g2["row_off"][centre]:g2["row_off"][centre + 1]]


# ---- the CPU oracle's checks as the verdicts, on the inputs of tests/test_gpu_roadmap.py
def seen_statuses(res):
    out = set()
    for s, n in zip(res["status"], res["n_out"]):
        out.add("direct" if s == ref.SOLVED and n == 2 else int(s))
    return out


@pytest.fixture(scope="module")
def franka_oracle():
    model, qidx, base, lo, hi = plan_cases.franka_planning()
    orc = pyoracle.Oracle(model, planning_qidx=qidx, qpos_base=base)
    vc = lambda Q: orc.valid_configs(Q, nthreads=4).astype(bool)  # noqa: E731
    ve = lambda QA, QB: orc.valid_edges(QA, QB, cases.FRANKA_STEP, nthreads=4).astype(bool)  # noqa: E731
    return vc, ve, cases.franka_inputs(lo, hi, vc)


def test_franka_inputs_cover_every_status(franka_oracle):
    vc, ve, (Q, QI, QG) = franka_oracle
    assert Q.shape == (cases.FRANKA_N, 7) and QI.shape == QG.shape == (cases.FRANKA_B, 7)
    seen = set()
    for k, radius in cases.FRANKA_BUILDS:
        g = ref.build(Q, vc, ve, radius, k)
        cases.check_graph(Q, dict(g, radius=radius), k)
        ok = g["node_valid"].astype(bool)
        assert not ok[list(cases.ROW_INVALID)].any() and not ok[cases.ROW_NAN] and ok[[cases.ROW_DUP, cases.DUP_OF, cases.ROW_NEAR, cases.NEAR_OF]].all()
        assert ok.sum() == cases.FRANKA_N - 3
        with np.errstate(invalid="ignore"):
            in_range = np.array([(ok & (ref.d2(Q, Q[i]) <= radius * radius) & (ref.d2(Q, Q[i]) >= radius * radius * 2.0 ** -40)).sum() - 0
                                 for i in np.flatnonzero(ok)])
        assert (in_range < k).any() and (in_range > k).any(), (k, in_range.min(), in_range.max())
        assert g["pair_valid"].any() and not g["pair_valid"].all()
        # the duplicate and the near row are never joined to their twins
        for a, b in ((cases.ROW_DUP, cases.DUP_OF), (cases.ROW_NEAR, cases.NEAR_OF)):
            assert b not in g["adj"][g["row_off"][a]:g["row_off"][a + 1]]
        print(f"k {k} radius {radius}: {len(g['pairs'])} candidates, {g['pair_valid'].sum()} valid, in range {in_range.min()}..{in_range.max()}, "
              f"components {len(np.unique(ref.components(g['row_off'], g['adj'], g['node_valid']))) - 1}")
        for connections, max_rows in ((1, 256), (4, 256), (32, 256), (4, 3)):
            res = ref.query(Q, g, QI, QG, vc, ve, radius, connections, max_rows)
            cases.check_paths(Q, QI, QG, res, ve)
            print(f"  connections {connections} max_rows {max_rows}: status counts {np.bincount(res['status'], minlength=5)}, "
                  f"direct {(res['n_out'] == 2).sum()}, rows up to {res['n_out'].max()}")
            assert res["status"][cases.PROB_SAME] == ref.SOLVED and res["n_out"][cases.PROB_SAME] == 2
            assert res["status"][cases.PROB_NAN] == ref.NONFINITE and res["status"][cases.PROB_INVALID] == ref.INVALID_END
            assert res["status"][cases.PROB_FAR] in (ref.NO_PATH, ref.SOLVED) and res["n_out"][cases.PROB_FAR] in (0, 2)
            seen |= seen_statuses(res)
            if max_rows == 3:
                assert (res["n_out"] <= 3).all()
    assert seen == {"direct", ref.SOLVED, ref.NO_PATH, ref.NONFINITE, ref.INVALID_END, ref.LONG}


@pytest.mark.parametrize("name", ["split", "around"])
def test_ball_grids(name):
    orc = pyoracle.Oracle(scenes.two_dof_ball())
    vc = lambda Q: orc.valid_configs(Q).astype(bool)  # noqa: E731
    ve = lambda QA, QB: orc.valid_edges(QA, QB, cases.BALL_STEP).astype(bool)  # noqa: E731
    Q, radius = cases.ball_grid(name)
    QI, QG = cases.ball_queries(name)
    g = ref.build(Q, vc, ve, radius, 5)
    cases.check_graph(Q, dict(g, radius=radius), 5)
    ok = g["node_valid"].astype(bool)
    in_range = np.array([(ok & (ref.d2(Q, Q[i]) <= radius * radius)).sum() - 1 for i in np.flatnonzero(ok)])
    assert in_range.max() == 8  # more in range than k, and they tie: four at one spacing, four at the diagonal
    label = ref.components(g["row_off"], g["adj"], g["node_valid"])
    ncomp = len(np.unique(label[label >= 0]))
    res = ref.query(Q, g, QI, QG, vc, ve, radius, 4, 64)
    cases.check_paths(Q, QI, QG, res, ve)
    print(name, "components", ncomp, "status", res["status"], "rows", res["n_out"], "cost", res["cost"])
    assert res["status"][3] == ref.INVALID_END and res["status"][1] == ref.SOLVED and res["n_out"][1] == 2
    if name == "split":
        assert ncomp == 2 and not ok.all()
        assert (res["status"][[0, 2, 4]] == ref.NO_PATH).all()
    else:
        assert ncomp == 1
        assert (res["status"][[0, 2, 4, 5]] == ref.SOLVED).all() and (res["n_out"][[0, 2, 4, 5]] > 2).all()
        # the ends on the axis: over the wall and under it cost the same, and the walk's lowest-index rule decides
        P = res["P"][2, :res["n_out"][2]]
        mirrored = P * np.array([1.0, -1.0])
        total = np.float64(0.0)
        for seg in np.sqrt(ref.d2(mirrored[:-1], mirrored[1:])):
            total = total + seg
        assert total == res["cost"][2] and np.abs(P[:, 1]).max() > 0.6
