"""Constrained batched planning without a GPU: the ABI of mjpl_plan_paths_constrained*, and the NumPy statement of the
algorithm (tests/cplan_reference.py) held to its own invariants on a CPU stand-in of scenes.two_dof_ball() -- the very
problems tests/test_gpu_cplan.py runs on the real kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cplan_cases as cases
import cplan_reference as ref
import mjpl_amd
from mjpl_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name in ("mjpl_plan_paths_constrained", "mjpl_plan_paths_constrained_dev"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in engine.ABI, name
    assert re.search(r"#define\s+MJPL_PLAN_LONG\s+5\b", code)
    assert engine.PLAN_LONG == ref.LONG == 5
    assert C.sizeof(engine.CplanDesc) == 48
    assert [f[0] for f in engine.CplanDesc._fields_] == ["epsilon", "step_dist", "seed", "rounds", "candidates", "nodes", "chain", "max_rows",
                                                         "reserved"]
    assert re.search(r"double epsilon, step_dist;\s*uint64_t seed;\s*int32_t rounds, candidates, nodes, chain, max_rows, reserved;\s*}\s*"
                     r"mjpl_cplan_desc;", code)
    assert "plan_paths_constrained" in mjpl_amd.__all__ and "plan_paths_constrained" in mjpl_amd.planning.__all__
    assert mjpl_amd.plan_paths_constrained is mjpl_amd.planning.plan_paths_constrained


def test_bad_parameters_are_value_errors_before_any_engine():
    nan = float("nan")
    for kw in (dict(step_dist=0.0), dict(step_dist=nan), dict(epsilon=0.0), dict(epsilon=nan), dict(rounds=0), dict(rounds=4097),
               dict(candidates=0), dict(candidates=65), dict(nodes=1), dict(nodes=65537), dict(chain=0), dict(chain=33),
               dict(max_rows=1)):
        with pytest.raises(ValueError):
            engine.Engine.cplan_desc(**{**dict(step_dist=0.1, epsilon=1.0), **kw})
    d = engine.Engine.cplan_desc(0.01, 0.5)
    assert (d.rounds, d.candidates, d.nodes, d.chain, d.max_rows, d.seed, d.reserved) == (64, 16, 1024, 8, 256, 0, 0)


# ---- the stand-in of scenes.two_dof_ball(): every verdict in NumPy
WALL_LO, WALL_HI, BALL_R = np.array([0.5, -0.5]), np.array([0.7, 0.5]), 0.1


def ball_configs(Q):
    Q = np.asarray(Q, float)
    away = Q - np.clip(Q, WALL_LO, WALL_HI)
    return np.linalg.norm(away, axis=1) > BALL_R


def ball_edges(QA, QB):
    out = np.zeros(len(QA), bool)
    for e, (a, b) in enumerate(zip(QA, QB)):
        n = max(int(np.ceil(np.linalg.norm(b - a) / cases.BALL_STEP)), 1)
        out[e] = ball_configs(a + (b - a) * (np.arange(1, n + 1) / n)[:, None]).all()
    return out


def ball_pose_valid(Q):
    Q = np.asarray(Q, float)
    off = Q[:, 1] - np.clip(Q[:, 1], *cases.BALL_BAND)
    return (np.abs(off) <= cases.BALL_TOL) & (np.abs(Q) <= 2.0).all(axis=1)


def ball_project(A, X):
    Y = np.array(X, float)
    Y[:, 1] = np.clip(Y[:, 1], *cases.BALL_BAND)
    ok = (np.sqrt(ref.d2(np.asarray(A, float), Y)) <= 2.0 * cases.BALL_QSTEP) & (np.abs(Y) <= 2.0).all(axis=1)
    return Y, ok


VERDICTS = (ball_configs, ball_edges, ball_project, ball_pose_valid)


def run(rounds=32, seed=0, **kw):
    QI, QG = cases.ball_ends()
    return ref.plan_paths_constrained(QI, QG, cases.BALL_LO, cases.BALL_HI, *VERDICTS, rounds=rounds, seed=seed,
                                      **{**cases.BALL_PARAMS, **kw})


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
def test_statement_on_the_ball(seed):
    QI, QG = cases.ball_ends()
    res = run(seed=seed)
    print("status", res["status"], "rounds", res["rounds_used"], "rows", res["n_out"], "edges", res["edges"], "nodes", res["tree_nodes"].tolist())
    assert tuple(res["status"]) == cases.BALL_STATUS
    assert res["rounds_used"].max() <= 15 and res["n_out"].max() <= 37
    assert res["rounds_used"][1] == 2
    cases.check_invariants(QI, QG, res, ball_edges, ball_pose_valid, cases.BALL_PARAMS["epsilon"], cases.BALL_QSTEP, 256)
    for R1 in (1, 5):
        cases.check_rounds_prefix(QI, QG, cases.BALL_LO, cases.BALL_HI, VERDICTS, res, R1, seed=seed, **cases.BALL_PARAMS)
    # across the wall means over it, inside the band
    P = res["P"][0, :res["n_out"][0]]
    assert (P[:, 1] > 0.6).any() and (P[:, 0] < 0.4).any() and (P[:, 0] > 0.8).any()


def test_each_callable_is_called_once_per_stage():
    calls = dict(configs=0, pose=0, project=[], edges=[])

    def vc(Q):
        calls["configs"] += 1
        return ball_configs(Q)

    def pv(Q):
        calls["pose"] += 1
        return ball_pose_valid(Q)

    def pj(A, X):
        calls["project"].append(len(A))
        return ball_project(A, X)

    def ve(QA, QB):
        calls["edges"].append(len(QA))
        return ball_edges(QA, QB)

    QI, QG = cases.ball_ends()
    res = ref.plan_paths_constrained(QI, QG, cases.BALL_LO, cases.BALL_HI, vc, ve, pj, pv, rounds=32, seed=0, **cases.BALL_PARAMS)
    R = int(res["rounds_used"].max())
    assert calls["configs"] == calls["pose"] == 1
    assert len(calls["edges"]) <= R and sum(calls["edges"]) == res["edges"].sum()
    assert len(calls["project"]) <= R * (cases.BALL_PARAMS["chain"] + 1)


def test_long_paths_are_reported_not_truncated():
    full, res = run(), run(max_rows=16)
    assert full["n_out"][4] > 16 and full["n_out"][1] == 13
    assert res["status"][4] == ref.LONG and res["n_out"][4] == 0 and not res["P"][4].any()
    assert res["status"][1] == ref.SOLVED and res["n_out"][1] == 13
    assert res["rounds_used"][4] == full["rounds_used"][4]


def test_node_capacity():
    res = run(nodes=12)
    assert ref.NODES in res["status"]
    assert (res["tree_nodes"] <= 12).all()
    assert all(len(t[0]) <= 12 and len(t[2]) <= 12 for t in res["trees"] if t is not None)


def test_the_bridge_is_what_joins_quickly():
    res = run(chain=1)
    assert res["rounds_used"][1] >= 12  # the free straight line, one link per round
