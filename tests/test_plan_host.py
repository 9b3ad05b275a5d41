"""Batched planning without a GPU: the ABI of mjpl_plan_paths*, and the NumPy statement of the algorithm
(tests/plan_reference.py) held to its own invariants -- under a pure-NumPy verdict and under the CPU oracle's checks,
on the very inputs tests/test_gpu_plan.py runs (which shows here that they exercise every final status)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plan_cases as cases
import plan_reference as ref
import mjpl_amd
from mjpl_amd import build, engine, scenes
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name in ("mjpl_plan_paths", "mjpl_plan_paths_dev"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in engine.ABI, name
    values = dict(SOLVED=0, ROUNDS=1, NONFINITE=2, INVALID_END=3, NODES=4)
    for name, value in values.items():
        assert re.search(rf"#define\s+MJPL_PLAN_{name}\s+{value}\b", code), name
        assert getattr(engine, f"PLAN_{name}") == getattr(ref, name) == value
    assert C.sizeof(engine.PlanDesc) == 40
    assert [f[0] for f in engine.PlanDesc._fields_] == ["epsilon", "step_dist", "seed", "rounds", "candidates", "nodes", "reserved"]
    assert re.search(r"double epsilon, step_dist;\s*uint64_t seed;\s*int32_t rounds, candidates, nodes, reserved;\s*}\s*mjpl_plan_desc;", code)
    assert "plan_paths" in mjpl_amd.__all__ and "plan_paths" in mjpl_amd.planning.__all__
    assert mjpl_amd.plan_paths is mjpl_amd.planning.plan_paths
    names = engine.option_names()
    writable = engine.option_names(writable_only=True)
    assert "plan_chunk_bytes" in names and "plan_chunk_bytes" in writable
    for name in ("plan_last_chunks", "plan_last_rounds", "plan_last_edges"):
        assert name in names and name not in writable, name


def test_bad_parameters_are_value_errors_before_any_engine():
    nan = float("nan")
    for kw in (dict(step_dist=0.0), dict(step_dist=-1.0), dict(step_dist=nan), dict(epsilon=0.0), dict(epsilon=-0.5), dict(epsilon=nan),
               dict(rounds=0), dict(rounds=4097), dict(candidates=0), dict(candidates=65), dict(nodes=1), dict(nodes=65537)):
        with pytest.raises(ValueError):
            engine.Engine.plan_desc(**{**dict(step_dist=0.1, epsilon=1.0), **kw})
    d = engine.Engine.plan_desc(0.01, 0.5, 4096, 64, 65536, seed=2**64 - 1)
    assert (d.epsilon, d.step_dist, d.seed, d.rounds, d.candidates, d.nodes, d.reserved) == (0.5, 0.01, 2**64 - 1, 4096, 64, 65536, 0)
    d = engine.Engine.plan_desc(0.01, 0.5)
    assert (d.rounds, d.candidates, d.nodes, d.seed) == (32, 16, 1024, 0)


def test_target_rule():
    assert ref.splitmix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    lo, hi = np.array([-2.0, 0.5, 1.25, -3.0]), np.array([2.0, 0.75, 1.25, -1.0])
    T = np.stack([ref.target(lo, hi, 3, b, r, l) for b in range(4) for r in range(5) for l in range(64)])
    assert (T >= lo).all() and (T <= hi).all()
    assert (T[:, 2] == 1.25).all()  # lo == hi
    for c in (0, 1, 3):  # uniform enough: every tenth of the range is hit
        assert len(np.unique(np.floor((T[:, c] - lo[c]) / (hi[c] - lo[c]) * 10))) == 10
    base = ref.target(lo, hi, 3, 1, 2, 5)
    for other in (ref.target(lo, hi, 4, 1, 2, 5), ref.target(lo, hi, 3, 2, 2, 5), ref.target(lo, hi, 3, 1, 3, 5), ref.target(lo, hi, 3, 1, 2, 6)):
        assert (other[[0, 1, 3]] != base[[0, 1, 3]]).all()  # every column depends on seed, b, r and l
    assert np.array_equal(base, ref.target(lo, hi, 3, 1, 2, 5))
    # the columns of one target are different draws
    u = (base[[0, 1, 3]] - lo[[0, 1, 3]]) / (hi[[0, 1, 3]] - lo[[0, 1, 3]])
    assert len(np.unique(np.round(u, 6))) == 3


def test_step_and_nearest():
    a, t = np.array([0.0, 0.0]), np.array([3.0, 4.0])
    assert np.array_equal(ref.step(a, t, 5.0), t) and np.array_equal(ref.step(a, t, 6.0), t)
    assert np.allclose(ref.step(a, t, 1.0), [0.6, 0.8], atol=1e-15)
    T = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, 0.5]])
    assert ref.nearest(T[:3], np.zeros(2))[0] == 0  # a tie goes to the lowest index
    assert ref.nearest(T, np.zeros(2)) == (3, 0.25)


# ---- a 2-D point and a disc: the verdicts in NumPy
DISC_C, DISC_R, DISC_STEP = np.array([0.0, 0.0]), 0.5, 0.02


def disc_configs(Q):
    return np.linalg.norm(np.asarray(Q) - DISC_C, axis=1) > DISC_R


def disc_edges(QA, QB):
    out = np.zeros(len(QA), bool)
    for e, (a, b) in enumerate(zip(QA, QB)):
        n = max(int(np.ceil(np.linalg.norm(b - a) / DISC_STEP)), 1)
        pts = a + (b - a) * (np.arange(1, n + 1) / n)[:, None]
        out[e] = (np.linalg.norm(pts - DISC_C, axis=1) > DISC_R).all()
    return out


@pytest.mark.parametrize("K, epsilon, rounds, nodes, seed", [(1, 0.4, 12, 64, 0), (7, 0.4, 12, 64, 1), (64, 0.25, 12, 512, 2), (16, 0.4, 6, 20, 3)])
def test_reference_invariants_point_and_disc(K, epsilon, rounds, nodes, seed):
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    QI, QG = cases.random_ends(lo, hi, disc_configs, 24, seed=3)
    params = dict(epsilon=epsilon, candidates=K, nodes=nodes, seed=seed)
    res = ref.plan_paths(QI, QG, lo, hi, disc_configs, disc_edges, rounds=rounds, **params)
    cases.check_invariants(QI, QG, res, disc_edges, epsilon, rounds)
    for R1 in (1, rounds // 2):
        cases.check_rounds_prefix(QI, QG, lo, hi, disc_configs, disc_edges, res, R1, **params)
    solved = res["status"] == ref.SOLVED
    assert (solved & (res["rounds_used"] == 0)).any() and (solved & (res["rounds_used"] > 0)).any()
    assert res["status"][5] == ref.SOLVED and res["n_out"][5] == 2  # q_goal == q_init: the direct edge
    assert (res["tree_nodes"] <= nodes).all()
    if nodes == 20:
        assert ref.NODES in res["status"]


# ---- the CPU oracle's checks as the verdicts
@pytest.fixture(scope="module")
def ball_oracle():
    orc = pyoracle.Oracle(scenes.two_dof_ball())
    return (lambda Q: orc.valid_configs(Q).astype(bool)), (lambda QA, QB: orc.valid_edges(QA, QB, cases.BALL_STEP).astype(bool))


def test_reference_invariants_two_dof_ball_oracle(ball_oracle):
    vc, ve = ball_oracle
    QI, QG = cases.ball_ends()
    params = dict(epsilon=0.5, candidates=16, nodes=512, seed=0)
    res = ref.plan_paths(QI, QG, cases.BALL_LO, cases.BALL_HI, vc, ve, rounds=32, **params)
    print("status", res["status"], "rounds", res["rounds_used"], "edges", res["edges"], "nodes", res["tree_nodes"].tolist())
    cases.check_invariants(QI, QG, res, ve, 0.5, 32)
    cases.check_rounds_prefix(QI, QG, cases.BALL_LO, cases.BALL_HI, vc, ve, res, 3, **params)
    solved = res["status"] == ref.SOLVED
    # a path across the wall goes round one of its ends
    across = [b for b in range(len(QI)) if solved[b] and res["rounds_used"][b] > 0]
    assert across
    for b in across:
        P = res["P"][b, :res["n_out"][b]]
        assert np.abs(P[:, 1]).max() > 0.5


def test_status_coverage_two_dof_ball(ball_oracle):
    vc, ve = ball_oracle
    QI, QG = cases.ball_ends()
    seen = set()

    def run(K, epsilon, rounds, nodes, QI=QI):
        res = ref.plan_paths(QI, QG, cases.BALL_LO, cases.BALL_HI, vc, ve, epsilon=epsilon, rounds=rounds, candidates=K, nodes=nodes, seed=0)
        print((K, epsilon, rounds, nodes), "status", res["status"], "rounds", res["rounds_used"])
        cases.check_invariants(QI, QG, res, ve, epsilon, rounds)
        for s, r in zip(res["status"], res["rounds_used"]):
            seen.add("direct" if s == ref.SOLVED and r == 0 else int(s))
        return res
    run(16, 0.5, 32, 512)
    run(1, 0.5, 8, 64)
    run(64, 0.25, 32, 128)
    bad = QI.copy()
    bad[2, 1] = np.nan
    res = run(16, 0.5, 4, 512, QI=bad)
    assert res["status"][2] == ref.NONFINITE and res["edges"][2] == 0 and res["n_out"][2] == 0
    assert seen == {"direct", ref.SOLVED, ref.ROUNDS, ref.NONFINITE, ref.INVALID_END, ref.NODES}


@pytest.mark.parametrize("K", [7, 64])
def test_reference_invariants_franka_oracle(K):
    model, qidx, base, lo, hi = cases.franka_planning()
    orc = pyoracle.Oracle(model, planning_qidx=qidx, qpos_base=base)
    step = 0.05

    def vc(Q):
        return orc.valid_configs(Q, nthreads=4).astype(bool)
    calls = []

    def ve(QA, QB):
        ok = orc.valid_edges(QA, QB, step, nthreads=4).astype(bool)
        calls.append(ok)
        return ok
    QI, QG = cases.random_ends(lo, hi, vc, 16, seed=11)
    params = dict(epsilon=1.0, candidates=K, nodes=512, seed=0)
    res = ref.plan_paths(QI, QG, lo, hi, vc, ve, rounds=6, **params)
    verdicts = np.concatenate(calls)
    assert verdicts.any() and not verdicts.all()
    assert len(verdicts) == res["edges"].sum()
    print("status", res["status"], "rounds", res["rounds_used"], "edges", res["edges"].sum())
    cases.check_invariants(QI, QG, res, ve, 1.0, 6)
    cases.check_rounds_prefix(QI, QG, lo, hi, vc, ve, res, 2, **params)
    solved = res["status"] == ref.SOLVED
    assert (solved & (res["rounds_used"] == 0)).any() and (solved & (res["rounds_used"] > 0)).any()
