"""Batched path shortcutting without a GPU: the ABI of mjpl_shortcut_paths*, and the NumPy statement of the algorithm
(tests/shortcut_reference.py) held to its own invariants -- under a pure-NumPy verdict and under the CPU oracle's edge
check, on the very inputs tests/test_gpu_shortcut.py runs (which shows here that they exercise accepted shortcuts,
rejected ones and both final statuses)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shortcut_cases as cases
import shortcut_reference as ref
import mjpl_amd
from mjpl_amd import build, engine, scenes
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name in ("mjpl_shortcut_paths", "mjpl_shortcut_paths_dev"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name), name
        assert name in engine.ABI, name
    for name, value in (("MJPL_SHORTCUT_CONVERGED", 0), ("MJPL_SHORTCUT_ROUNDS", 1), ("MJPL_SHORTCUT_NONFINITE", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    assert (engine.SHORTCUT_CONVERGED, engine.SHORTCUT_ROUNDS, engine.SHORTCUT_NONFINITE) == (ref.CONVERGED, ref.ROUNDS, ref.NONFINITE) == (0, 1, 2)
    assert C.sizeof(engine.ShortcutDesc) == 32
    assert [f[0] for f in engine.ShortcutDesc._fields_] == ["step_dist", "min_saving", "seed", "rounds", "candidates"]
    assert "smooth_paths" in mjpl_amd.__all__ and "smooth_paths" in mjpl_amd.planning.__all__
    assert mjpl_amd.smooth_paths is mjpl_amd.planning.smooth_paths
    names = engine.option_names()
    assert "shortcut_chunk_bytes" in names and "shortcut_last_chunks" in names
    writable = engine.option_names(writable_only=True)
    assert "shortcut_chunk_bytes" in writable and "shortcut_last_chunks" not in writable


def test_bad_parameters_are_value_errors_before_any_engine():
    for kw in (dict(step_dist=0.0), dict(step_dist=float("nan")), dict(step_dist=0.1, rounds=0), dict(step_dist=0.1, candidates=0),
               dict(step_dist=0.1, candidates=65), dict(step_dist=0.1, min_saving=-1.0), dict(step_dist=0.1, min_saving=float("nan"))):
        with pytest.raises(ValueError):
            engine.Engine.shortcut_desc(**kw)
    d = engine.Engine.shortcut_desc(0.01, 3, 7, seed=2**64 - 1, min_saving=0.5)
    assert (d.step_dist, d.min_saving, d.seed, d.rounds, d.candidates) == (0.01, 0.5, 2**64 - 1, 3, 7)


def test_candidate_rule():
    assert ref.splitmix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    for m, K, exhaustive in ((3, 1, True), (4, 1, False), (5, 7, True), (6, 7, False), (12, 64, True), (13, 64, False)):
        ex, cands = ref.candidates_of(m, K, 1, 0, 0)
        assert ex == exhaustive
        assert len(cands) == ((m - 1) * (m - 2) // 2 if ex else K)
        assert all(0 <= i and i + 2 <= j <= m - 1 for _, i, j in cands)
        if ex:
            assert [(i, j) for _, i, j in cands] == sorted({(i, j) for _, i, j in cands})
    # every pair can be drawn, and the draw depends on path, round and seed
    seen = {(i, j) for r in range(40) for _, i, j in ref.candidates_of(13, 64, 5, 2, r)[1]}
    assert len(seen) == 66
    assert ref.candidates_of(40, 64, 5, 2, 0)[1] != ref.candidates_of(40, 64, 5, 3, 0)[1] != ref.candidates_of(40, 64, 6, 3, 0)[1]


# ---- a 2-D point and a disc: the verdict in NumPy
DISC_C, DISC_R, DISC_STEP = np.array([0.0, 0.0]), 0.5, 0.02


def disc_verdict(QA, QB):
    out = np.zeros(len(QA), bool)
    for e, (a, b) in enumerate(zip(QA, QB)):
        n = max(int(np.ceil(np.linalg.norm(b - a) / DISC_STEP)), 1)
        pts = a + (b - a) * (np.arange(1, n + 1) / n)[:, None]
        out[e] = (np.linalg.norm(pts - DISC_C, axis=1) > DISC_R).all()
    return out


def disc_paths(seed=3):
    def free(Q):
        return np.linalg.norm(Q - DISC_C, axis=1) > DISC_R
    return cases.random_walks([-1.5, -1.5], [1.5, 1.5], free, cases.path_lengths(24), seed, step=0.4)


@pytest.mark.parametrize("K, rounds, seed", [(1, 6, 0), (7, 6, 1), (64, 6, 2), (64, 40, 3)])
def test_reference_invariants_point_and_disc(K, rounds, seed):
    W, off = cases.pack(disc_paths())
    res = ref.shortcut_paths(W, off, disc_verdict, rounds=rounds, candidates=K, seed=seed)
    cases.check_invariants(W, off, res, disc_verdict)
    for R1 in (1, rounds // 2):
        cases.check_rounds_prefix(W, off, disc_verdict, res, R1, candidates=K, seed=seed)
    if K == 64:
        assert res["accepted"].sum() > 0 and (res["proposed"] > res["accepted"]).any()
    if rounds == 40:
        assert (res["status"] == ref.CONVERGED).all()


def test_reference_min_saving_and_nonfinite():
    paths = disc_paths()
    W, off = cases.pack(paths)
    plain = ref.shortcut_paths(W, off, disc_verdict, rounds=4, candidates=64, seed=0)
    picky = ref.shortcut_paths(W, off, disc_verdict, rounds=4, candidates=64, seed=0, min_saving=0.3)
    cases.check_invariants(W, off, picky, disc_verdict, min_saving=0.3)
    assert picky["proposed"].sum() < plain["proposed"].sum()
    bad = W.copy()
    bad[off[9] + 1, 1] = np.nan
    res = ref.shortcut_paths(bad, off, disc_verdict, rounds=4, candidates=64, seed=0)
    assert res["status"][9] == ref.NONFINITE and res["keep"][off[9]:off[10]].all() and np.isnan(res["length"][9])
    assert res["proposed"][9] == 0 and res["accepted"][9] == 0
    for b in range(len(paths)):
        if b != 9:
            assert np.array_equal(res["keep"][off[b]:off[b + 1]], plain["keep"][off[b]:off[b + 1]])
            assert res["length"][b] == plain["length"][b] and res["status"][b] == plain["status"][b]


# ---- the CPU oracle's edge check as the verdict
def test_reference_invariants_two_dof_ball_oracle():
    orc = pyoracle.Oracle(scenes.two_dof_ball())
    step = 0.02

    def verdict(QA, QB):
        return orc.valid_edges(QA, QB, step).astype(bool)
    paths = cases.ball_paths()
    W, off = cases.pack(paths)
    assert orc.valid_configs(W).all()
    assert verdict(W[:-1], W[1:])[np.diff(np.repeat(np.arange(2), np.diff(off))) == 0].all()  # the inputs are valid paths
    res = ref.shortcut_paths(W, off, verdict, rounds=16, candidates=64, seed=0)
    cases.check_invariants(W, off, res, verdict)
    cases.check_rounds_prefix(W, off, verdict, res, 2, candidates=64, seed=0)
    assert res["status"].tolist() == [ref.CONVERGED, ref.CONVERGED]
    assert res["n_out"][0] == 2 and res["n_out"][1] > 2
    straight = np.linalg.norm(paths[1][-1] - paths[1][0])
    assert straight < res["length"][1] < ref.arc_lengths(W, np.arange(off[1], off[2]))[-1]
    assert (res["proposed"] > res["accepted"]).all()  # rejected shortcuts: through the wall, or overlapping a better one


@pytest.mark.parametrize("K", [7, 64])
def test_reference_invariants_franka_oracle(K):
    model, qidx, base = cases.franka_planning()
    orc = pyoracle.Oracle(model, planning_qidx=qidx, qpos_base=base)
    step = 0.05
    lo, hi = model.jnt_range[qidx, 0], model.jnt_range[qidx, 1]
    paths = cases.random_walks(lo, hi, lambda Q: orc.valid_configs(Q, nthreads=4).astype(bool), cases.path_lengths(37), seed=11)
    W, off = cases.pack(paths)
    calls = []

    def verdict(QA, QB):
        ok = orc.valid_edges(QA, QB, step, nthreads=4).astype(bool)
        calls.append(ok)
        return ok
    res = ref.shortcut_paths(W, off, verdict, rounds=5, candidates=K, seed=0)
    verdicts = np.concatenate(calls)
    assert verdicts.any() and not verdicts.all()  # accepted and rejected shortcuts
    assert len(verdicts) == res["proposed"].sum()
    cases.check_invariants(W, off, res, verdict)
    cases.check_rounds_prefix(W, off, verdict, res, 2, candidates=K, seed=0)
    assert res["accepted"].sum() > 0
    assert ref.CONVERGED in res["status"]
    if K == 7:  # (64 candidates a round settle every one of these paths within 5 rounds)
        assert ref.ROUNDS in res["status"]
