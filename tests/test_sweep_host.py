"""Certified edge checks, the parts that need no GPU: the C ABI of mjpl_sweep_* (declared in include/mjpl_hip.h,
exported by the built library, bound by mjpl_amd.engine), the pair lever table of the host-only export
mjpl_sweep_levers against the NumPy statement (tests/sweep_reference.py), and the property the certificate rests on:
no pair's distance changes by more than sum_c |dq_c| W[p][c] (distances from tests/distance_reference.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import distance_reference as ref
import sweep_reference as sref
from mjpl_amd import build as _build
from mjpl_amd import engine, scenes
from test_gpu_contacts import candidate_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_sweep_levers", "mjpl_sweep_bounds", "mjpl_sweep_measure", "mjpl_sweep_measure_dev", "mjpl_sweep_edges",
           "mjpl_sweep_edges_dev")
PROPERTY_ROWS = 2000


def sweep_models():
    """(name, model, allowed body pairs, qidx, qpos_base, lo, hi): lo / hi over the planning columns, the joint ranges
    (finite for every slide joint)."""
    from test_gpu_models import random_model
    out = []

    def add(name, m, allowed, qidx, base):
        qidx = np.asarray(qidx, np.int32)
        rng = np.asarray(m.jnt_range, float)[qidx]
        out.append((name, m, tuple(allowed), qidx, np.asarray(base, float).copy(), rng[:, 0].copy(), rng[:, 1].copy()))

    m = scenes.franka_p(obstacles=True)
    add("franka_p+16obs, arm", m, (), scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos)
    add("franka_p+16obs, nine joints", m, (), np.arange(m.nq), m.qpos0)
    u = scenes.ur5e()
    add("ur5e", u, (), np.arange(u.nq), u.qpos0)
    tb = scenes.two_dof_ball()
    add("two_dof_ball", tb, (), np.arange(tb.nq), tb.qpos0)
    for seed, boxes in ((1002, False), (1005, False), (1003, True), (1004, True)):
        rm, allowed = random_model(seed, moving_boxes=boxes)
        add(f"random_model({seed})", rm, allowed, np.arange(rm.nq), rm.qpos0)
    return out


MODELS = sweep_models()
IDS = [x[0] for x in MODELS]


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mjpl_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_build.build_hip())
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine.ABI, f"{name} is not bound"
    assert "mjpl_sweep_desc" in header
    for k, name in enumerate(("SWEEP_FREE", "SWEEP_HIT", "SWEEP_UNDECIDED", "SWEEP_NONFINITE", "SWEEP_RANGE")):
        assert getattr(engine, name) == k and re.search(rf"#define MJPL_{name}\s+{k}\b", header), name
    assert len(engine.ABI["mjpl_sweep_edges"][1]) == len(engine.ABI["mjpl_sweep_edges_dev"][1]) == 12
    assert len(engine.ABI["mjpl_sweep_measure"][1]) == len(engine.ABI["mjpl_sweep_measure_dev"][1]) == 10
    assert engine.ABI["mjpl_sweep_edges"][1][1] == ctypes.POINTER(engine.SweepDesc)
    assert ctypes.sizeof(engine.SweepDesc) == 2 * 8 + 4 + 4 + 2 * 8
    from mjpl_amd import CertifiedIntervals, ClearanceConstraint, CollisionConstraint
    assert hasattr(CollisionConstraint, "certified_interval") and hasattr(CollisionConstraint, "certified_edges_planning")
    assert hasattr(ClearanceConstraint, "certified_interval") and not hasattr(ClearanceConstraint, "valid_interval")
    assert hasattr(CertifiedIntervals, "valid_interval") and hasattr(CertifiedIntervals, "valid_intervals")


@pytest.mark.parametrize("name,m,allowed,qidx,base,lo,hi", MODELS, ids=IDS)
def test_levers_equal_the_numpy_table(name, m, allowed, qidx, base, lo, hi):
    pairs, _ = candidate_table(m, allowed)
    W = engine.sweep_levers(m, allowed, qidx, base, lo, hi)
    want = sref.lever_table(m, pairs, qidx, base, lo, hi)
    assert W.shape == want.shape == (len(pairs), len(qidx))
    assert np.array_equal(W == 0, want == 0), "zeros are exactly zero, and nowhere else"
    assert np.isfinite(W).all() and (W >= 0).all()
    nz = want != 0
    assert np.all(np.abs(W[nz] - want[nz]) <= 1e-12 * np.abs(want[nz]))
    assert nz.any()


def test_a_planning_slide_without_bounds_gives_inf_below_it():
    # Franka-P, nine joints: the finger slides hang below all seven hinges
    name, m, allowed, qidx, base, lo, hi = MODELS[1]
    pairs, _ = candidate_table(m, allowed)
    W = engine.sweep_levers(m, allowed, qidx, base)
    want = sref.lever_table(m, pairs, qidx, base)
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(W), ~fin) and np.isinf(W).any()
    assert np.all(np.abs(W[fin] - want[fin]) <= 1e-12 * np.abs(want[fin]))
    jtype, jq = np.asarray(m.jnt_type), [int(a) for a in m.jnt_qposadr]
    slides = [c for c, a in enumerate(qidx) if jtype[jq.index(int(a))] == sref.JT_SLIDE]
    assert slides
    bid = np.asarray(m.geom_bodyid)
    jbody = {int(m.jnt_qposadr[m.body_jntadr[b] + k]): b for b in range(m.nbody) for k in range(m.body_jntnum[b])}
    slide_bodies = {jbody[int(qidx[c])] for c in slides}
    # every inf sits in a hinge column of a pair with a geom on a slide's body; slide columns themselves read 1 or 0
    rows, cols = np.nonzero(np.isinf(W))
    assert all(c not in slides for c in cols)
    assert all(bid[pairs[p][0]] in slide_bodies or bid[pairs[p][1]] in slide_bodies for p in rows)
    assert set(np.unique(W[:, slides])) <= {0.0, 1.0}
    # ... and with the bounds every lever is finite
    assert np.isfinite(engine.sweep_levers(m, allowed, qidx, base, lo, hi)).all()


@pytest.mark.parametrize("name,m,allowed,qidx,base,lo,hi", MODELS, ids=IDS)
def test_no_distance_changes_by_more_than_the_levers_allow(name, m, allowed, qidx, base, lo, hi):
    pairs, _ = candidate_table(m, allowed)
    W = engine.sweep_levers(m, allowed, qidx, base, lo, hi)
    rng = np.random.default_rng(11)
    n, nplan = PROPERTY_ROWS, len(qidx)
    Q = rng.uniform(lo, hi, size=(n, nplan))
    move = rng.uniform(-0.3, 0.3, size=(n, nplan))
    single = np.arange(n) % 2 == 0  # half of the moves are along one column
    only = rng.integers(0, nplan, size=n)
    move[single] *= (np.arange(nplan)[None, :] == only[single, None])
    Q2 = np.clip(Q + move, lo, hi)

    def full(S):
        F = np.tile(base, (len(S), 1))
        F[:, qidx] = S
        return F

    D = ref.reference_distances(m, full(np.concatenate([Q, Q2])), pairs)
    d1, d2 = D[:n], D[n:]
    bound = np.abs(Q2 - Q) @ W.T  # [n, P]
    worst = np.max(np.abs(d2 - d1) - bound)
    big = bound > 1e-6
    print(f"{name}: {len(pairs)} pairs, largest |dd| - bound = {worst:.3e}, largest |dd| / bound (bound > 1e-6) = "
          f"{np.max((np.abs(d2 - d1) / np.where(big, bound, 1.0))[big]):.3f}")
    assert np.all(np.abs(d2 - d1) <= bound + 1e-9)
