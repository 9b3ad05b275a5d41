"""Push-out, the parts that need no GPU: the C ABI of mjpl_push_out* (declared in include/mjpl_hip.h, exported by the
built library, bound by mjpl_amd.engine) with ClearanceConstraint importable, and the study that pins the inputs of the
GPU test (tests/test_gpu_push_out.py): the NumPy statement of the iteration (tests/push_reference.py), fed by the
reference distances with central differences, brings at least 0.85 of the rows that need a push to the clearance
within 16 iterations."""
import ctypes
import os
import re

import numpy as np

import distance_reference as ref
import push_reference as pref
from mjpl_amd import build as _build
from mjpl_amd import engine, scenes
from helpers import uniform_configs
from test_gpu_contacts import candidate_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_push_out", "mjpl_push_out_dev")

# the study: the rows, clearance and central-difference step the GPU test shares
PUSH_ROWS, PUSH_SEED, PUSH_DMIN, PUSH_H, PUSH_K = 128, 7, 0.02, 1e-6, 16
PUSH_SHARE = 0.85  # of the rows that need a push, those that must end with clearance >= d_min


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mjpl_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_build.build_hip())
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine.ABI, f"{name} is not bound"
    assert "mjpl_push_desc" in header
    for k, name in enumerate(("PUSH_OK", "PUSH_STUCK", "PUSH_DEGENERATE", "PUSH_NONFINITE")):
        assert getattr(engine, name) == k and re.search(rf"#define MJPL_{name}\s+{k}\b", header), name
    # the descriptor behind the engine, the outputs in the header's order, the same count in both forms
    assert len(engine.ABI["mjpl_push_out"][1]) == len(engine.ABI["mjpl_push_out_dev"][1]) == 10
    assert engine.ABI["mjpl_push_out"][1][1] == ctypes.POINTER(engine.PushDesc)
    assert ctypes.sizeof(engine.PushDesc) == 4 * 8 + 2 * 4 + 2 * 8
    from mjpl_amd import ClearanceConstraint
    from mjpl_amd.constraint import ClearanceConstraint as C2
    assert ClearanceConstraint is C2 and ClearanceConstraint.projects is True


def test_reference_iteration_reaches_the_clearance():
    m = scenes.franka_p(obstacles=True)
    pairs, allowed = candidate_table(m)
    margins = ref.pair_margins(m, pairs)
    dstar = PUSH_DMIN + margins[~allowed].max()
    Q = uniform_configs(m, PUSH_ROWS, seed=PUSH_SEED)

    def distances(S):
        return ref.reference_distances(m, S, pairs)

    def clearance(S):
        return ref.clearance_from(np.minimum(distances(S), dstar), margins, allowed)[0]

    start = clearance(Q)
    needing = start < PUSH_DMIN
    near = pref.fd_near(distances, allowed, dstar, PUSH_K, PUSH_H)
    Q_out, iters, degenerate, _decision, _w = pref.push_out(near, Q, margins, PUSH_DMIN)
    end = clearance(Q_out)
    ok = end >= PUSH_DMIN
    print(f"needing {int(needing.sum())} of {PUSH_ROWS}, converged {int((ok & needing).sum())}, "
          f"most steps of a converged row {int(iters[ok & needing].max())}, degenerate {int(degenerate.sum())}")
    # rows that need no push are not moved
    assert np.array_equal(Q_out[~needing], Q[~needing]) and np.all(iters[~needing] == 0)
    assert np.all(iters[needing] >= 1)
    assert needing.sum() >= 64  # (the study has something to push)
    assert (ok & needing).sum() >= PUSH_SHARE * needing.sum(), (int((ok & needing).sum()), int(needing.sum()))
    assert iters[ok & needing].max() <= 12
