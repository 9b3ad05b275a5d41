"""Near pairs, the parts that need no GPU: the C ABI of mjpl_near_pairs* (declared in include/mjpl_hip.h, exported by
the built library, bound by mjpl_amd.engine), and the study that pins the inputs of the GPU test's central-difference
check (tests/test_gpu_near_pairs.py): on its rows the NumPy reference lists 845 near pairs, and central differences of
the reference at h and h / 2 agree on all of them."""
import ctypes
import os
import re

import numpy as np

import distance_reference as ref
import near_reference as nref
from mjpl_amd import build as _build
from mjpl_amd import engine, scenes
from helpers import uniform_configs
from test_gpu_contacts import candidate_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_near_pairs", "mjpl_near_pairs_dev")

# the central-difference study: the rows, distmax and step of test_gpu_near_pairs.py
FD_ROWS, FD_SEED, FD_DISTMAX, FD_H = 96, 43, 0.1, 1e-6


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mjpl_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_build.build_hip())
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine.ABI, f"{name} is not bound"
    # K sits behind distmax in both, the outputs in the header's order
    assert len(engine.ABI["mjpl_near_pairs"][1]) == len(engine.ABI["mjpl_near_pairs_dev"][1]) == 13
    assert engine.ABI["mjpl_near_pairs"][1][4:6] == [ctypes.c_double, ctypes.c_int32]


def test_reference_list_and_its_central_differences():
    m = scenes.franka_p(obstacles=True)
    pairs, allowed = candidate_table(m)  # (what engine.contact_pairs() returns: tests/test_gpu_contacts.py)
    assert len(pairs) == 213
    Q = uniform_configs(m, FD_ROWS, seed=FD_SEED)
    rows, D = nref.near_pairs(m, Q, pairs, allowed, FD_DISTMAX)
    i, p, d = nref.flatten(rows)
    assert len(p) == 845, len(p)
    assert np.all(d < FD_DISTMAX) and max(len(r[0]) for r in rows) <= 32
    for pp, _ in rows:
        assert np.all(np.diff(pp) > 0)
    fd_h, fd_h2 = nref.central_differences(lambda S: ref.reference_distances(m, S, pairs), Q, FD_H)
    steady = np.all(np.abs(fd_h[i, :, p] - fd_h2[i, :, p]) <= 1e-8, axis=1)
    print(f"reference: {len(p)} listed, {int(steady.sum())} with central differences at h and h/2 within 1e-8")
    assert steady.mean() >= 0.95, (int(steady.sum()), len(p))
