"""The generated checks with the fused pose helpers of mjpl_pose_f32.h and sincos_half_f32 (what build() generates) against the
same programs generated with pose_fma = False, sincos = False -- plain expressions, sincosf: spec/unfused/, compiled
by __graft_entry__.build() -- on the four models of tests/overlay_models.py.  The binary32 poses of the two differ by
design, so what they hand to the exact re-check may differ; what comes back may not: verdicts and first-bad indices equal
each other's and the oracle's on 4 096 random edges in two rounds, on 512 in one round (fused_single = 1 024 puts the
threshold between the two sizes), on the rows of tests/threshold_cases.py, and on 4 096 configurations, where the numbers
of pairs handed over stay within the 0.1 max + 20 of tests/test_gpu_spec.py.  And sincos_half_f32 on the device returns
the host's bits."""
import ctypes as C
import os

import numpy as np
import pytest

from mjpl_amd import build as build_mod
from mjpl_amd import engine as eng_mod
from mjpl_amd import specialise
from overlay_models import overlay_models
from spec_models import spec_models
from test_threshold_cases_host import cases
from threshold_cases import STEP

pytestmark = pytest.mark.gpu

UNFUSED_DIR = os.path.join(specialise.SPEC_DIR, specialise.UNFUSED_SUBDIR)
KEYS = ("MJPL_SPEC_DIR", "MJPL_SPEC")
IDS = [c[0][0] for c in overlay_models()]


def _engine(m, allowed, qidx, base, **env):
    """An engine made (and its program compiled) under the given MJPL_* variables; the process is left without them."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        with eng_mod.options(fused_single=1024):
            e = eng_mod.Engine(m, allowed)
            e.set_planning(qidx, base)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return e


def _random_edges(m, qidx, n, seed):
    """tests/test_gpu_spec.py's recipe: a third of the edges six times as long, every 97th of length zero."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[qidx, 0], m.jnt_range[qidx, 1]
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    qb = np.clip(qa + rng.choice([0.05, 0.05, 0.3], size=(n, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True), lo, hi)
    qb[::97] = qa[::97]
    return qa, qb


@pytest.fixture(scope="module", params=range(len(IDS)), ids=IDS)
def pair(request, oracle_mod):
    """(entry, index in spec_models(), the default build's engine, the unfused build's engine, the oracle)"""
    entry, _, _ = overlay_models()[request.param]
    name, m, allowed, qidx, base = entry
    which = [e[0] for e in spec_models()].index(name)
    fused = _engine(m, allowed, qidx, base)
    unfused = _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=UNFUSED_DIR)
    try:
        assert fused.spec_kind() == 1, f"{name}: no library of this program (run __graft_entry__.build())"
        assert unfused.spec_kind() == 1, f"{name}: no unfused build under spec/unfused (run __graft_entry__.build())"
        yield entry, which, fused, unfused, oracle_mod.Oracle(m, allowed, planning_qidx=qidx, qpos_base=base)
    finally:
        fused.close()
        unfused.close()
        eng_mod.set_spec_dir(None)


@pytest.mark.parametrize("n", [4096, 512], ids=["two_rounds", "one_round"])
def test_random_edges(pair, oracle_mod, n):
    (name, m, allowed, qidx, base), which, fused, unfused, orc = pair
    qa, qb = _random_edges(m, qidx, n, 700 + which)
    with oracle_mod.portable_trig():
        want, wfb, _ = orc.valid_edges(qa, qb, STEP, nthreads=8, info=True)
    for e in (fused, unfused):
        got, gfb = e.check_edges(qa, qb, STEP, first_bad=True)
        np.testing.assert_array_equal(got, want, err_msg=name)
        np.testing.assert_array_equal(gfb, wfb, err_msg=name)
    assert 0.02 < want.mean() < 0.98, name


def test_threshold_rows(pair):
    (name, m, allowed, qidx, base), which, fused, unfused, _ = pair
    _, c = cases("spec", which, True)
    for e in (fused, unfused):
        np.testing.assert_array_equal(e.check_configs(c.Q), c.valid, err_msg=name)
        for edges in (c.ending, c.through, c.filler):
            got, gfb = e.check_edges(edges.qa, edges.qb, STEP, first_bad=True)
            np.testing.assert_array_equal(got, edges.valid, err_msg=name)
            np.testing.assert_array_equal(gfb, edges.first_bad, err_msg=name)


def test_configurations_and_hand_off_counts(pair, oracle_mod):
    (name, m, allowed, qidx, base), which, fused, unfused, orc = pair
    Q = _random_edges(m, qidx, 4096, 900 + which)[1]
    with oracle_mod.portable_trig():
        want = orc.valid_configs(Q, nthreads=8)
    counts = []
    for e in (fused, unfused):
        np.testing.assert_array_equal(e.check_configs(Q), want, err_msg=name)
        counts.append(e.last_undecided())
    print(f"{name}: pairs handed to the exact re-check, fused / unfused: {counts}")
    assert abs(counts[0] - counts[1]) <= 0.1 * max(counts) + 20, (name, counts)


def test_device_sincos_half_returns_the_hosts_bits():
    """2^20 arguments of the host sweep (tests/test_pose_fma.py: every 64th binary32 of [-3.3, 3.3]), evenly thinned, both
    signs, in one launch."""
    assert os.path.exists(build_mod.POSE_PROBE_LIB), f"{build_mod.POSE_PROBE_LIB}: run __graft_entry__.build()"
    lib = C.CDLL(build_mod.POSE_PROBE_LIB)
    top = int(np.float32(3.3).view(np.uint32))
    mags = (np.linspace(0, top // 64, 1 << 19).astype(np.uint32) * np.uint32(64)).view(np.float32)
    x = np.ascontiguousarray(np.concatenate([mags, -mags]))
    assert len(x) == 1 << 20 and np.abs(x).max() <= np.float32(3.3)
    F = C.POINTER(C.c_float)
    out = [np.zeros_like(x) for _ in range(4)]
    lib.mjpl_probe_sincos_host(x.ctypes.data_as(F), out[0].ctypes.data_as(F), out[1].ctypes.data_as(F), C.c_long(len(x)))
    status = lib.mjpl_probe_sincos_device(x.ctypes.data_as(F), out[2].ctypes.data_as(F), out[3].ctypes.data_as(F), C.c_long(len(x)))
    assert status == 0, f"HIP status {status}"
    assert np.array_equal(out[0].view(np.uint32), out[2].view(np.uint32)) and np.array_equal(out[1].view(np.uint32), out[3].view(np.uint32))
    assert np.abs(out[2] - np.sin(x.astype(np.float64))).max() <= 4 * 2.0 ** -24
    assert np.abs(out[3] - np.cos(x.astype(np.float64))).max() <= 4 * 2.0 ** -24
