"""The never-touch set on the GPU: the benchmark model's own library leaves the pairs of the set out of
its generated check; verdicts and first-bad indices are those of the interpreting kernels (which test every pair of
ip) and of the CPU oracle -- at a batch of two tiles, in single-round mode, just above it, and on configurations with
angles beyond the full circle."""
import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes

pytestmark = pytest.mark.gpu

STEP = 0.01
SIZES = (65, 4096, 33000)  # two tiles; one round of checks; just above option "fused_single" (32 768)


def _model():
    m = scenes.franka_p(obstacles=True)
    return m, scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()


def _edges(m, qidx, n, seed):
    """bench.py's recipe (q_a uniform in the joint ranges, a normalised Gaussian direction, clipped), with every 7th edge
    90 steps long instead of 5 and every 13th of length zero."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[qidx, 0], m.jnt_range[qidx, 1]
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    eps = np.full((n, 1), 0.05)
    eps[::7] = 0.9
    qb = np.clip(qa + eps * d, lo, hi)
    qb[::13] = qa[::13]
    return qa, qb


@pytest.fixture(scope="module")
def engines():
    m, qidx, base = _model()
    spec = eng_mod.Engine(m)
    spec.set_planning(qidx, base)
    interp = eng_mod.Engine(m)
    interp.set_planning(qidx, base)
    interp.set_spec(0)
    yield m, qidx, base, spec, interp
    spec.close()
    interp.close()


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """The oracle's verdicts and first-bad indices per batch size: computed once, shared, never written to."""
    m, qidx, base = _model()
    out = {}
    with oracle_mod.portable_trig():
        orc = oracle_mod.Oracle(m, planning_qidx=qidx, qpos_base=base)
        for n in SIZES:
            qa, qb = _edges(m, qidx, n, 40 + n)
            want, wfb, _ = orc.valid_edges(qa, qb, STEP, nthreads=8, info=True)
            for a in (qa, qb, want, wfb):
                a.setflags(write=False)
            out[n] = (qa, qb, want, wfb)
        rng = np.random.default_rng(5)
        q = rng.uniform(-6.5, 6.5, size=(2048, len(qidx)))
        wantc = orc.valid_configs(q, nthreads=8)
        q.setflags(write=False)
        wantc.setflags(write=False)
        out["wide"] = (q, wantc)
    return out


def test_the_library_in_use_leaves_pairs_out(engines):
    m, qidx, base, spec, interp = engines
    assert spec.spec_kind() == 1, "no per-program library for the benchmark model (run __graft_entry__.build())"
    assert not spec.info()["filter_interpreter"]
    assert spec.get_option("pairs_never_touch") >= 2 and spec.get_option("prune_contact_evals") > 0
    assert interp.spec_kind() == 0 and interp.get_option("pairs_never_touch") == spec.get_option("pairs_never_touch")
    # the tables keep the pairs: the counts are those of a program without the stage
    spec.set_option("prune_contacts", 0)
    spec.set_planning(qidx, base)
    try:
        assert spec.get_option("pairs_never_touch") == 0
        off = spec.info()
    finally:
        spec.set_option("prune_contacts", 1)
        spec.set_planning(qidx, base)
    on = spec.info()
    assert spec.spec_kind() == 1 and (on["npairs"], on["npairs_world"]) == (off["npairs"], off["npairs_world"])


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_equal_interpreter_and_oracle(engines, reference, n):
    m, qidx, base, spec, interp = engines
    qa, qb, want, wfb = reference[n]
    assert spec.spec_kind() == 1 and interp.spec_kind() == 0
    assert (np.abs(qb - qa).sum(axis=1) == 0).any() and (np.linalg.norm(qb - qa, axis=1) > 64 * STEP).any()
    assert 0.02 < want.mean() < 0.98
    for e in (spec, interp):
        got, gfb = e.check_edges(qa, qb, STEP, first_bad=True)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(gfb, wfb)


def test_configurations_beyond_the_full_circle(engines, reference):
    m, qidx, base, spec, interp = engines
    q, wantc = reference["wide"]
    assert spec.spec_kind() == 1
    np.testing.assert_array_equal(spec.check_configs(q), wantc)
    np.testing.assert_array_equal(interp.check_configs(q), wantc)


def test_hand_offs_do_not_increase(engines, reference):
    """Pairs handed to the exact pair re-check on a configuration launch (on edges the count depends on the order the
    waves take waypoints in): no more than with the option off (build() compiles that program's library, too)."""
    m, qidx, base, spec, interp = engines
    q = reference[4096][1]
    spec.check_configs(q)
    with_set = spec.last_undecided()
    print("hand-offs with the set:", with_set)
    spec.set_option("prune_contacts", 0)
    spec.set_planning(qidx, base)
    try:
        assert spec.spec_kind() == 1, "no library of the program without the set (run __graft_entry__.build())"
        spec.check_configs(q)
        without = spec.last_undecided()
    finally:
        spec.set_option("prune_contacts", 1)
        spec.set_planning(qidx, base)
    print("hand-offs without:", without)
    assert with_set <= without
