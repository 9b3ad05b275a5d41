"""mjpl_amd/csrc/mjpl_overlay.h, queue_drain<float, BOXQ, ALL, false>: the drain whose undecided candidates have their
waypoints rebuilt by the whole wave (lane k holds planning column k) instead of by one lane.  The recurrence is
exact_waypoint's, operation for operation, so against spec/plain/ -- the same text WITHOUT the overlay, which
__graft_entry__.build() makes -- everything must be equal bit for bit: verdicts, first-bad indices, item and
interior-edge counts, the number of pairs handed to the exact re-check and the set of (edge, index, geom, geom) handed
over.  Verdicts and indices hang on the rebuilt rows: the exact kernels decide from them.  On a batch with invalid
edges, how many waypoints BEHIND an edge's first bad one are looked at depends on the order the waves take tiles in, so
counts and sets of hand-offs are compared on the batch's valid edges, where every waypoint is looked at.
The four models of tests/overlay_models.py: slot files 8, 4 and 16 wide, and moving boxes (MBOX: not specialised)."""
import os

import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import specialise
from overlay_models import PLAIN_SUBDIR, overlay_models
from spec_models import spec_models
from test_threshold_cases_host import cases
from threshold_cases import STEP

pytestmark = pytest.mark.gpu

PLAIN_DIR = os.path.join(specialise.SPEC_DIR, PLAIN_SUBDIR)
KEYS = ("MJPL_SPEC_DIR", "MJPL_SPEC", "MJPL_FUSED_SINGLE", "MJPL_FUSED_POOL")
MODELS = pytest.mark.parametrize("case", range(len(overlay_models())), ids=[c[0][0] for c in overlay_models()])

# (edges, variables of the engines): two rounds over the pool (endpoint tiles, then item tiles), the same edges in one
# round, and two rounds over a ring of pool entries small enough to be written several times over
TWO_ROUNDS, ONE_ROUND = {"MJPL_FUSED_SINGLE": 0}, {"MJPL_FUSED_SINGLE": 100000000}
SHAPES = ((4096, TWO_ROUNDS), (4096, ONE_ROUND), (40000, {"MJPL_FUSED_SINGLE": 0, "MJPL_FUSED_POOL": 320}))


def _engine(m, allowed, qidx, base, **env):
    """An engine made (and its program compiled) under the given MJPL_* variables; the process is left without them."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        e = eng_mod.Engine(m, allowed)
        e.set_planning(qidx, base)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return e


def _pair(entry, **env):
    """(this build, the build without the overlay) of a model's library."""
    _, m, allowed, qidx, base = entry
    new, plain = _engine(m, allowed, qidx, base, **env), _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=PLAIN_DIR, **env)
    assert new.spec_kind() == 1 and plain.spec_kind() == 1, f"{entry[0]}: a library is missing (run __graft_entry__.build())"
    return new, plain


def _close(*engines):
    for e in engines:
        e.close()
    eng_mod.set_spec_dir(None)


def _random_edges(m, qidx, n, seed):
    """tests/test_gpu_spec.py's recipe: a third of the edges six times as long, every 97th of length zero."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[qidx, 0], m.jnt_range[qidx, 1]
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    qb = np.clip(qa + rng.choice([0.05, 0.05, 0.3], size=(n, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True), lo, hi)
    qb[::97] = qa[::97]
    return qa, qb


def _handed(e):
    """(pairs handed over by the last launch, their sorted (edge, index, geom, geom) rows)"""
    total, edge, idx, ga, gb = e.undecided_pairs()
    assert len(edge) == total  # (the record is complete)
    rows = np.stack([edge, idx, ga, gb], axis=1)
    return total, rows[np.lexsort(rows.T[::-1])]


def _edge_launch(e, qa, qb):
    v, fb = e.check_edges(qa, qb, STEP, first_bad=True)
    return v, fb, e.last_items(), e.last_interior_edges()


def _compare_edges(new, plain, qa, qb, tag):
    """Both builds on the batch, then on its valid edges alone -> hand-offs of the valid edges."""
    (v, fb, items, interior), (pv, pfb, pitems, pinterior) = _edge_launch(new, qa, qb), _edge_launch(plain, qa, qb)
    np.testing.assert_array_equal(v, pv, err_msg=tag)
    np.testing.assert_array_equal(fb, pfb, err_msg=tag)
    assert (items, interior) == (pitems, pinterior), tag
    keep = v != 0
    assert keep.any(), tag
    va, vb = np.ascontiguousarray(qa[keep]), np.ascontiguousarray(qb[keep])
    seen = []
    for e in (new, plain):
        vv, _, vitems, vinterior = _edge_launch(e, va, vb)
        assert vv.all(), tag
        seen.append((e.last_undecided(), vitems, vinterior, *_handed(e)))
    assert seen[0][:4] == seen[1][:4], (tag, seen[0][:4], seen[1][:4])
    np.testing.assert_array_equal(seen[0][4], seen[1][4], err_msg=tag)
    return v, items, seen[0][3]


@MODELS
@pytest.mark.parametrize("n,env", SHAPES, ids=["two_rounds", "one_round", "ring_wraps"])
def test_random_edges(case, n, env):
    entry, _, _ = overlay_models()[case]
    name, m, _, qidx, _ = entry
    new, plain = _pair(entry, **env)
    try:
        v, items, _ = _compare_edges(new, plain, *_random_edges(m, qidx, n, 500 + case), f"{name}, {n} edges, {env}")
        assert items > 0 and 0.02 < v.mean() < 0.98, name
    finally:
        _close(new, plain)


@pytest.mark.parametrize("case", (0, 3), ids=[overlay_models()[c][0][0] for c in (0, 3)])
def test_dense_contact_overflows_a_queue(case):
    """512 edges of the two Franka models with the elbow in the folded tenth of its range: the forearm lies along the
    upper arm, the 64 configurations of a wave pass more culls than the 64 records its queue holds, and batches leave
    in mid-stage (queue_push's own drain) as well as at the end of a configuration."""
    entry, _, _ = overlay_models()[case]
    name, m, _, qidx, _ = entry
    rng = np.random.default_rng(11)
    lo, hi = m.jnt_range[qidx, 0].copy(), m.jnt_range[qidx, 1].copy()
    hi[3] = lo[3] + 0.1 * (hi[3] - lo[3])
    qa = rng.uniform(lo, hi, size=(512, len(qidx)))
    d = rng.normal(size=qa.shape)
    qb = np.clip(qa + 0.05 * d / np.linalg.norm(d, axis=1, keepdims=True), lo, hi)
    for env in (TWO_ROUNDS, ONE_ROUND):
        new, plain = _pair(entry, **env)
        try:
            v, items, _ = _compare_edges(new, plain, qa, qb, f"{name}, dense contact, {env}")
            assert 0 < v.sum() < len(v), name
        finally:
            _close(new, plain)


@MODELS
def test_threshold_rows_are_handed_over_alike(oracle_mod, case):
    """The rows of tests/threshold_cases.py: configurations and waypoints within 1e-9 .. 1e-3 of a contact threshold, so
    hand-offs happen on every row.  Verdicts equal the oracle's as well (the rebuilt waypoints are what decides)."""
    entry, _, _ = overlay_models()[case]
    name, m, _, qidx, _ = entry
    _, c = cases("spec", [e[0] for e in spec_models()].index(name), True)
    new, plain = _pair(entry)
    try:
        got = [(e.check_configs(c.Q), e.last_undecided(), *_handed(e)) for e in (new, plain)]
        np.testing.assert_array_equal(got[0][0], got[1][0], err_msg=name)
        np.testing.assert_array_equal(got[0][0], c.valid, err_msg=name)
        assert got[0][1:3] == got[1][1:3] and got[0][2] > 0, (name, got[0][1:3], got[1][1:3])
        np.testing.assert_array_equal(got[0][3], got[1][3], err_msg=name)
        for shape in ("ending", "through"):
            ed = getattr(c, shape)
            v, _, handed = _compare_edges(new, plain, ed.qa, ed.qb, f"{name}, edges {shape}")
            np.testing.assert_array_equal(v, ed.valid, err_msg=f"{name}, edges {shape}")
            assert handed > 0, (name, shape)
    finally:
        _close(new, plain)


@MODELS
def test_configurations(case):
    """check_configs on 4 096 configurations: verdicts, the undecided count and the pairs handed over."""
    entry, _, _ = overlay_models()[case]
    name, m, _, qidx, _ = entry
    Q = _random_edges(m, qidx, 4096, 700 + case)[0]
    new, plain = _pair(entry)
    try:
        got = [(e.check_configs(Q), e.last_undecided(), *_handed(e)) for e in (new, plain)]
        np.testing.assert_array_equal(got[0][0], got[1][0], err_msg=name)
        assert got[0][1:3] == got[1][1:3], (name, got[0][1:3], got[1][1:3])
        np.testing.assert_array_equal(got[0][3], got[1][3], err_msg=name)
        assert 0.02 < got[0][0].mean() < 0.98, name
    finally:
        _close(new, plain)


@pytest.mark.parametrize("case", (0, 1, 2), ids=[overlay_models()[c][0][0] for c in (0, 1, 2)])
def test_interpreting_kernels_against_the_oracle(oracle_mod, case):
    """The interpreting kernels of libmjpl_hip.so (the same drain, instantiated 8, 4 and 16 slots wide) on the edges of
    the first test, in both launch shapes, against the CPU oracle."""
    (name, m, allowed, qidx, base), _, _ = overlay_models()[case]
    qa, qb = _random_edges(m, qidx, 4096, 500 + case)
    orc = oracle_mod.Oracle(m, allowed, planning_qidx=qidx, qpos_base=base)
    want, want_fb, _ = orc.valid_edges(qa, qb, STEP, nthreads=8, info=True)
    for env in (TWO_ROUNDS, ONE_ROUND):
        e = _engine(m, allowed, qidx, base, MJPL_SPEC=0, **env)
        try:
            assert e.spec_kind() == 0
            v, fb = e.check_edges(qa, qb, STEP, first_bad=True)
            np.testing.assert_array_equal(v, want, err_msg=f"{name}, {env}")
            np.testing.assert_array_equal(fb, want_fb, err_msg=f"{name}, {env}")
        finally:
            _close(e)
