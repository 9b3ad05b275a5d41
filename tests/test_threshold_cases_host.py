"""tests/threshold_cases.py on the CPU: what tests/test_gpu_spec_adversarial.py takes for granted about its inputs.  Per
entry of spec_models() and per scene of the generic libraries, under both of the oracle's sin/cos: the bisection ends on
adjacent values; the oracle's verdicts on the probes change at most once with the offset on either side of the
threshold, and not before 1e-7 (a line that grazes a contact region would flip back: another seed, not fewer rows);
both verdicts occur among the edges of each shape and a waypoint of the through-edges is the probe; at least one offset
beyond 0 is "near".  Over the models together the flipping pairs cover all nine type pairs."""
import functools

import numpy as np
import pytest

import threshold_cases as tc
from mjpl_amd import scenes
from spec_models import generic_scenes, spec_models

SEED = 1


def generic_cases():
    """The scenes a robot's generic library serves (expected kind 2) as entries like those of spec_models()."""
    out = []
    for name, m, kind in generic_scenes():
        if kind == 2:
            out.append((name, m, (), scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()))
    return out


@functools.lru_cache(maxsize=None)
def entries(kind):
    return spec_models() if kind == "spec" else generic_cases()


@functools.lru_cache(maxsize=None)
def cases(kind, which, portable):
    """(entry, Cases) -- computed once per session, shared, never written to.  With libm's sin/cos the offsets from
    1e-9 up only: two libm's differ in the last bit of some sin/cos themselves."""
    from oracle import pyoracle
    pyoracle.build()
    entry = entries(kind)[which]
    _, m, allowed, qidx, base = entry
    if portable:
        with pyoracle.portable_trig():
            return entry, tc.build(pyoracle, m, allowed, qidx, base, seed=SEED)
    return entry, tc.build(pyoracle, m, allowed, qidx, base, seed=SEED, offsets=tc.OFFSETS[tc.OFFSETS > 0])


ALL = [("spec", i) for i in range(len(spec_models()))] + [("generic", i) for i in range(len(generic_cases()))]


@pytest.mark.parametrize("portable", [True, False], ids=["portable_trig", "libm"])
@pytest.mark.parametrize("kind,which", ALL, ids=[f"{k}{i}" for k, i in ALL])
def test_cases_are_what_the_gpu_tests_assume(oracle_mod, kind, which, portable):
    (name, m, allowed, qidx, base), c = cases(kind, which, portable)
    n, noff = tc.ROWS, len(c.offsets)
    assert c.A.shape == c.B.shape == c.q_free.shape == c.q_hit.shape == (n, len(qidx))
    assert len(c.Q) == 2 * noff * n < 2000 and len(c.ending.qa) + len(c.through.qa) + len(c.filler.qa) < 6000
    assert (np.abs(c.q_hit - c.q_free) <= tc.adjacency_slack(c.A, c.B)).all(), name
    # verdicts per (offset, side, row)
    v = c.valid.reshape(noff, 2, n).astype(bool)
    free, hit = v[:, 0, :], ~v[:, 1, :]     # True while the probe still has the verdict of its side
    small = c.offsets <= 1e-7
    assert small.any()
    for side, tag in ((free, "free"), (hit, "hit")):
        bad = np.flatnonzero(~side[small].all(axis=0))
        assert bad.size == 0, f"{name}: {tag} side flips within 1e-7 of the threshold in rows {bad.tolist()}"
        flips = (side[1:] != side[:-1]).sum(axis=0)
        bad = np.flatnonzero(flips > 1)
        assert bad.size == 0, f"{name}: {tag} side is not monotone in the offset in rows {bad.tolist()}: the line grazes"
    assert 0 < c.valid.sum() < len(c.valid)
    # edges: both verdicts in each shape; a through-edge's third waypoint is its probe
    for e in (c.ending, c.through, c.filler):
        assert ((e.valid == 0) == (e.first_bad >= 0)).all()
    for e in (c.ending, c.through):
        assert 0 < e.valid.sum() < len(e.valid), name
    assert c.filler.valid.mean() > 0.5, name   # (there to be certified)
    from oracle import pyoracle
    for i in range(0, len(c.Q), 97):
        w = pyoracle.step(c.through.qa[i], c.through.qb[i], tc.STEP)
        assert np.abs(w - c.Q[i]).max() <= 4 * np.spacing(np.abs(c.Q[i]).max() + tc.STEP), name
    # ... so where the edge's end is free, the probe decides it (from 1e-9 on: the waypoint is the probe but for rounding)
    decides = (c.through.first_bad != 0) & (c.off >= 1e-9)
    assert decides.sum() > 0.5 * len(c.Q), name
    assert ((c.through.first_bad == 1) == (c.valid == 0))[decides].all(), name
    assert ((c.ending.first_bad == 0) == (c.valid == 0)).all()
    # "near"
    assert c.near[c.off == c.offsets[0]].all()
    assert (c.near & (c.off > 0)).any(), (name, c.L)
    assert not c.near[c.off >= 1e-5].any()   # (L >= nq >= 2)
    # the flipping pairs are candidates of the right types
    assert (c.types[:, 0] <= c.types[:, 1]).all() and set(np.unique(c.types)) <= set(tc.TYPE_NAMES)
    print(f"{name} [{'portable' if portable else 'libm'} trig]: L = {c.L:.2f}, near offsets "
          f"{sorted(set(c.off[c.near].tolist()))}, flipping pairs {c.type_histogram()}")


def test_flipping_pairs_cover_all_nine_type_pairs(oracle_mod):
    seen = {}
    for i in range(len(spec_models())):
        (name, *_), c = cases("spec", i, True)
        for k, cnt in c.type_histogram().items():
            seen[k] = seen.get(k, 0) + cnt
    print("flipping type pairs over spec_models():", seen)
    assert set(seen) == set(tc.NINE_TYPE_PAIRS), sorted(set(tc.NINE_TYPE_PAIRS) ^ set(seen))
