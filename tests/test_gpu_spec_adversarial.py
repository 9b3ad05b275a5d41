"""Threshold parity of the GENERATED per-model libraries (mjpl_amd/specialise.py, DESIGN.md sections 3 and 5.6).

tests/test_gpu_filter_adversarial.py bisects every routine's contact threshold, on models made for it: no library is
prebuilt for those, so its engines run the interpreting kernels.  The code of the headline path -- straight-line FK with
literals, static-partner culls in expanded form (for a sphere partner the cull IS the contact test), stored partners
read through the overlay, partners from a scene table, the exact re-check with folded float64 constants, the
certificate and float64 builds, the code generation option -- met the oracle on uniformly random inputs only, which
almost never land within 1e-4 m of a threshold.  Here the threshold is bisected on the very models the libraries are
built for (tests/threshold_cases.py; its assumptions are checked on the CPU by tests/test_threshold_cases_host.py):
96 rows, 20 probes a row at offsets from 0 to 1e-3 on either side, edges that end on a probe and edges with a waypoint
on one.  Each case runs twice, like the suite it extends: against the oracle with its bit-reproducible sin/cos (every
offset) and with libm's (offsets from 1e-9 up).  Everything at the default band: a library is tied to its filter_tol.

What a shrunk cull constant does here, worked out on the CPU from the emitted text of random_model(1002), row 67 of
its cases (static sphere 4 against moving sphere 12, contact at |c - X| = 0.184994 m, |X| = 0.81 m), the cull
fl(|c|^2 - 2 c.X) <= THR evaluated in binary32 on the oracle's centres.  THR = (r + tol)^2 - |X|^2 + allowance, emitted
as -0x1.3bad86p-1f = -0.6165583: the allowance (specialise.expanded_threshold) is 2.3e-6 m^2 of it, 6e-6 m at this
radius, the tolerance 3.7e-5 m^2.  Dropping the allowance ALONE moves no probe across the cull: the tolerance's
widening, 1e-4 m, is sixteen times as wide (in this row the bounding spheres are the geoms), and that margin is the filter's
budget for its binary32 poses, not the form's rounding -- no test at any offset can see it, short of coordinates where
the allowance outgrows the tolerance.  Dropping the widening as well -- THR = r^2 - |X|^2, the band constant gone --
fails the cull for this row's free-side probes from 1e-7 up (3.5e-8 m from contact): "near" probes that are not handed
to the re-check, which _band reports probe by probe (the count alone would not: 1 849 items >= 576).  Its hit-side
probes at 0 and 1e-9 penetrate by less than 4e-10 m, below the binary32 poses' own error: culled or not as the
rounding falls, a "free" where the oracle says contact, which the verdict comparison reports."""
import os

import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import specialise
from overlay_models import PLAIN_SUBDIR, overlay_models
from spec_models import spec_models
from test_threshold_cases_host import cases, generic_cases
from threshold_cases import STEP

pytestmark = pytest.mark.gpu

KEYS = ("MJPL_SPEC_DIR", "MJPL_SPEC", "MJPL_FUSED_SINGLE", "MJPL_FUSED_CERT")
TRIG = pytest.mark.parametrize("portable", [True, False], ids=["portable_trig", "libm"])


def _engine(m, allowed, qidx, base, options=None, **env):
    """An engine made (and its program compiled) under the given MJPL_* variables; the process is left without them."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        e = eng_mod.Engine(m, allowed, options=options)
        e.set_planning(qidx, base)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return e


def _configs(e, c, name, band=False):
    """check_configs in both layouts against the oracle -> verdicts.  band: the band's two sides, too."""
    got = e.check_configs(c.Q)
    if band:
        _band(e, c, name)
    np.testing.assert_array_equal(got, c.valid, err_msg=_where(c, got, c.valid, name))
    soa = e.check_configs(np.ascontiguousarray(c.Q.T), layout=eng_mod.SOA)
    np.testing.assert_array_equal(soa, c.valid, err_msg=_where(c, soa, c.valid, name + " (SOA)"))
    return got


def _band(e, c, name):
    """After a configuration launch.  last_undecided() counts ITEMS handed to the float64 kernels: whole configurations
    plus geom pairs, and an arm near one threshold often has several pairs inside the band (2 302 items from 1 920
    probes of the Franka with its fingers planned).  So besides the count, per probe, from the launch's own records
    (undecided_pairs: the configuration of every pair handed over): every "near" probe is among them, and at least
    one probe is not -- the filter still decides far ones by itself."""
    undecided = e.last_undecided()
    total, probe, _, _, _ = e.undecided_pairs()
    assert len(probe) == total <= undecided, (name, total, undecided)   # (the record is complete)
    whole = undecided - total                                         # configurations handed over whole: not recorded
    handed = np.unique(probe)
    print(f"{name}: {undecided} items undecided ({whole} whole configurations) of {len(handed) + whole} probes at most, "
          f"{int(c.near.sum())} near, {len(c.Q)} probes")
    assert undecided >= c.near.sum(), (name, undecided, int(c.near.sum()))
    missing = np.setdiff1d(np.flatnonzero(c.near), handed)
    assert len(missing) <= whole, _where(c, np.isin(np.arange(len(c.Q)), missing), np.zeros(len(c.Q), bool),
                                         name + ": near probes the filter decided by itself")
    assert len(handed) + whole < len(c.Q), (name, len(handed), whole, len(c.Q))


def _edges(e, c, name, shapes=("ending", "through")):
    out = []
    for shape in shapes:
        ed = getattr(c, shape)
        got, fb = e.check_edges(ed.qa, ed.qb, STEP, first_bad=True)
        np.testing.assert_array_equal(got, ed.valid, err_msg=_where(c, got, ed.valid, f"{name}, edges {shape}"))
        np.testing.assert_array_equal(fb, ed.first_bad, err_msg=_where(c, fb, ed.first_bad, f"{name}, first bad of edges {shape}"))
        out += [got, fb]
    return out


def _where(c, got, want, name):
    """For the failure message: model, and per differing probe its offset, side and the flipping pair's types."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))[:8]
    rows = [(int(i), float(c.off[i]), "hit" if c.hit_side[i] else "free", c.pairs[c.row[i]].tolist(), c.types[c.row[i]].tolist())
            for i in bad if i < len(c.off)]
    return f"{name}: (probe, offset, side, flipping geoms, their types) {rows}"


def _no_contact_that_counts(e, Q):
    """True where contacts(Q) has no bit of a pair that the allowed body pairs do not excuse."""
    _, excused = e.contact_pairs()
    counts = np.zeros(e.contact_words(), np.uint64)
    for p in np.flatnonzero(~excused):
        counts[p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return ~((e.contacts(Q) & counts) != 0).any(axis=1)


def _attack(entry, c, expect_kind):
    name, m, allowed, qidx, base = entry
    lib = _engine(m, allowed, qidx, base)
    interp = _engine(m, allowed, qidx, base, MJPL_SPEC=0)
    try:
        assert lib.spec_loaded() and lib.spec_kind() == expect_kind, f"{name}: no library of kind {expect_kind} (run __graft_entry__.build())"
        assert interp.spec_kind() == 0
        assert lib.info()["filter_enabled"] and abs(lib.info()["filter_tol"] - 1e-4) < 1e-9
        # every probe within 2e-5 m of its threshold lies inside the band; the filter still decides far ones by itself
        outs = [_configs(lib, c, name, band=True)] + _edges(lib, c, name)
        outs_i = [_configs(interp, c, name + " (interpreter)", band=True)] + _edges(interp, c, name + " (interpreter)")
        for x, y in zip(outs, outs_i):
            np.testing.assert_array_equal(x, y, err_msg=name)
        for e in (lib, interp):
            np.testing.assert_array_equal(_no_contact_that_counts(e, c.Q), c.valid.astype(bool), err_msg=name)
    finally:
        lib.close()
        interp.close()


@TRIG
@pytest.mark.parametrize("which", range(len(spec_models())))
def test_own_libraries_at_the_threshold(oracle_mod, which, portable):
    _attack(*cases("spec", which, portable), expect_kind=1)


@TRIG
@pytest.mark.parametrize("which", range(len(generic_cases())))
def test_scene_generic_libraries_at_the_threshold(oracle_mod, which, portable):
    _attack(*cases("generic", which, portable), expect_kind=2)


def _spec_index(entry):
    return [e[0] for e in spec_models()].index(entry[0])


def _counted(e, c):
    """Everything two builds of one text must agree on, bit for bit: verdicts and first-bad indices, the undecided count of
    the configuration launch, items and interior edges of every edge launch -- and the undecided count of the VALID
    edges of each shape, where every waypoint is looked at whatever order the waves take them in (behind an edge's first
    bad waypoint, how many more are looked at depends on that order: tests/test_gpu_overlay.py)."""
    out = [e.check_configs(c.Q), e.last_undecided()]
    for ed in (c.ending, c.through):
        v, fb = e.check_edges(ed.qa, ed.qb, STEP, first_bad=True)
        out += [v, fb, e.last_items(), e.last_interior_edges()]
        keep = ed.valid != 0
        vv = e.check_edges(np.ascontiguousarray(ed.qa[keep]), np.ascontiguousarray(ed.qb[keep]), STEP)
        out += [vv, e.last_undecided(), e.last_items(), e.last_interior_edges()]
    return out


@TRIG
@pytest.mark.parametrize("case", range(len(overlay_models())), ids=[c[0][0] for c in overlay_models()])
def test_builds_without_overlay_and_without_the_option_at_the_threshold(oracle_mod, case, portable):
    """spec/plain (no forced include of mjpl_overlay.h) and spec/structurized (no -structurizecfg-skip-uniform-regions)
    against the default build, in the single-round and the two-round launch shape."""
    entry, _, _ = overlay_models()[case]
    name, m, allowed, qidx, base = entry
    _, c = cases("spec", _spec_index(entry), portable)
    plain_dir = os.path.join(specialise.SPEC_DIR, PLAIN_SUBDIR)
    structurized_dir = os.path.join(specialise.SPEC_DIR, specialise.STRUCTURIZED_SUBDIR)
    lib_name = os.path.basename(specialise.spec_path(int(specialise.dump_program(m, allowed, qidx, base)[3].hash)))
    if not os.path.exists(os.path.join(plain_dir, lib_name)):
        pytest.skip("no build without the overlay under spec/plain (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(structurized_dir, lib_name)):
        pytest.skip("no build without the option under spec/structurized (run __graft_entry__.build())")
    try:
        for opts in ({}, {"MJPL_FUSED_SINGLE": 0}):
            engines = [_engine(m, allowed, qidx, base, **opts), _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=plain_dir, **opts),
                       _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=structurized_dir, **opts)]
            try:
                assert [e.spec_kind() for e in engines] == [1, 1, 1], name
                want = _counted(engines[0], c)
                np.testing.assert_array_equal(want[0], c.valid, err_msg=name)
                for e, tag in zip(engines[1:], ("plain", "structurized")):
                    for k, (x, y) in enumerate(zip(_counted(e, c), want)):
                        np.testing.assert_array_equal(x, y, err_msg=f"{name}, {tag}, {opts}, output {k}")
            finally:
                for e in engines:
                    e.close()
    finally:
        eng_mod.set_spec_dir(None)


@TRIG
def test_certificate_build_at_the_threshold(oracle_mod, portable):
    """spec/cert in the two-round launch shape: an endpoint tile widens every cull by what the pair can move along the edge
    and keeps certified edges out of the pool.  A certificate too generous by a micrometre certifies an edge whose
    waypoint sits on a probe just past the threshold: a wrong "valid"."""
    entry, c = cases("spec", 0, portable)
    name, m, allowed, qidx, base = entry
    assert name.startswith("franka_p+16obs, arm planned")   # the benchmark's model
    cert_dir = os.path.join(specialise.SPEC_DIR, "cert")
    key = int(specialise.dump_program(m, allowed, qidx, base)[3].hash)
    if not os.path.exists(os.path.join(cert_dir, os.path.basename(specialise.spec_path(key)))):
        pytest.skip("no certificate build of the benchmark model under spec/cert (python __graft_entry__.py makes it)")
    qa = np.concatenate([c.ending.qa, c.through.qa, c.filler.qa])
    qb = np.concatenate([c.ending.qb, c.through.qb, c.filler.qb])
    want = np.concatenate([c.ending.valid, c.through.valid, c.filler.valid])
    wfb = np.concatenate([c.ending.first_bad, c.through.first_bad, c.filler.first_bad])
    assert len(qa) < 6000
    try:
        on = _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=cert_dir, MJPL_FUSED_SINGLE=0)
        off = _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=cert_dir, MJPL_FUSED_SINGLE=0, MJPL_FUSED_CERT=0)
        try:
            assert on.spec_kind() == 1 and off.spec_kind() == 1 and on.info()["fused_edges"]
            got, gfb = on.check_edges(qa, qb, STEP, first_bad=True)
            certified = on.last_certified()
            print(f"{certified} of {int(want.sum())} valid edges certified ({len(qa)} edges)")
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(gfb, wfb)
            assert 0 < certified <= want.sum()   # the certificate code ran, and spared valid edges only
            got0, gfb0 = off.check_edges(qa, qb, STEP, first_bad=True)
            assert off.last_certified() == 0
            np.testing.assert_array_equal(got0, got)
            np.testing.assert_array_equal(gfb0, gfb)
            for e in (on, off):
                _configs(e, c, name + " (certificate build)")
        finally:
            on.close()
            off.close()
    finally:
        eng_mod.set_spec_dir(None)


@TRIG
def test_generated_float64_check_at_the_threshold(oracle_mod, portable):
    """spec/f64 with the filter off: the generated float64 check (struct ExactFull) decides every probe and waypoint by
    itself -- a literal folded one ulp off flips a probe at offset 0 -- and the interpreting pool kernel (f64_spec = 0)."""
    entry, c = cases("spec", 0, portable)
    name, m, allowed, qidx, base = entry
    f64_dir = os.path.join(specialise.SPEC_DIR, "f64")
    if not os.path.isdir(f64_dir) or not os.listdir(f64_dir):
        pytest.skip("no library with the generated float64 check (python -c 'import __graft_entry__ as g; g.build()')")
    res = []
    try:
        for tag, opts in (("generated", {}), ("interpreting", {"f64_spec": 0})):
            e = _engine(m, allowed, qidx, base, options=opts, MJPL_SPEC_DIR=f64_dir)
            try:
                e.set_filter(False)
                assert e.spec_kind() == 1 and not e.info()["filter_enabled"]
                res.append([_configs(e, c, f"{name} (float64, {tag})")] + _edges(e, c, f"{name} (float64, {tag})"))
            finally:
                e.close()
        for x, y in zip(*res):
            np.testing.assert_array_equal(x, y)
    finally:
        eng_mod.set_spec_dir(None)
