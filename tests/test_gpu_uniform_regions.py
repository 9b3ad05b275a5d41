"""build.codegen_flags(): the code generation option on the compiler's line of libmjpl_hip.so and of every per-model
library (-structurizecfg-skip-uniform-regions: wave-uniform branches stay scalar branches).  It changes how control flow
is laid out, never a value, so a library built WITH it must return, bit for bit, what the same text built WITHOUT it
returns (spec/structurized/, compiled by __graft_entry__.build(), overlay and all else as shipped): verdicts, first-bad
indices, the item and interior-edge counts and -- on a batch of valid edges, where every waypoint is looked at whatever
order the waves take them in -- the number of pairs handed to the exact re-check.  The interpreting kernels of the main
library (built with the option too) must agree on verdicts and indices.  Shapes and recipes are those of
tests/test_gpu_overlay.py (restated here): endpoint and item tiles of a two-round launch with a ragged tile, the
single-round mode, two rounds with a pool that is reused; one model per slot-file kind; and check_configs."""
import ctypes
import json
import os

import numpy as np
import pytest

from mjpl_amd import build as build_mod
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes, specialise
from overlay_models import overlay_models

gpu = pytest.mark.gpu

STEP = 0.01
STRUCTURIZED_DIR = os.path.join(specialise.SPEC_DIR, specialise.STRUCTURIZED_SUBDIR)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generated_source_digests.json")
KEYS = ("MJPL_SPEC_DIR", "MJPL_SPEC", "MJPL_FUSED_SINGLE", "MJPL_FUSED_POOL")
OPTION = "-structurizecfg-skip-uniform-regions"

BENCH_SHAPES = ((64 * 12 + 1, {"MJPL_FUSED_SINGLE": 0}), (1024, {}), (40000, {"MJPL_FUSED_POOL": 832}))
MODEL_SHAPES = ((64 * 12 + 1, {"MJPL_FUSED_SINGLE": 0}), (1024, {}))


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


def _folded_edges(m, qidx, n, seed=2):
    """bench.py's make_edges (its seed, its edge length) with the elbow kept in the folded quarter of its range: stored
    partners are pushed in most configurations and about half of the edges end in a self-contact or at an obstacle."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[qidx, 0].copy(), m.jnt_range[qidx, 1].copy()
    hi[3] = lo[3] + 0.25 * (hi[3] - lo[3])
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return qa, np.clip(qa + 0.05 * d, lo, hi)


def _random_edges(m, qidx, n, seed):
    """tests/test_gpu_spec.py's recipe: a third of the edges six times as long, every 97th of length zero."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[qidx, 0], m.jnt_range[qidx, 1]
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    qb = np.clip(qa + rng.choice([0.05, 0.05, 0.3], size=(n, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True), lo, hi)
    qb[::97] = qa[::97]
    return qa, qb


def _launch(e, qa, qb):
    valid, fb = e.check_edges(qa, qb, STEP, first_bad=True)
    return valid, fb, e.last_items(), e.last_interior_edges()


def _compare(with_option, structurized, qa, qb, tag, others=()):
    """Both builds on the batch, then on its valid edges alone; `others`: engines that must agree on verdicts and indices."""
    v, fb, items, interior = _launch(with_option, qa, qb)
    pv, pfb, pitems, pinterior = _launch(structurized, qa, qb)
    np.testing.assert_array_equal(v, pv, err_msg=tag)
    np.testing.assert_array_equal(fb, pfb, err_msg=tag)
    assert (items, interior) == (pitems, pinterior), tag
    for o in others:
        ov, ofb = o.check_edges(qa, qb, STEP, first_bad=True)
        np.testing.assert_array_equal(v, ov, err_msg=tag)
        np.testing.assert_array_equal(fb, ofb, err_msg=tag)
    keep = v != 0
    assert keep.any(), tag
    va, vb = np.ascontiguousarray(qa[keep]), np.ascontiguousarray(qb[keep])
    counts = []
    for e in (with_option, structurized):
        vv, vfb, vitems, vinterior = _launch(e, va, vb)
        assert vv.all(), tag
        counts.append((e.last_undecided(), vitems, vinterior))
    assert counts[0] == counts[1], (tag, counts)
    return v, fb, items


def _bench_model():
    m = scenes.franka_p(obstacles=True)
    return m, scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()


def _three(m, allowed, qidx, base, opts):
    """(the shipped build, the build without the option, the interpreting kernels of the main library)"""
    return (_engine(m, allowed, qidx, base, **opts),
            _engine(m, allowed, qidx, base, MJPL_SPEC_DIR=STRUCTURIZED_DIR, **opts),
            _engine(m, allowed, qidx, base, MJPL_SPEC=0, **opts))


@gpu
@pytest.mark.parametrize("n,opts", BENCH_SHAPES, ids=[str(s[0]) for s in BENCH_SHAPES])
def test_benchmark_model_with_and_without_the_option(n, opts):
    m, qidx, base = _bench_model()
    qa, qb = _folded_edges(m, qidx, n)
    with_option, structurized, interp = engines = _three(m, (), qidx, base, opts)
    try:
        assert with_option.spec_kind() == 1, "no library of the benchmark model (run __graft_entry__.build())"
        assert structurized.spec_kind() == 1, "no build without the option under spec/structurized (run __graft_entry__.build())"
        assert interp.spec_kind() == 0
        assert with_option.info()["fused_edges"] and structurized.info()["fused_edges"]
        v, fb, items = _compare(with_option, structurized, qa, qb, f"benchmark model, {n} edges", others=(interp,))
        assert items > 0
        assert ((v == 0) & (fb > 0)).any(), "no edge whose first bad check is a waypoint: the item tiles decided nothing"
        assert 0.2 < v.mean() < 0.8
    finally:
        for e in engines:
            e.close()
        eng_mod.set_spec_dir(None)


@gpu
@pytest.mark.parametrize("case", range(1, len(overlay_models())), ids=[c[0][0] for c in overlay_models()[1:]])
def test_other_models_with_and_without_the_option(case):
    """Random trees four and sixteen slots wide and the model with moving boxes (literal slots: SpecSlots)."""
    (name, m, allowed, qidx, base), width, mbox = overlay_models()[case]
    info = specialise.dump_program(m, allowed, qidx, base)[3]
    assert (int(info.maxs), bool(info.mbox)) == (width, mbox), name
    try:
        for n, opts in MODEL_SHAPES:
            qa, qb = _random_edges(m, qidx, n, 300 + case)
            with_option, structurized, interp = engines = _three(m, allowed, qidx, base, opts)
            try:
                assert with_option.spec_kind() == 1 and structurized.spec_kind() == 1 and interp.spec_kind() == 0, name
                v, fb, items = _compare(with_option, structurized, qa, qb, f"{name}, {n} edges", others=(interp,))
                assert items > 0 and 0.02 < v.mean() < 0.98, name
            finally:
                for e in engines:
                    e.close()
    finally:
        eng_mod.set_spec_dir(None)


@gpu
def test_configurations_with_and_without_the_option():
    """check_configs (k_filter_configs of the per-model library, the exact kernels of the main one) on 4 096 configurations
    of the benchmark model, half of them with the folded elbow: equal verdicts from both builds and from the interpreter."""
    m, qidx, base = _bench_model()
    Q = np.concatenate([_folded_edges(m, qidx, 2048)[0], _random_edges(m, qidx, 2048, 7)[0]])
    engines = _three(m, (), qidx, base, {})
    try:
        assert [e.spec_kind() for e in engines] == [1, 1, 0]
        v, pv, iv = (e.check_configs(Q) for e in engines)
        np.testing.assert_array_equal(v, pv)
        np.testing.assert_array_equal(v, iv)
        assert 0.1 < v.mean() < 0.9
    finally:
        for e in engines:
            e.close()
        eng_mod.set_spec_dir(None)


def test_the_option_rides_on_both_compile_lines_and_nowhere_else(monkeypatch):
    """Host only.  The option is in codegen_flags(), which build_hip and specialise._compile put on their lines (and
    _compile leaves off on request), and in neither hipcc_flags() -- the stamp's line -- nor overlay_flags(); the
    benchmark program's hash is the recorded one and both builds of its library carry the stamp of build.src_stamp()."""
    assert OPTION in build_mod.codegen_flags() and OPTION not in build_mod.codegen_flags(uniform_regions=False)
    assert OPTION not in build_mod.hipcc_flags() and OPTION not in build_mod.overlay_flags()
    assert not any("structurize" in f for f in (*build_mod.hipcc_flags(), *build_mod.overlay_flags()))
    lines = []

    class Done(Exception):
        pass

    def record(cmd, **kw):
        lines.append(list(cmd))
        raise Done

    monkeypatch.setattr(build_mod.subprocess, "run", record)
    monkeypatch.setattr(specialise.subprocess, "run", record)
    with pytest.raises(Done):
        build_mod.build_hip(force=True)
    scratch = os.path.join(specialise.SPEC_DIR, "uniform_regions_test")
    for on in (True, False):
        with pytest.raises(Done):
            specialise._compile("", scratch + ".hip", scratch + ".so", False, (), uniform_regions=on)
    assert not [f for f in os.listdir(specialise.SPEC_DIR) if f.startswith("uniform_regions_test")]
    hip, spec_on, spec_off = lines
    for line in (hip, spec_on):
        assert line[line.index(OPTION) - 1] == "-mllvm"
    assert OPTION not in spec_off
    assert [f for f in spec_on if f not in spec_off] == ["-mllvm", OPTION]

    with open(GOLDEN) as f:
        golden = json.load(f)
    m, qidx, base = _bench_model()
    info = specialise.dump_program(m, (), qidx, base)[3]
    want = next(v["hash"] for k, v in golden["models"].items() if k.startswith("franka_p+16obs, arm planned"))
    assert f"{int(info.hash):016x}" == want
    stamp = build_mod.src_stamp()
    name = os.path.basename(specialise.spec_path(int(info.hash)))
    for path in (specialise.spec_path(int(info.hash)), os.path.join(STRUCTURIZED_DIR, name)):
        assert os.path.exists(path), f"{path}: run __graft_entry__.build()"
        lib = ctypes.CDLL(path)
        lib.mjpl_spec_src_stamp.restype = ctypes.c_ulonglong
        lib.mjpl_spec_hash.restype = ctypes.c_ulonglong
        assert int(lib.mjpl_spec_src_stamp()) == stamp, path
        assert int(lib.mjpl_spec_hash()) == int(info.hash), path
