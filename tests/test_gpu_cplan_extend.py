"""mjpl_plan_paths_constrained_ext* (chained extensions, mjpl_amd/csrc/mjpl_cplan.h) against their NumPy statement
(tests/cplan_extend_reference.py), bit for bit with the engine's own checks and the handle's own projection as the
verdicts, on the scenes of tests/test_gpu_cplan.py.  Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import cplan_cases as cases
import cplan_extend_reference as xref
from mjpl_amd import engine
from test_gpu_cplan import BALL, DEFAULT_CHUNK_BYTES, FIELDS, FRANKA, ball, franka, franka_pose, same_bits  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def check_against_statement(s, what, **kw):
    """test_gpu_cplan.check_against_statement with the statement that knows `extend`."""
    calls = []
    ref_kw = dict(kw)
    step_dist = ref_kw.pop("step_dist")
    want = xref.plan_paths_constrained(s.QI, s.QG, s.lo, s.hi, *s.verdicts(step_dist, calls), **ref_kw)
    got = s.run(**kw)
    print(f"{what}: status counts {np.bincount(got['status'], minlength=6)}, rounds used {got['rounds_used'].tolist()}, "
          f"rows {got['n_out'].tolist()}, edges {got['edges'].sum()}, largest tree {got['tree_nodes'].max()}")
    same_bits(got, want, what)
    # one edge launch per round at most, in one chunk: the library validated exactly the statement's edges
    assert s.e.get_option("plan_last_edges") == sum(calls) == got["edges"].sum()
    assert s.e.get_option("plan_last_chunks") == 1
    return got, want


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
@pytest.mark.parametrize("extend", [2, 5, 32])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("rounds", [1, 32])
def test_bits_of_the_statement_ball(ball, rounds, K, extend, seed):
    kw = {**BALL, **dict(rounds=rounds, candidates=K, chain=8, seed=seed, extend=extend)}
    check_against_statement(ball, f"ball rounds={rounds} K={K} extend={extend}", **kw)


@pytest.mark.parametrize("extend", [2, 5])
@pytest.mark.parametrize("K", [1, 7])
def test_bits_of_the_statement_franka(franka, K, extend):
    got, _ = check_against_statement(franka, f"franka K={K} extend={extend}", rounds=4, candidates=K, chain=5, seed=3, extend=extend,
                                     **FRANKA)
    assert got["status"][5] == engine.PLAN_SOLVED and got["rounds_used"][5] == 1 and got["n_out"][5] == 2  # (q_goal == q_init)


def test_extend_one_is_the_old_entry_point(franka, ball):
    F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for s, params in ((franka, dict(rounds=4, candidates=7, chain=5, seed=3, **FRANKA)), (ball, dict(rounds=32, seed=0, **BALL))):
        lib, B, d = s.e.lib, len(s.QI), s.QI.shape[1]
        desc = engine.Engine.cplan_desc(**params)
        lo, hi = np.ascontiguousarray(s.lo, np.float64), np.ascontiguousarray(s.hi, np.float64)
        QI, QG = np.ascontiguousarray(s.QI), np.ascontiguousarray(s.QG)

        def call(fn, *extend):
            out = dict(P=np.full((B, desc.max_rows, d), 7.0), n_out=np.full(B, 7, np.int32), status=np.full(B, 7, np.int32),
                       rounds_used=np.full(B, 7, np.int32), edges=np.full(B, 7, np.int32), tree_nodes=np.full((B, 2), 7, np.int32))
            rc = fn(s.pose._proj.h, C.byref(desc), *extend, QI.ctypes.data_as(F64P), QG.ctypes.data_as(F64P), B, lo.ctypes.data_as(F64P),
                    hi.ctypes.data_as(F64P), out["P"].ctypes.data_as(F64P), *(out[f].ctypes.data_as(I32P) for f in FIELDS[1:]))
            assert rc == 0
            return out, int(s.e.get_option("plan_last_edges")), int(s.e.get_option("plan_last_rounds"))
        old, old_edges, old_rounds = call(lib.mjpl_plan_paths_constrained)
        new, new_edges, new_rounds = call(lib.mjpl_plan_paths_constrained_ext, 1)
        same_bits(new, old, "extend = 1")
        assert (new_edges, new_rounds) == (old_edges, old_rounds) and old_edges > 0
        assert (old["status"] == engine.PLAN_SOLVED).any()
        # ... and the Python surface's default is that call
        same_bits(s.run(**params), old, "the default")


def test_refused_extend(franka):
    e = franka.e
    desc = engine.Engine.cplan_desc(rounds=2, **FRANKA)
    for extend in (0, 33, -1):
        for fn in (e.lib.mjpl_plan_paths_constrained_ext, e.lib.mjpl_plan_paths_constrained_ext_dev):
            assert fn(franka.pose._proj.h, C.byref(desc), extend, None, None, 0, None, None, None, None, None, None, None, None) == -1
        with pytest.raises(ValueError):
            franka.run(rounds=2, extend=extend, **FRANKA)
    # B = 0 with a good `extend` launches nothing (the box is still looked at, as by the old entry point)
    F64P = C.POINTER(C.c_double)
    lo, hi = np.ascontiguousarray(franka.lo, np.float64), np.ascontiguousarray(franka.hi, np.float64)
    assert e.lib.mjpl_plan_paths_constrained_ext(franka.pose._proj.h, C.byref(desc), 32, None, None, 0, lo.ctypes.data_as(F64P),
                                                 hi.ctypes.data_as(F64P), None, None, None, None, None, None) == 0
    assert e.get_option("plan_last_chunks") == 0 and e.get_option("plan_last_edges") == 0


def test_full_trees(ball):
    got, want = check_against_statement(ball, "nodes=12 extend=32", rounds=32, seed=0, extend=32, **{**BALL, "nodes": 12})
    assert got["tree_nodes"].max() == 12  # the appending stops at `nodes`, in the middle of a chain
    assert all(len(t[0]) <= 12 and len(t[2]) <= 12 for t in want["trees"] if t is not None)


def test_long_paths_are_reported(ball):
    got, _ = check_against_statement(ball, "max_rows=16 extend=8", rounds=32, seed=0, max_rows=16, extend=8, **BALL)
    long_ones = np.flatnonzero(got["status"] == engine.PLAN_LONG)
    assert len(long_ones) >= 1
    assert not got["n_out"][long_ones].any() and not got["P"][long_ones].any() and got["P"].shape[1] == 16


def test_chunks_change_no_bit(franka):
    e = franka.e
    assert e.get_option("plan_chunk_bytes") == DEFAULT_CHUNK_BYTES
    kw = dict(rounds=4, candidates=7, chain=5, seed=7, extend=5, **FRANKA)
    one = franka.run(**kw)
    assert e.get_option("plan_last_chunks") == 1
    edges = e.get_option("plan_last_edges")
    try:
        for nbytes in (1, 300_000):
            e.set_option("plan_chunk_bytes", nbytes)
            got = franka.run(**kw)
            chunks = int(e.get_option("plan_last_chunks"))
            print(f"plan_chunk_bytes {nbytes}: {chunks} chunks")
            # (a problem's workspace grows with `extend`: 300 000 bytes hold a few problems, one byte holds one)
            assert 2 <= chunks <= 24 and (chunks == 24) == (nbytes == 1)
            same_bits(got, one, f"chunk bytes {nbytes}")
            assert e.get_option("plan_last_edges") == edges
    finally:
        e.set_option("plan_chunk_bytes", DEFAULT_CHUNK_BYTES)


def test_host_and_device_forms_agree(franka):
    e, QI, QG, lo, hi = franka.e, franka.QI, franka.QG, franka.lo, franka.hi
    kw = dict(rounds=4, candidates=7, chain=5, seed=3, extend=5, **FRANKA)
    host = franka.run(**kw)
    dkw = {k: v for k, v in kw.items() if k not in ("step_dist", "epsilon")}
    dQI, dQG = e.alloc(QI.nbytes).upload(QI), e.alloc(QG.nbytes).upload(QG)
    bufs = {f: e.alloc(max(host[f].nbytes, 8)) for f in FIELDS}
    e.plan_paths_constrained_dev(franka.pose, dQI.ptr, dQG.ptr, len(QI), lo, hi, kw["step_dist"], kw["epsilon"], bufs["P"].ptr,
                                 bufs["n_out"].ptr, bufs["status"].ptr, bufs["rounds_used"].ptr, bufs["edges"].ptr,
                                 bufs["tree_nodes"].ptr, **dkw)
    got = {f: bufs[f].download(host[f].dtype, host[f].size).reshape(host[f].shape) for f in FIELDS}
    same_bits(got, host, "device form")
    for buf in (dQI, dQG, *bufs.values()):
        buf.free()


def test_generated_chain_and_interpreting_kernels_agree(franka):
    if not franka.pose._proj.spec_loaded():
        pytest.skip("the engine's library has no generated projection for this chain")
    e = franka.e
    kw = dict(rounds=4, candidates=7, chain=5, seed=5, extend=5, **FRANKA)
    generated = franka.run(**kw)
    e.set_option("pose_spec", 0)
    try:
        plain = franka_pose(e, e.model, franka.base)
        assert not plain._proj.spec_loaded()
        same_bits(franka.run(pose=plain, **kw), generated, "interpreting handle")
    finally:
        e.set_option("pose_spec", 1)


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
def test_statuses_and_invariants_on_the_ball(ball, seed):
    kw = dict(rounds=32, seed=seed, extend=8, **BALL)
    got = ball.run(**kw)
    print("status", got["status"], "rounds", got["rounds_used"], "rows", got["n_out"], "nodes", got["tree_nodes"].tolist())
    assert tuple(got["status"]) == cases.BALL_STATUS
    # `forward` is the statement's: its outputs are the library's, bit for bit
    ref_kw = {k: v for k, v in kw.items() if k != "step_dist"}
    want = xref.plan_paths_constrained(ball.QI, ball.QG, ball.lo, ball.hi, *ball.verdicts(kw["step_dist"]), **ref_kw)
    same_bits(got, want, "extend=8")
    _, edges, _, pose_valid = ball.verdicts(kw["step_dist"])
    cases.check_invariants(ball.QI, ball.QG, {**got, "forward": want["forward"]}, edges, pose_valid, kw["epsilon"], cases.BALL_QSTEP, 256)
