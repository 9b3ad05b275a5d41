"""mjpl_shortcut_paths* (mjpl_amd/csrc/mjpl_shortcut.h) against their NumPy statement (tests/shortcut_reference.py), bit
for bit with the engine's own edge check as the verdict, and smooth_paths on top of them.  Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import shortcut_cases as cases
import shortcut_reference as ref
from mjpl_amd import CollisionConstraint, HipToppTrajectoryGenerator, engine, scenes, smooth_paths

pytestmark = pytest.mark.gpu

STEP = 0.02
DEFAULT_CHUNK_BYTES = 256 << 20
FIELDS = ("keep", "n_out", "length", "status", "proposed", "accepted")
E_ARG, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def franka():
    """(engine on the headline scene's planning columns, W, wp_off) of 37 seeded random walks of valid configurations."""
    model, qidx, base = cases.franka_planning()
    e = engine.Engine(model, device=0)
    e.set_planning(qidx, base)
    lo, hi = model.jnt_range[qidx, 0], model.jnt_range[qidx, 1]
    paths = cases.random_walks(lo, hi, lambda Q: e.check_configs(Q).astype(bool), cases.path_lengths(37), seed=11)
    W, off = cases.pack(paths)
    yield e, W, off
    e.close()


@pytest.fixture(scope="module")
def ball():
    c = CollisionConstraint(scenes.two_dof_ball())
    yield c
    c.engine.close()


def run(e, W, off, **kw):
    return dict(zip(FIELDS, e.shortcut_paths(W, off, STEP, **kw)))


def same_bits(got, want, what=""):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        a, b = got[f].view(np.uint64 if f == "length" else got[f].dtype), want[f].view(np.uint64 if f == "length" else want[f].dtype)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{what} {f}: {len(bad)} entries differ, first at {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}"


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("rounds", [1, 5])
@pytest.mark.parametrize("K", [1, 7, 64])
def test_bits_of_the_statement(franka, K, rounds, seed):
    e, W, off = franka
    calls = []

    def verdict(QA, QB):
        calls.append(len(QA))
        return e.check_edges(QA, QB, STEP).astype(bool)
    want = ref.shortcut_paths(W, off, verdict, rounds=rounds, candidates=K, seed=seed)
    got = run(e, W, off, rounds=rounds, candidates=K, seed=seed)
    print(f"K {K} rounds {rounds}: proposed {got['proposed'].sum()}, accepted {got['accepted'].sum()}, rows {got['n_out'].sum()} of {len(W)}, "
          f"status counts {np.bincount(got['status'], minlength=3)}")
    same_bits(got, want, f"K={K} rounds={rounds}")
    assert got["accepted"].sum() > 0 and (got["proposed"] >= got["accepted"]).all()
    if K == 64:  # (64 proposals on at most 130 waypoints overlap: some lose to a better one, whatever the verdicts)
        assert got["proposed"].sum() > got["accepted"].sum()
    # one edge launch per round that proposed anything: the library validated exactly the statement's edges
    assert e.get_option("shortcut_last_edges") == sum(calls) == got["proposed"].sum()
    assert e.get_option("shortcut_last_rounds") == len(calls) <= rounds and e.get_option("shortcut_last_chunks") == 1


def test_min_saving_bits(franka):
    e, W, off = franka
    want = ref.shortcut_paths(W, off, lambda a, b: e.check_edges(a, b, STEP).astype(bool), rounds=3, candidates=64, seed=4, min_saving=0.25)
    same_bits(run(e, W, off, rounds=3, candidates=64, seed=4, min_saving=0.25), want, "min_saving")


def test_two_dof_ball_and_wall(ball):
    paths = cases.ball_paths()
    W, off = cases.pack(paths)
    out, info = smooth_paths([list(p) for p in paths], ball, STEP, return_info=True)
    assert [i["status"] for i in info] == ["converged", "converged"]
    # a detour around nothing collapses to its two ends
    assert len(out[0]) == 2 and out[0][0] is not None and np.array_equal(out[0][0], paths[0][0]) and np.array_equal(out[0][1], paths[0][-1])
    assert info[0]["length"] == ref.dist(W, [0], [off[1] - 1])[0]
    # a path round the box keeps an interior waypoint, and every segment of it is valid
    over = np.stack(out[1])
    assert len(over) > 2 and np.array_equal(over[0], paths[1][0]) and np.array_equal(over[-1], paths[1][-1])
    assert ball.valid_edges_planning(over[:-1], over[1:], STEP).all()
    straight = float(np.linalg.norm(paths[1][-1] - paths[1][0]))
    before = ref.arc_lengths(W, np.arange(off[1], off[2]))[-1]
    print(f"over the wall: {len(paths[1])} -> {len(over)} waypoints, length {before:.4f} -> {info[1]['length']:.4f} (straight {straight:.4f})")
    assert straight < info[1]["length"] < before
    assert info[1]["proposed"] > info[1]["accepted"] > 0
    # ... and it is the statement's result
    want = ref.shortcut_paths(W, off, lambda a, b: ball.valid_edges_planning(a, b, STEP), rounds=16, candidates=64, seed=0)
    same_bits(dict(zip(FIELDS, ball.engine.shortcut_paths(W, off, STEP))), want, "ball")


def test_chunks_change_no_bit(franka):
    e, W, off = franka
    assert e.get_option("shortcut_chunk_bytes") == DEFAULT_CHUNK_BYTES
    one = run(e, W, off, rounds=5, candidates=64, seed=7)
    assert e.get_option("shortcut_last_chunks") == 1
    try:
        for nbytes, least in ((1, 37), (60_000, 3)):
            e.set_option("shortcut_chunk_bytes", nbytes)
            got = run(e, W, off, rounds=5, candidates=64, seed=7)
            chunks = int(e.get_option("shortcut_last_chunks"))
            print(f"shortcut_chunk_bytes {nbytes}: {chunks} chunks")
            assert least <= chunks <= 37 and (chunks == 37) == (nbytes == 1)
            same_bits(got, one, f"chunk bytes {nbytes}")
        with pytest.raises(engine.MjplError):
            e.set_option("shortcut_last_chunks", 1)
    finally:
        e.set_option("shortcut_chunk_bytes", DEFAULT_CHUNK_BYTES)


def test_nan_path_is_left_alone(franka):
    e, W, off = franka
    clean = run(e, W, off, rounds=5, candidates=64, seed=1)
    bad = W.copy()
    b = 17  # (a path in the middle of the batch)
    bad[off[b] + 3, 2] = np.nan
    got = run(e, bad, off, rounds=5, candidates=64, seed=1)
    assert got["status"][b] == engine.SHORTCUT_NONFINITE and got["keep"][off[b]:off[b + 1]].all()
    assert got["n_out"][b] == off[b + 1] - off[b] and np.isnan(got["length"][b]) and got["proposed"][b] == 0 == got["accepted"][b]
    others = np.arange(len(off) - 1) != b
    rows = np.ones(len(W), bool)
    rows[off[b]:off[b + 1]] = False
    assert np.array_equal(got["keep"][rows], clean["keep"][rows])
    for f in FIELDS[1:]:
        assert np.array_equal(got[f][others].view(np.uint8), clean[f][others].view(np.uint8)), f
    inf = W.copy()
    inf[off[3], 0] = np.inf
    assert run(e, inf, off, rounds=1)["status"][3] == engine.SHORTCUT_NONFINITE


def test_refused_arguments(franka, ball):
    e, W, off = franka
    lib, F64P, I64P, I32P, U8P = e.lib, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    keep, n_out, status = np.zeros(len(W), np.uint8), np.zeros(len(off) - 1, np.int32), np.zeros(len(off) - 1, np.int32)

    def call(desc=None, W=W, off=off, B=None, keep=keep, n_out=n_out, status=status):
        desc = engine.ShortcutDesc(STEP, 0.0, 0, 2, 8) if desc is None else desc
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        return lib.mjpl_shortcut_paths(e.h, C.byref(desc), p(W, F64P), p(off, I64P), (0 if off is None else len(off) - 1) if B is None else B, p(keep, U8P),
                                       p(n_out, I32P), None, p(status, I32P), None, None)
    assert call() == 0  # (length, proposed, accepted: NULL is allowed)
    assert call(W=None) == E_ARG and call(off=None, B=37) == E_ARG and call(keep=None) == E_ARG and call(n_out=None) == E_ARG
    assert call(status=None) == E_ARG
    assert lib.mjpl_shortcut_paths(e.h, None, None, None, 0, None, None, None, None, None, None) == E_ARG
    for bad in (engine.ShortcutDesc(0.0, 0.0, 0, 2, 8), engine.ShortcutDesc(float("nan"), 0.0, 0, 2, 8), engine.ShortcutDesc(STEP, 0.0, 0, 0, 8),
                engine.ShortcutDesc(STEP, 0.0, 0, 2, 0), engine.ShortcutDesc(STEP, 0.0, 0, 2, 65), engine.ShortcutDesc(STEP, -1e-9, 0, 2, 8),
                engine.ShortcutDesc(STEP, float("nan"), 0, 2, 8)):
        assert call(desc=bad) == E_ARG
        assert lib.mjpl_shortcut_paths_dev(e.h, C.byref(bad), None, None, 0, None, None, None, None, None, None) == E_ARG
    assert call(off=np.array([0, 5, 6], np.int64)) == E_ARG    # a path of one row
    assert call(off=np.array([0, 5, 3], np.int64)) == E_ARG    # offsets that fall
    assert call(off=np.array([1, 5], np.int64)) == E_ARG
    assert call(B=-1) == E_ARG
    assert call(off=np.array([0, 65537], np.int64)) == E_CAPACITY  # (refused before a row is read)
    assert b"65536" in lib.mjpl_last_error()
    # B = 0 launches nothing
    assert lib.mjpl_shortcut_paths(e.h, C.byref(engine.ShortcutDesc(STEP, 0.0, 0, 2, 8)), None, None, 0, None, None, None, None, None, None) == 0
    assert e.get_option("shortcut_last_chunks") == 0
    empty = e.shortcut_paths(np.zeros((0, W.shape[1])), [0], STEP)
    assert all(len(a) == 0 for a in empty)
    # the Python surface
    two = [np.zeros(2), np.ones(2)]
    assert smooth_paths([], ball, STEP) == []
    for paths, kw in (([[]], {}), ([[np.zeros(2)]], {}), ([two, []], {}), ([[np.zeros(3), np.ones(3)]], {}), ([two], dict(rounds=0)),
                      ([two], dict(candidates=65)), ([two], dict(min_saving=-1.0))):
        with pytest.raises(ValueError):
            smooth_paths(paths, ball, STEP, **kw)
    with pytest.raises(ValueError):
        smooth_paths([two], ball, 0.0)
    with pytest.raises(ValueError):
        e.shortcut_paths(W[:, :3], off, STEP)
    with pytest.raises(ValueError):
        e.shortcut_paths(W[:-1], off, STEP)


def test_host_and_device_forms_agree(franka):
    e, W, off = franka
    B = len(off) - 1
    host = run(e, W, off, rounds=4, candidates=7, seed=3)
    dW = e.alloc(W.nbytes).upload(W)
    bufs = {f: e.alloc(max(host[f].nbytes, 8)) for f in FIELDS}
    e.shortcut_paths_dev(dW.ptr, off, STEP, bufs["keep"].ptr, bufs["n_out"].ptr, bufs["length"].ptr, bufs["status"].ptr, bufs["proposed"].ptr,
                         bufs["accepted"].ptr, rounds=4, candidates=7, seed=3)
    got = {f: bufs[f].download(host[f].dtype, len(host[f])) for f in FIELDS}
    same_bits(got, host, "device form")
    # without the optional outputs
    for f in ("keep", "n_out", "status"):
        bufs[f].upload(np.zeros_like(host[f]))
    e.shortcut_paths_dev(dW.ptr, off, STEP, bufs["keep"].ptr, bufs["n_out"].ptr, None, bufs["status"].ptr, rounds=4, candidates=7, seed=3)
    for f in ("keep", "n_out", "status"):
        assert np.array_equal(bufs[f].download(host[f].dtype, len(host[f])), host[f]), f
    assert B == len(got["status"])
    for buf in (dW, *bufs.values()):
        buf.free()


def test_smooth_paths_feeds_the_trajectory_generator():
    model = scenes.franka_p(obstacles=True)
    c = CollisionConstraint(model)
    try:
        lo, hi = model.jnt_range[:, 0], model.jnt_range[:, 1]
        home = model.keyframe("home").qpos.copy()
        lo, hi = np.where(np.arange(model.nq) < 7, lo, home), np.where(np.arange(model.nq) < 7, hi, home)  # (the fingers stay put)
        walks = cases.random_walks(lo, hi, c.valid_configs, [2, 9, 40, 70], seed=5)
        paths = [list(w) for w in walks]
        out, info = smooth_paths(paths, c, STEP, rounds=8, seed=1, return_info=True)
        assert len(out) == len(paths)
        for path, short, i in zip(paths, out, info):
            assert 2 <= len(short) <= len(path) and short[0] is path[0] and short[-1] is path[-1]
            ids = [id(q) for q in path]
            at = [ids.index(id(q)) for q in short]  # the original arrays, in order
            assert at == sorted(at) and all(q.shape == (model.nq,) for q in short)
            Q = np.stack(short)
            new = np.flatnonzero(np.diff(at) > 1)  # (a walk's own segments were never checked: only its waypoints are valid)
            assert len(new) == 0 or c.engine.check_edges(Q[new], Q[new + 1], STEP).all()
            assert i["status"] in ("converged", "rounds") and i["length"] <= ref.arc_lengths(np.stack(path), np.arange(len(path)))[-1] * (1 + 1e-12)
        assert sum(i["accepted"] for i in info) > 0
        assert smooth_paths(paths, c, STEP, rounds=8, seed=1)[1][-1] is out[1][-1]
        gen = HipToppTrajectoryGenerator(0.01, np.full(model.nq, 2.0), np.full(model.nq, 4.0), engine=c.engine)
        trajs = gen.generate_trajectories(out)
        assert len(trajs) == len(out) and all(t is not None for t in trajs)
        for t, short in zip(trajs, out):
            assert np.allclose(t.positions[-1], short[-1], atol=1e-9)
    finally:
        c.engine.close()
