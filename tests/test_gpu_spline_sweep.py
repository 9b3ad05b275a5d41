"""Certified trajectories on the GPU (include/mjpl_hip.h: mjpl_sweep_splines*): closed forms on the wall scene of
test_gpu_sweep.py, the loop against the NumPy statement (tests/spline_sweep_reference.py) fed by Engine.sweep_measure,
soundness of FREE and HIT against Engine.clearance on the same batches, the reductions to sweep_edges and topp_profile,
batch sizes and forms, bad inputs and argument errors, the constraints and generate_certified_trajectory.

The closed-form path [0, 0.86, 0.86, 0] of the ball (r 0.01) and the wall 0.899 .. 0.901: its three straight segments
stay 0.029 clear, its spline peaks at 0.989 in the middle piece -- through the wall and back."""
import ctypes as C
import functools

import numpy as np
import pytest

import spline_sweep_reference as ssr
import sweep_reference as sref
import trajectory_reference as tref
from mjpl_amd import engine as eng_mod
from mjpl_amd.constraint import ClearanceConstraint, CollisionConstraint
from mjpl_amd.trajectory import HipToppTrajectoryGenerator, generate_certified_trajectory
from test_gpu_sweep import cap_of, gpu_models, wall_scene
from test_spline_sweep_host import WALL_PATH

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
FREE, HIT, UNDECIDED, NONFINITE, RANGE = (eng_mod.SWEEP_FREE, eng_mod.SWEEP_HIT, eng_mod.SWEEP_UNDECIDED,
                                          eng_mod.SWEEP_NONFINITE, eng_mod.SWEEP_RANGE)
NAMES = ("status", "t_hit", "clear_lb", "pair", "nodes", "depth")
DECISION = 1e-6  # pieces whose decision margins stay above this at every node are compared
PATHS, MAX_DEPTH, SEED = 48, 6, 5
WALL = dict(cap=0.1, lo=[-2.0], hi=[2.0])


def point(W, M, k, t):
    return W[k] if t == 0.0 else W[k + 1] if t == 1.0 else tref.spline_eval(W, M, k, t)[0]


# ---- closed forms
def test_the_spline_goes_through_the_wall_its_segments_avoid():
    e = eng_mod.Engine(wall_scene())
    off = [0, 4]
    assert list(e.sweep_edges(WALL_PATH[:-1], WALL_PATH[1:], **WALL)[0]) == [FREE, FREE, FREE]
    st, t, lb, pair, nodes, depth, M = e.sweep_splines(WALL_PATH, off, **WALL)
    assert list(st) == [FREE, HIT, FREE]
    assert t[1] == 0.0625 and depth[1] == 3 and pair[1] == 0 and np.isnan(lb[1])
    assert np.all(lb[[0, 2]] > 0) and np.isnan(t[[0, 2]]).all() and np.all(pair[[0, 2]] == -1)
    assert e.clearance(point(WALL_PATH, M, 1, t[1])[None, :], 0.1)[0][0] <= 0
    # the same path under hi = 0.95: the spline leaves the bounds before it reaches the wall's far side
    st, t, lb, pair, nodes, depth, M = e.sweep_splines(WALL_PATH, off, cap=0.1, lo=[-2.0], hi=[0.95])
    assert list(st) == [FREE, RANGE, FREE] and pair[1] == -2 and np.isfinite(t[1]) and np.isnan(lb[1])
    assert point(WALL_PATH, M, 1, t[1])[0] > 0.95
    # [0, 0.8, 0.8, 0] peaks at 0.92
    W = np.array([[0.0], [0.8], [0.8], [0.0]])
    assert list(e.sweep_splines(W, off, **WALL)[0]) == [FREE, HIT, FREE]


def test_certified_trajectory_after_one_insertion():
    """The case the issue sets: [0, 0.8, 0.8, 0] is HIT in its middle piece; one midpoint gives [0, 0.8, 0.8, 0.8, 0],
    whose spline peaks at 0.8508 (NumPy statement: FREE, clear_lb 0.0234; the TOPP statement parameterises both paths
    with status OK).  Both the path and its refinement hold two equal consecutive waypoints, which the generator
    refuses unless it is made with allow_repeated_waypoints (the default refusal stays: tests/test_gpu_trajectory.py)."""
    cc = CollisionConstraint(wall_scene())
    wps = [np.array([0.0]), np.array([0.8]), np.array([0.8]), np.array([0.0])]
    with pytest.raises(ValueError):
        generate_certified_trajectory(wps, HipToppTrajectoryGenerator(0.01, [1.0], [2.0], engine=cc.engine), [], cc, **WALL)
    gen = HipToppTrajectoryGenerator(0.01, [1.0], [2.0], engine=cc.engine, allow_repeated_waypoints=True)
    traj, cert = generate_certified_trajectory(wps, gen, [], cc, **WALL)
    assert len(cert.piece_status) == 4 and len(wps) == 4  # exactly one insertion
    peak = max(float(q[0]) for q in traj.positions)
    print(f"clear_lb {cert.clear_lb}, largest sampled x {peak}")
    assert cert.status == FREE and 0 < cert.clear_lb <= 0.889 - 0.8508 + 1e-6
    assert abs(peak - 0.8508) <= 1e-4 and abs(float(traj.positions[-1][0])) <= 1e-12


def test_certified_trajectory_without_equal_waypoints():
    # [0, 0.8, 0.81, 0] peaks at 0.9258: HIT; with the midpoint 0.805 of its middle piece the peak is 0.8604 (NumPy statement)
    cc = CollisionConstraint(wall_scene())
    gen = HipToppTrajectoryGenerator(0.01, [1.0], [2.0], engine=cc.engine)
    wps = [np.array([0.0]), np.array([0.8]), np.array([0.81]), np.array([0.0])]
    first = cc.certified_spline(wps, **WALL)
    assert first.status == HIT and first.piece == 1 and first.pair == tuple(int(g) for g in cc.engine.contact_pairs()[0][0])
    assert abs(first.s_hit - (1 + 0.25) / 3) < 1e-15 and cc.clearance(first.q_hit, 0.1)[0] <= 0
    # (no sampled constraint: the certificate alone finds the pass through the wall and places the waypoint)
    traj, cert = generate_certified_trajectory(wps, gen, [], cc, **WALL)
    assert len(cert.piece_status) == 4 and len(wps) == 4  # exactly one insertion, into a copy
    print(f"clear_lb {cert.clear_lb}")
    assert cert.status == FREE and cert.piece == -1 and 0 < cert.clear_lb <= 0.889 - 0.8604 + 1e-6
    assert max(float(q[0]) for q in traj.positions) <= 0.8604 + 1e-4
    assert generate_certified_trajectory([np.array([0.0]), np.array([0.86]), np.array([0.87]), np.array([0.0])], gen, [cc], cc,
                                         max_rounds=3, **WALL) is None


# ---- the batches: the models of test_gpu_sweep, 48 random walks each (180 pieces)
MODELS = gpu_models()
IDS = [x[0] for x in MODELS]


@functools.lru_cache(maxsize=None)
def engine_of(k):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = eng_mod.Engine(m, allowed)
    e.set_planning(qidx, base)
    return e


@functools.lru_cache(maxsize=None)
def swept(k, d_min):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    paths = ssr.random_walk_paths(lo, hi, PATHS, SEED)
    W, off = ssr.pack(paths)
    cap = cap_of(e, d_min)
    return paths, W, off, cap, e.sweep_splines(W, off, d_min, cap=cap, max_depth=MAX_DEPTH, lo=lo, hi=hi)


@pytest.mark.parametrize("d_min", [0.0, 0.01])
@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_pieces_equal_the_numpy_loop(k, d_min):
    name, m, allowed, qidx, base, lo, hi = MODELS[k]
    e = engine_of(k)
    paths, W, off, cap, got = swept(k, d_min)
    assert len(got[0]) == 180
    e.sweep_bounds(lo, hi)
    want = ssr.sweep_splines(lambda Q, HD: e.sweep_measure(Q, HD, cap), paths, d_min, MAX_DEPTH, lo, hi)
    cmp = want["margin"] > DECISION
    out = int((~cmp).sum())
    st = got[0]
    print(f"{name}, d_min {d_min}: {out} of {len(cmp)} pieces left out ({out / len(cmp):.3f}); FREE {int((st == FREE).sum())}, HIT "
          f"{int((st == HIT).sum())}, UNDECIDED {int((st == UNDECIDED).sum())}, RANGE {int((st == RANGE).sum())}; nodes per "
          f"piece {got[4].mean():.1f}")
    assert out <= 0.05 * len(cmp)
    for name_, a in zip(NAMES, got):
        b = want[name_]
        if name_ == "clear_lb":
            assert np.array_equal(np.isnan(a[cmp]), np.isnan(b[cmp])), name_
            ok = ~np.isnan(b) & cmp
            worst = float(np.max(np.abs(a[ok] - b[ok]), initial=0.0))
            print(f"largest |clear_lb - NumPy| = {worst:.3e}")
            assert worst <= 1e-9, name_
        else:
            assert np.array_equal(a[cmp], b[cmp], equal_nan=True), name_
    assert got[6].tobytes() == want["M"].tobytes(), "M is the statement's, bit for bit"


@pytest.mark.parametrize("d_min", [0.0, 0.01])
@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_free_pieces_are_free_and_hits_are_hits(k, d_min):
    e = engine_of(k)
    paths, W, off, cap, (st, t_hit, lb, pair, nodes, depth, M) = swept(k, d_min)
    rows, want, hits, at = [], [], [], 0
    for b, P in enumerate(paths):
        Mb = M[off[b]:off[b + 1]]
        for j in range(len(P) - 1):
            i = at + j
            if st[i] == FREE:
                rows.append(ssr.piece_samples(P, Mb, j, 257))
                want.append(max(d_min, lb[i] - 1e-9))
            elif st[i] == HIT:
                hits.append(point(P, Mb, j, t_hit[i]))
        at += len(P) - 1
    free, hit = st == FREE, st == HIT
    assert free.sum() + hit.sum() > 0
    if rows:
        clear = e.clearance(np.concatenate(rows), cap)[0].reshape(len(rows), 257)
        assert np.all(clear >= np.array(want)[:, None])
        assert np.all(lb[free] > 0) and np.all(lb[free] <= cap)
    if hits:
        clear, cp = e.clearance(np.stack(hits), cap)
        assert np.all((clear <= 0) | (clear < d_min))
        assert np.array_equal(cp, pair[hit])


# ---- reductions and forms
def test_two_waypoints_reduce_to_sweep_edges_and_M_is_topp_profiles():
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    paths = ssr.random_walk_paths(lo, hi, 40, seed=9, lengths=(2,))
    W, off = ssr.pack(paths)
    kw = dict(cap=cap_of(e, 0.0), max_depth=MAX_DEPTH, lo=lo, hi=hi)
    got = e.sweep_splines(W, off, **kw)
    edges = e.sweep_edges(W[0::2], W[1::2], **kw)
    assert not got[6].any(), "M of a two-waypoint path is zero"
    e.sweep_bounds(lo, hi)
    want = ssr.sweep_splines(lambda Q, HD: e.sweep_measure(Q, HD, kw["cap"]), paths, 0.0, MAX_DEPTH, lo, hi)
    line = sref.sweep_edges(lambda Q, HD: e.sweep_measure(Q, HD, kw["cap"]), W[0::2], W[1::2], 0.0, MAX_DEPTH, lo, hi)
    cmp = (want["margin"] > DECISION) & (line["margin"] > DECISION)
    print(f"{int((~cmp).sum())} of {len(cmp)} two-waypoint paths left out")
    assert cmp.sum() >= 0.8 * len(cmp)
    for name_, a, b in zip(NAMES, got, edges):
        if name_ == "clear_lb":
            assert np.allclose(a[cmp], b[cmp], rtol=0, atol=1e-9, equal_nan=True)
        else:
            assert np.array_equal(a[cmp], b[cmp], equal_nan=True), name_
    # M: byte-equal to topp_profile's on the same W, whatever the lengths
    paths = ssr.random_walk_paths(lo, hi, 9, seed=2, lengths=(2, 3, 5, 9, 33))
    W, off = ssr.pack(paths)
    lim = np.ones(W.shape[1])
    M = e.topp_profile(W, off, -lim, lim, -lim, lim)[0]
    with_M = e.sweep_splines(W, off, **kw)
    assert with_M[6].tobytes() == M.tobytes()
    without = e.sweep_splines(W, off, want_M=False, **kw)
    assert without[6] is None and all(a.tobytes() == b.tobytes() for a, b in zip(with_M[:6], without[:6]))


@pytest.mark.parametrize("B", [1, 65])
def test_batch_sizes_and_forms(B):
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    paths = ssr.random_walk_paths(lo, hi, B, seed=9)
    W, off = ssr.pack(paths)
    kw = dict(cap=cap_of(e, 0.0), max_depth=16, lo=lo, hi=hi)  # (max_depth 16: chunks of 64 pieces)
    got = e.sweep_splines(W, off, **kw)
    again = e.sweep_splines(W, off, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two identical calls, identical bytes"
    # a path alone gives what it gives in the batch (chunks and packing change nothing)
    for b in (0, B - 1):
        one = e.sweep_splines(paths[b], [0, len(paths[b])], **kw)
        p = slice(off[b] - b, off[b + 1] - b - 1)
        assert all(a.tobytes() == c[p].tobytes() for a, c in zip(one[:6], got[:6]))
        assert one[6].tobytes() == got[6][off[b]:off[b + 1]].tobytes()
    # the device form, with and without M
    n = len(got[0])
    dW, dM = e.alloc(W.nbytes).upload(W), e.alloc(W.nbytes)
    outs = [e.alloc(n * (4 if x in ("status", "pair", "nodes", "depth") else 8)) for x in NAMES]
    try:
        e.sweep_splines_dev(dW.ptr, off, 0.0, dM.ptr, *[o.ptr for o in outs], **kw)
        for x, o, a in zip(NAMES, outs, got):
            assert o.download(a.dtype, n).tobytes() == a.tobytes(), x
        assert dM.download(np.float64, W.size).tobytes() == got[6].tobytes()
        e.sweep_splines_dev(dW.ptr, off, 0.0, None, *[o.ptr for o in outs], **kw)
        for x, o, a in zip(NAMES, outs, got):
            assert o.download(a.dtype, n).tobytes() == a.tobytes(), x
    finally:
        for buf in (dW, dM, *outs):
            buf.free()


# ---- bad inputs and refusals
def test_nonfinite_and_range_paths():
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    paths = ssr.random_walk_paths(lo, hi, 6, seed=2, lengths=(3, 5, 9))
    W, off = ssr.pack(paths)
    ref = e.sweep_splines(W, off, lo=lo, hi=hi)
    bad = W.copy()
    bad[off[1] + 2, 1] = np.nan        # path 1: pieces 2 .. 5
    bad[off[4], 0] = np.inf            # path 4: pieces 16 .. 19
    bad[off[3] + 1, 2] = hi[2] + 1e-3  # path 3, waypoint 1: pieces 14 and 15 of 14 .. 15
    st, t, lb, pair, nodes, depth, M = e.sweep_splines(bad, off, lo=lo, hi=hi)
    piece0 = off[:-1] - np.arange(len(paths))
    nonfinite = list(range(piece0[1], piece0[2])) + list(range(piece0[4], piece0[5]))
    outside = [piece0[3], piece0[3] + 1]
    assert np.all(st[nonfinite] == NONFINITE) and np.all(st[outside] == RANGE)
    for i in nonfinite + outside:
        assert np.isnan(t[i]) and np.isnan(lb[i]) and pair[i] == -1 and nodes[i] == 0 and depth[i] == 0
    for b in (0, 2, 5):  # the other paths as without them
        p = slice(piece0[b], piece0[b] + len(paths[b]) - 1)
        assert all(a[p].tobytes() == c[p].tobytes() for a, c in zip((st, t, lb, pair, nodes, depth), ref))
        assert M[off[b]:off[b + 1]].tobytes() == ref[6][off[b]:off[b + 1]].tobytes()
    assert not np.isfinite(M[off[1]:off[2]][1:-1, 1]).any()  # (the column of the NaN: every interior knot)


def test_argument_refusals():
    name, m, allowed, qidx, base, lo, hi = MODELS[0]
    e = engine_of(0)
    W, off = ssr.pack(ssr.random_walk_paths(lo, hi, 2, seed=2, lengths=(3,)))
    mm = e.sweep_margin_max()
    bad = [dict(d_min=-1e-3), dict(d_min=float("nan")), dict(cap=float("nan")), dict(cap=mm), dict(cap=float("inf")),
           dict(max_depth=-1), dict(max_depth=17), dict(lo=np.full(len(lo), np.nan)), dict(lo=hi + 1.0, hi=hi)]
    for kw in bad:
        with pytest.raises(eng_mod.MjplError) as ei:
            e.sweep_splines(W, off, **kw)
        assert ei.value.code == E_ARG, kw
    F, I, L = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    desc, keep = e.sweep_desc()
    p = lambda a, T: a.ctypes.data_as(T)
    M = np.full_like(W, 7.0)
    st, i32, f64 = np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7.0)
    outs = [p(st, I), p(f64, F), p(f64, F), p(i32, I), p(i32, I), p(i32, I)]
    call = lambda d, w, o, B, m, outs_: e.lib.mjpl_sweep_splines(e.h, d, w, o, B, m, *outs_)
    good = np.array([0, 3, 6], np.int64)
    assert call(None, p(W, F), p(good, L), 2, p(M, F), outs) == E_ARG
    assert call(C.byref(desc), None, p(good, L), 2, p(M, F), outs) == E_ARG
    assert call(C.byref(desc), p(W, F), None, 2, p(M, F), outs) == E_ARG
    assert call(C.byref(desc), p(W, F), p(good, L), 2, p(M, F), [None] + outs[1:]) == E_ARG
    assert call(C.byref(desc), p(W, F), p(good, L), -1, p(M, F), outs) == E_ARG
    for offsets in ([0, 1, 6], [0, 6, 3], [1, 3, 6], [0, 3, 3]):  # a one-waypoint path, falling, not from 0, an empty path
        assert call(C.byref(desc), p(W, F), p(np.array(offsets, np.int64), L), 2, p(M, F), outs) == E_ARG, offsets
    assert np.all(M == 7.0) and np.all(st == 7) and np.all(i32 == 7) and np.all(f64 == 7.0), "a refused call writes nothing"
    assert call(C.byref(desc), None, None, 0, None, [None] * 6) == 0
    assert call(C.byref(desc), p(W, F), p(good, L), 2, None, outs) == 0  # M = NULL is accepted
    with pytest.raises(ValueError):
        e.sweep_splines(W[:, :-1], off)
    del keep


# ---- the constraints
def test_constraints_agree_with_the_engine():
    m = wall_scene()
    cc = CollisionConstraint(m)
    paths = [[q for q in WALL_PATH], [np.array([0.0]), np.array([0.5]), np.array([0.7])], [np.array([0.0]), np.array([0.88])]]
    W, off = ssr.pack([np.array(p) for p in paths])
    for con, d_min, kw in ((cc, 0.0, WALL), (ClearanceConstraint(cc, 0.01, lower=[-2.0], upper=[2.0]), 0.01, dict(cap=0.1))):
        st, t, lb, pair, nodes, depth, M = cc.engine.sweep_splines(W, off, d_min, **WALL)
        certs = con.certified_splines(paths, **kw)
        assert [c.status for c in certs] == [HIT, FREE, FREE if d_min == 0.0 else HIT]
        assert certs[0].piece == 1 and certs[0].s_hit == (1 + t[1]) / 3 and certs[0].pair == tuple(int(g) for g in cc.engine.contact_pairs()[0][0])
        assert np.array_equal(certs[0].q_hit, point(WALL_PATH, M[:4], 1, t[1])) and certs[0].nodes == nodes[:3].sum()
        assert np.isnan(certs[0].clear_lb) and certs[1].clear_lb == lb[3:5].min() and certs[1].piece == -1
        assert certs[1].q_hit is None and np.isnan(certs[1].s_hit) and certs[1].pair is None
        for b, c in enumerate(certs):
            assert np.array_equal(c.piece_status, st[off[b] - b:off[b + 1] - b - 1])
        one = con.certified_spline(paths[2], **kw)
        assert (one.status, one.piece, one.nodes) == (certs[2].status, certs[2].piece, certs[2].nodes)
    assert cc.certified_splines([]) == []
    with pytest.raises(ValueError):
        cc.certified_spline([np.array([0.0])])
