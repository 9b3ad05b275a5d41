"""mjpl_topp_profile* / mjpl_topp_sample* (mjpl_amd/csrc/mjpl_topp.h) against their NumPy statement
(tests/trajectory_reference.py), and the trajectory generators built on them.  Needs the MI355X."""
import ctypes as C

import numpy as np
import pytest

import trajectory_reference as R
from mjpl_amd import (CollisionConstraint, HipToppTrajectoryGenerator, JointLimitConstraint, engine, generate_constrained_trajectories,
                      generate_constrained_trajectory, scenes)
from mjpl_amd.trajectory.topp_trajectory import sample_count

pytestmark = pytest.mark.gpu

TOL = 1e-9  # relative to an array's largest magnitude: the project's bound for NumPy statements (TOL_FIRST_STEP)
CASES = R.parity_cases()
IDS = [c[0] for c in CASES]
G = R.PARITY_GRID
EDGES = R.edge_cases()
EDGE_IDS = [c[0] for c in EDGES]


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(scenes.one_dof_ball(), device=0)
    yield e
    e.close()


def pack(paths):
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in paths]), off


def run(eng, paths, lim, grid=G):
    """[(M, x, u, t, status)] per path of one call."""
    W, off = pack(paths)
    M, x, u, t, status = eng.topp_profile(W, off, *lim, grid=grid)
    g = eng.topp_offsets(off, grid)[1]
    return [(M[off[b]:off[b + 1]], x[g[b]:g[b + 1]], u[g[b]:g[b + 1]], t[g[b]:g[b + 1]], int(status[b])) for b in range(len(paths))]


def close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{what}: max error {err:.3e} on a scale of {scale:.3e}")
    assert err <= TOL * max(scale, 1e-300), what


def same_bits(a, b):
    return all(np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for p, q in zip(a[:4], b[:4])) and a[4] == b[4]


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_parity_with_the_statement(eng, k):
    _, W, *lim = CASES[k]
    want = R.parity_profile(k)
    M, x, u, t, status = run(eng, [W], lim)[0]
    assert status == engine.TOPP_OK == want["status"]
    for name, got in (("M", M), ("x", x), ("u", u), ("t", t)):
        close(got, want[name], f"{IDS[k]} {name}")
    assert x[0] == 0 and x[-1] == 0 and u[-1] == 0 and t[0] == 0


def test_offsets_mixed_lengths_and_batch_sizes(eng):
    ids = [IDS.index(f"d4-n{n}") for n in (2, 3, 17)]
    paths, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    alone = [run(eng, [p], lim)[0] for p in paths]
    together = run(eng, paths, lim)
    for a, b in zip(alone, together):
        assert same_bits(a, b)
    # more paths than a workgroup has waves, and more than one wave per CU: copies of one path, identical bits
    for B in (65, 257):
        out = run(eng, [paths[2]] * B, lim)
        assert all(same_bits(o, alone[2]) for o in out), B
    mixed = run(eng, (paths * 22)[:65], lim)
    assert all(same_bits(o, alone[k % 3]) for k, o in enumerate(mixed))


@pytest.mark.parametrize("vmax, grid, T", [(10.0, 2, 2.0), (10.0, 16, 2.0), (0.5, 8, 2.5), (0.5, 16, 2.5)])
def test_closed_forms(eng, vmax, grid, T):
    _, x, u, t, status = run(eng, [[[0.0], [1.0]]], ([-vmax], [vmax], [-1.0], [1.0]), grid)[0]
    assert status == engine.TOPP_OK and abs(t[-1] - T) <= 1e-12


def sample_on_gpu(eng, paths, lim, dt, grid=G):
    W, off = pack(paths)
    M, x, u, t, status = eng.topp_profile(W, off, *lim, grid=grid)
    g = eng.topp_offsets(off, grid)[1]
    counts = [sample_count(t[g[b + 1] - 1], dt) for b in range(len(paths))]
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos, vel, acc = eng.topp_sample(W, off, M, x, u, t, dt, soff, *lim, grid=grid)
    out = []
    for b in range(len(paths)):
        prof = dict(M=M[off[b]:off[b + 1]], x=x[g[b]:g[b + 1]], u=u[g[b]:g[b + 1]], t=t[g[b]:g[b + 1]])
        s = slice(soff[b], soff[b + 1])
        out.append((prof, pos[s], vel[s], acc[s]))
    return out


def test_samples_match_the_statement(eng):
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17", "d3-n2")]
    paths, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    together = sample_on_gpu(eng, paths, lim, 0.05)
    for b, (prof, pos, vel, acc) in enumerate(together):
        want = R.sample(paths[b], prof, 0.05)  # the statement on the profile the GPU returned
        assert len(pos) == len(want[0]) > 1
        for name, got, w in zip(("pos", "vel", "acc"), (pos, vel, acc), want):
            close(got, w, f"path {b} {name}")
        alone = sample_on_gpu(eng, [paths[b]], lim, 0.05)[0]  # samp_off across paths changes nothing
        assert all(np.array_equal(p, q) for p, q in zip(alone[1:], (pos, vel, acc)))


def test_sample_counts(eng):
    lim = ([-10.0], [10.0], [-1.0], [1.0])
    line = [[[0.0], [1.0]]]  # T = 2
    for dt, m in ((0.25, 8), (0.3, 7), (3.0, 1)):
        prof, pos, vel, acc = sample_on_gpu(eng, line, lim, dt, grid=2)[0]
        assert prof["t"][-1] == 2.0 and len(pos) == m
        assert abs(pos[-1, 0] - 1.0) <= 1e-12 and abs(vel[-1, 0]) <= 1e-12  # the last sample is at T itself
        if m > 1:
            assert abs(pos[0, 0] - 0.5 * dt * dt) <= 1e-12 and abs(vel[0, 0] - dt) <= 1e-12 and abs(acc[0, 0] - 1.0) <= 1e-12


def test_reference_trajectory_case(eng):
    # the reference's own generator test: 7 columns, two random waypoints, unit limits, dt 0.002.  A straight path makes
    # the discretisation exact, so the limits hold at every sample
    rng = np.random.default_rng(5)
    waypoints = [rng.random(7), rng.random(7)]
    gen = HipToppTrajectoryGenerator(0.002, np.ones(7), np.ones(7), engine=eng)
    traj = gen.generate_trajectory(waypoints)
    assert traj is not None and traj.dt == 0.002 and np.array_equal(traj.q_init, waypoints[0])
    assert len(traj.positions) == len(traj.velocities) == len(traj.accelerations)
    assert np.abs(np.stack(traj.velocities)).max() <= 1 + 1e-8
    assert np.abs(np.stack(traj.accelerations)).max() <= 1 + 1e-8
    np.testing.assert_allclose(traj.positions[-1], waypoints[1], rtol=1e-5, atol=1e-8)
    assert np.abs(traj.velocities[-1]).max() <= 1e-8
    T = gen.durations([waypoints])[0]
    assert len(traj.positions) == sample_count(T, 0.002) and abs(T - R.profile(np.array(waypoints), -np.ones(7), np.ones(7), -np.ones(7), np.ones(7), 8)["t"][-1]) <= TOL * T


@pytest.mark.parametrize("name", ["d3-n17", "d7-n64", "asymmetric"])
def test_limits_on_curved_paths(eng, name):
    k = IDS.index(name)
    _, W, vmin, vmax, amin, amax = CASES[k]
    want = R.parity_profile(k)
    prof, pos, vel, acc = sample_on_gpu(eng, [W], (vmin, vmax, amin, amax), 0.01)[0]
    x, u, a, b = prof["x"], prof["u"], want["a"], want["b"]
    N = len(x) - 1
    # at the grid points, from the returned x and u
    v = a * np.sqrt(x)[:, None]
    assert np.all(v <= vmax * (1 + 1e-9)) and np.all(v >= vmin * (1 + 1e-9))
    for g in (a[:-1] * u[:N, None] + b[:-1] * x[:-1, None], a[1:] * u[:N, None] + b[1:] * x[1:, None]):
        assert np.all(g <= amax * (1 + 1e-9)) and np.all(g >= amin * (1 + 1e-9))
    # between them the discretisation overshoots: the kernel may add nothing to the statement's own figure
    _, _, acc_ref = R.sample(W, want, 0.01)
    over = lambda A: max((A / amax).max(), (A / amin).max(), 1.0) - 1.0
    print(f"{name}: sampled acceleration overshoot {over(acc):.3e}, the statement's {over(acc_ref):.3e}")
    assert over(acc) <= over(acc_ref) + 1e-9


def test_statuses(eng):
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17")]
    good, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    bad = good[1].copy()
    bad[5, 1] = np.nan
    alone = [run(eng, [p], lim)[0] for p in good]
    out = run(eng, [good[0], bad, good[1]], lim)
    assert out[1][4] == engine.TOPP_NONFINITE and all(np.all(np.isnan(a)) for a in out[1][:4])
    assert same_bits(out[0], alone[0]) and same_bits(out[2], alone[1])
    gen = HipToppTrajectoryGenerator(0.05, lim[1], lim[3], engine=eng)
    trajs = gen.generate_trajectories([good[0], bad, good[1]])
    assert trajs[1] is None and trajs[0] is not None and trajs[2] is not None
    assert np.isnan(gen.durations([good[0], bad])[1])
    with pytest.raises(ValueError):
        gen.generate_trajectory([good[0][0], good[0][0], good[0][1]])  # two equal waypoints
    with pytest.raises(ValueError):
        gen.generate_trajectory([good[0][0]])


def test_run_to_run_identity(eng):
    paths, lim = [CASES[k][1] for k in range(len(CASES)) if CASES[k][1].shape[1] == 7], CASES[IDS.index("d7-n2")][2:]
    first = run(eng, paths, lim)
    for _ in range(2):
        assert all(same_bits(a, b) for a, b in zip(first, run(eng, paths, lim)))


def test_host_and_device_forms_agree(eng):
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17", "d3-n2")]
    paths, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    W, off = pack(paths)
    M, x, u, t, status = eng.topp_profile(W, off, *lim, grid=G)
    g = eng.topp_offsets(off, G)[1]
    soff = np.concatenate([[0], np.cumsum([sample_count(t[g[b + 1] - 1], 0.05) for b in range(3)])]).astype(np.int64)
    pos, vel, acc = eng.topp_sample(W, off, M, x, u, t, 0.05, soff, *lim, grid=G)
    dW = eng.alloc(W.nbytes).upload(W)
    dM, dx, du, dt = eng.alloc(M.nbytes), eng.alloc(x.nbytes), eng.alloc(x.nbytes), eng.alloc(x.nbytes)
    dst = eng.alloc(4 * 3)
    dpos, dvel, dacc = (eng.alloc(pos.nbytes) for _ in range(3))
    try:
        eng.topp_profile_dev(dW.ptr, off, 3, *lim, G, dM.ptr, dx.ptr, du.ptr, dt.ptr, dst.ptr)
        eng.topp_sample_dev(dW.ptr, off, 3, dM.ptr, dx.ptr, du.ptr, dt.ptr, 0.05, soff, *lim, G, dpos.ptr, dvel.ptr, dacc.ptr)
        for buf, want in ((dM, M), (dx, x), (du, u), (dt, t), (dpos, pos), (dvel, vel), (dacc, acc)):
            got = buf.download(np.float64, want.size)
            assert np.array_equal(got.view(np.uint64), want.reshape(-1).view(np.uint64))
        assert np.array_equal(dst.download(np.int32, 3), status)
    finally:
        for buf in (dW, dM, dx, du, dt, dst, dpos, dvel, dacc):
            buf.free()


def test_argument_errors(eng):
    W = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]])
    off = np.array([0, 3], np.int64)
    one, lim = np.ones(2), (-np.ones(2), np.ones(2), -np.ones(2), np.ones(2))
    M, x, u, t, status = eng.topp_profile(W, off, *lim)
    soff = np.array([0, 4], np.int64)

    def code(f, *a, **k):
        with pytest.raises(engine.MjplError) as err:
            f(*a, **k)
        return err.value.code

    ARG, CAP = -1, -4
    assert code(eng.topp_profile, W, off, *lim, grid=1) == ARG
    assert code(eng.topp_profile, W, np.array([0, 1, 3], np.int64), *lim) == ARG  # a path of one waypoint
    assert code(eng.topp_profile, W, np.array([0, 3, 3], np.int64), *lim) == ARG
    for j in range(4):  # a limit of the wrong sign, zero, NaN, infinite
        for v in (-lim[j][1], 0.0, np.nan, np.inf * lim[j][1]):
            l = [a.copy() for a in lim]
            l[j][1] = v
            assert code(eng.topp_profile, W, off, *l) == ARG, (j, v)
    W17 = np.zeros((2, 17))
    W17[1] = 1
    assert code(eng.topp_profile, W17, off[:1].tolist() + [2], -np.ones(17), np.ones(17), -np.ones(17), np.ones(17)) == CAP
    for dt in (0.0, -0.1, np.nan):
        assert code(eng.topp_sample, W, off, M, x, u, t, dt, soff, *lim) == ARG
    # samp_off that falls (two paths)
    W2, off2 = np.concatenate([W, W]), np.array([0, 3, 6], np.int64)
    M2, x2, u2, t2, _ = eng.topp_profile(W2, off2, *lim)
    assert code(eng.topp_sample, W2, off2, M2, x2, u2, t2, 0.1, np.array([0, 4, 2], np.int64), *lim) == ARG
    # NULL pointers, straight at the ABI
    lib, F64, I64, I32 = eng.lib, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    desc, keep = eng.topp_desc(2, 8, *lim)
    p = lambda a, T=F64: a.ctypes.data_as(T)
    full = [eng.h, C.byref(desc), p(W), p(off, I64), 1, p(M), p(x), p(u), p(t), p(status, I32)]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        args = list(full)
        args[k] = None
        assert lib.mjpl_topp_profile(*args) == ARG, k
        assert lib.mjpl_topp_profile_dev(*args) == ARG, k
    pos = np.zeros((4, 2))
    full = [eng.h, C.byref(desc), p(W), p(off, I64), 1, p(M), p(x), p(u), p(t), 0.1, p(soff, I64), p(pos), p(pos), p(pos)]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13):
        args = list(full)
        args[k] = None
        assert lib.mjpl_topp_sample(*args) == ARG, k
        assert lib.mjpl_topp_sample_dev(*args) == ARG, k
    null_lim = engine.ToppDesc(2, 8, None, p(one), p(one), p(one))
    assert lib.mjpl_topp_profile(eng.h, C.byref(null_lim), *full[2:4], 1, *full[5:9], p(status, I32)) == ARG
    # nothing to do is not an error
    assert lib.mjpl_topp_profile(eng.h, C.byref(desc), None, None, 0, None, None, None, None, None) == 0


# ---- what the parity list leaves out: block edges of the forward sweep, grids that are no power of two, the row without
# u, dead rows at d = 16 (trajectory_reference.edge_cases; test_trajectory_host.py ties the statement on them to an LP)

@pytest.mark.parametrize("k", range(len(EDGES)), ids=EDGE_IDS)
def test_parity_on_the_edge_cases(eng, k):
    name, W, *lim, grid = EDGES[k]
    want = R.edge_profile(k)
    M, x, u, t, status = run(eng, [W], lim, grid)[0]
    assert status == engine.TOPP_OK == want["status"]
    assert len(x) == (len(W) - 1) * grid + 1
    for what, got in (("M", M), ("x", x), ("u", u), ("t", t)):
        close(got, want[what], f"{name} {what}")
    assert x[0] == 0 and x[-1] == 0 and u[-1] == 0 and t[0] == 0


@pytest.mark.parametrize("name", ["N65", "reversal-2d", "d16-still-0-15"])
def test_samples_on_the_edge_cases(eng, name):
    _, W, *lim, grid = EDGES[EDGE_IDS.index(name)]
    prof, pos, vel, acc = sample_on_gpu(eng, [W], lim, 0.05, grid)[0]
    want = R.sample(W, prof, 0.05)  # the statement on the profile the GPU returned
    assert len(pos) == len(want[0]) > 1
    for what, got, w in zip(("pos", "vel", "acc"), (pos, vel, acc), want):
        close(got, w, f"{name} {what}")


# ---- chunks of paths (launch_topp_profile): option "topp_chunk_bytes" makes them small enough to cross at these shapes

DEFAULT_CHUNK_BYTES = 512 << 20


def chunk_bounds(paths, d, grid, chunk_bytes):
    """[(b0, b1)] by the documented rule: a chunk takes paths while the workspace of its grid points, (5 * 2d + 1) * 8
    bytes each, fits chunk_bytes, and always at least one path."""
    per_pt = (5 * 2 * d + 1) * 8
    pts = [(len(p) - 1) * grid + 1 for p in paths]
    out, b0 = [], 0
    while b0 < len(paths):
        b1, have = b0 + 1, pts[b0]
        while b1 < len(paths) and (have + pts[b1]) * per_pt <= chunk_bytes:
            have += pts[b1]
            b1 += 1
        out.append((b0, b1))
        b0 = b1
    return out


@pytest.fixture()
def chunk_eng():
    """An engine of its own: its workspace starts empty, so the first chunked call grows it from chunk to chunk."""
    e = engine.Engine(scenes.one_dof_ball(), device=0)
    assert e.get_option("topp_chunk_bytes") == DEFAULT_CHUNK_BYTES and e.get_option("topp_last_chunks") == 0
    yield e
    e.close()


def test_chunks_change_no_bit(eng, chunk_eng):
    e = chunk_eng
    ids = [IDS.index(f"d4-n{n}") for n in (2, 3, 17)]
    three, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    paths = (three * 22)[:65]
    sizes = (1, 8192, 65536, 200000, DEFAULT_CHUNK_BYTES)
    # (the chunked runs come first, the smallest chunks first: chunks 1, 2, 3 of the first call each need a larger workspace
    #  than the one before, later ones a smaller)
    got, counts = {}, {}
    for v in sizes:
        e.set_option("topp_chunk_bytes", v)
        assert e.get_option("topp_chunk_bytes") == v
        got[v] = run(e, paths, lim)
        counts[v] = int(e.get_option("topp_last_chunks"))
    alone = [run(e, [p], lim)[0] for p in three]  # (at the default: the loop's last value)
    assert e.get_option("topp_last_chunks") == 1
    also = [run(eng, [p], lim)[0] for p in three]  # ... and on another engine
    assert all(same_bits(a, b) for a, b in zip(alone, also))
    for v in sizes:
        want = len(chunk_bounds(paths, 4, G, v))
        print(f"topp_chunk_bytes {v}: {counts[v]} chunks, {want} by the rule")
        assert counts[v] == want, v
        if v == 1:
            assert want == 65  # every path its own chunk: one path may exceed the size
        elif v == DEFAULT_CHUNK_BYTES:
            assert want == 1
        else:
            assert want >= 3  # (the input must cross boundaries, whatever becomes of the sizes)
        assert all(o[4] == engine.TOPP_OK for o in got[v])
        assert all(same_bits(o, alone[k % 3]) for k, o in enumerate(got[v])), v
    with pytest.raises(engine.MjplError):
        e.set_option("topp_chunk_bytes", 0)
    with pytest.raises(engine.MjplError):
        e.set_option("topp_last_chunks", 1)
    # B = 0 launches nothing and says so
    desc, keep = e.topp_desc(4, G, *lim)
    assert e.lib.mjpl_topp_profile(e.h, C.byref(desc), None, None, 0, None, None, None, None, None) == 0
    assert e.get_option("topp_last_chunks") == 0


def test_chunks_at_sixteen_columns_and_on_device_pointers(chunk_eng):
    e = chunk_eng
    k2 = IDS.index("d16-n2")
    three = [EDGES[EDGE_IDS.index("N129")][1], EDGES[EDGE_IDS.index("d16-still-0-15")][1], CASES[k2][1]]
    lim = CASES[k2][2:]  # a batch has one set of limits and one grid: N129's grid keeps its N at 129, one past two blocks
    paths = (three * 3)[:9]
    grid = EDGES[EDGE_IDS.index("N129")][6]
    bounds = chunk_bounds(paths, 16, grid, 8192)
    assert len(bounds) >= 3
    e.set_option("topp_chunk_bytes", 8192)
    chunked = run(e, paths, lim, grid)
    assert e.get_option("topp_last_chunks") == len(bounds)
    # the same call on device pointers
    W, off = pack(paths)
    g = e.topp_offsets(off, grid)[1]
    ng = int(g[-1])
    dW = e.alloc(W.nbytes).upload(W)
    dM, dx, du, dt, dst = e.alloc(W.nbytes), e.alloc(8 * ng), e.alloc(8 * ng), e.alloc(8 * ng), e.alloc(4 * len(paths))
    try:
        e.topp_profile_dev(dW.ptr, off, W.shape[1], *lim, grid, dM.ptr, dx.ptr, du.ptr, dt.ptr, dst.ptr)
        assert e.get_option("topp_last_chunks") == len(bounds)
        M = dM.download(np.float64, W.size).reshape(W.shape)
        x, u, t = (b.download(np.float64, ng) for b in (dx, du, dt))
        status = dst.download(np.int32, len(paths))
    finally:
        for buf in (dW, dM, dx, du, dt, dst):
            buf.free()
    dev = [(M[off[b]:off[b + 1]], x[g[b]:g[b + 1]], u[g[b]:g[b + 1]], t[g[b]:g[b + 1]], int(status[b])) for b in range(len(paths))]
    e.set_option("topp_chunk_bytes", DEFAULT_CHUNK_BYTES)
    alone = [run(e, [p], lim, grid)[0] for p in three]
    assert e.get_option("topp_last_chunks") == 1
    assert all(a[4] == engine.TOPP_OK for a in alone)
    for k in range(len(paths)):
        assert same_bits(chunked[k], alone[k % 3]), k
        assert same_bits(dev[k], alone[k % 3]), k


def test_nonfinite_path_inside_and_first_in_a_chunk(chunk_eng):
    e = chunk_eng
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17")]
    (g0, g1), lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    bad = g1.copy()
    bad[5, 1] = np.nan
    paths = [g0, bad, g0, bad, g1, g0]
    bounds = chunk_bounds(paths, 3, G, 70000)
    assert bounds == [(0, 3), (3, 6)]  # path 1 in the middle of its chunk, path 3 the first of its
    alone = {id(p): run(e, [p], lim)[0] for p in (g0, g1)}
    e.set_option("topp_chunk_bytes", 70000)
    out = run(e, paths, lim)
    assert e.get_option("topp_last_chunks") == 2
    e.set_option("topp_chunk_bytes", DEFAULT_CHUNK_BYTES)
    for b, p in enumerate(paths):
        if p is bad:
            assert out[b][4] == engine.TOPP_NONFINITE and all(np.all(np.isnan(a)) for a in out[b][:4]), b
        else:
            assert same_bits(out[b], alone[id(p)]), b


# ---- MJPL_TOPP_STALLED, and sampling where there is little or nothing to sample

def stalled_batch():
    """[good, stalled, good] at d = 1 with the limits of the fixed edge cases (v = +-1, a = +-2, G = 8)."""
    Ws, *lim, grid = R.stalled_case()
    good = [EDGES[EDGE_IDS.index(n)] for n in ("reversal-1d", "repeat")]
    assert grid == G and all(c[6] == G and all(np.array_equal(a, b) for a, b in zip(c[2:6], lim)) for c in good)
    return [good[0][1], Ws, good[1][1]], lim


def test_status_stalled(eng):
    paths, lim = stalled_batch()
    want = R.profile(paths[1], *lim, G)
    assert want["status"] == R.STALLED
    alone = [run(eng, [p], lim)[0] for p in (paths[0], paths[2])]
    out = run(eng, paths, lim)
    M, x, u, t, status = out[1]
    assert status == engine.TOPP_STALLED == want["status"]
    close(M, want["M"], "stalled M")
    assert np.all(x == 0) and np.array_equal(x, want["x"])
    assert np.array_equal(u, want["u"], equal_nan=True) and np.array_equal(t, want["t"], equal_nan=True)
    assert t[-1] == np.inf
    assert same_bits(out[0], alone[0]) and same_bits(out[2], alone[1])
    assert alone[0][4] == alone[1][4] == engine.TOPP_OK
    gen = HipToppTrajectoryGenerator(0.05, lim[1], lim[3], engine=eng, allow_repeated_waypoints=True)
    trajs = gen.generate_trajectories(paths)
    assert trajs[1] is None and trajs[0] is not None and trajs[2] is not None
    T = gen.durations(paths)
    assert not np.isfinite(T[1]) and np.isfinite(T[0]) and np.isfinite(T[2])


def profile_and_counts(eng, paths, lim, dt):
    W, off = pack(paths)
    prof = eng.topp_profile(W, off, *lim, grid=G)
    g = eng.topp_offsets(off, G)[1]
    T = [prof[3][g[b + 1] - 1] for b in range(len(paths))]
    return W, off, prof, [sample_count(v, dt) if np.isfinite(v) else 0 for v in T]


def sample_with(eng, W, off, prof, counts, lim, dt):
    """[(pos, vel, acc)] per path, from samp_off built on the host out of `counts`."""
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos, vel, acc = eng.topp_sample(W, off, *prof[:4], dt, soff, *lim, grid=G)
    return [(pos[soff[b]:soff[b + 1]], vel[soff[b]:soff[b + 1]], acc[soff[b]:soff[b + 1]]) for b in range(len(counts))]


def sampled_alone(eng, path, lim, dt, count):
    W, off, prof, _ = profile_and_counts(eng, [path], lim, dt)
    return sample_with(eng, W, off, prof, [count], lim, dt)[0]


@pytest.mark.parametrize("counts", [(5, 0, 4, 0), (0, 3, 0, 0, 2)], ids=["middle-and-end", "first-and-two-in-a-row"])
def test_paths_without_samples_are_passed_over(eng, counts):
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17", "d3-n2")]
    three, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    paths = (three * 2)[:len(counts)]
    W, off, prof, full = profile_and_counts(eng, paths, lim, 0.05)
    assert all(c <= f for c, f in zip(counts, full))
    got = sample_with(eng, W, off, prof, counts, lim, 0.05)
    for b, c in enumerate(counts):
        assert all(len(a) == c for a in got[b])
        if c:
            want = sampled_alone(eng, paths[b], lim, 0.05, c)
            assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(got[b], want)), b


def test_samples_past_the_duration_rest_at_the_last_waypoint(eng):
    ids = [IDS.index(n) for n in ("d3-n3", "d3-n17", "d3-n2")]
    paths, lim = [CASES[k][1] for k in ids], CASES[ids[0]][2:]
    W, off, prof, full = profile_and_counts(eng, paths, lim, 0.05)
    counts = [full[0], full[1] + 3, full[2]]
    got = sample_with(eng, W, off, prof, counts, lim, 0.05)
    pos, vel, _ = got[1]
    assert len(pos) == full[1] + 3
    for k in range(full[1], full[1] + 3):  # past the duration: at T itself, like the last sample of test_sample_counts
        assert np.abs(pos[k] - paths[1][-1]).max() <= 1e-12 and np.abs(vel[k]).max() <= 1e-12, k
    assert all(np.array_equal(a[full[1]:], np.broadcast_to(a[-1], (3, 3))) for a in got[1])  # ... one and the same row
    want = sampled_alone(eng, paths[1], lim, 0.05, full[1])  # the rows before them are not moved
    assert all(np.array_equal(p[:full[1]].view(np.uint64), q.view(np.uint64)) for p, q in zip(got[1], want))
    for b in (0, 2):
        want = sampled_alone(eng, paths[b], lim, 0.05, full[b])
        assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(got[b], want)), b


def test_sampling_paths_that_are_not_ok_returns(eng):
    """include/mjpl_hip.h: "sampling a path that is not OK reads NaN / inf times and gives meaningless rows, never a
    fault" -- k_topp_sample clamps its interval to [0, N-1] and its segment to [0, n-2] whatever t, x and u hold.  The
    call returns MJPL_OK (the binding raises otherwise) and the good paths' rows are what they are alone; nothing is
    asserted about the other rows."""
    paths, lim = stalled_batch()
    nan_path = paths[0].copy()
    nan_path[1, 0] = np.nan
    paths = [paths[0], nan_path, paths[1], paths[2]]
    W, off, prof, full = profile_and_counts(eng, paths, lim, 0.05)
    assert [int(s) for s in prof[4]] == [engine.TOPP_OK, engine.TOPP_NONFINITE, engine.TOPP_STALLED, engine.TOPP_OK]
    counts = [full[0], 3, 3, full[3]]
    got = sample_with(eng, W, off, prof, counts, lim, 0.05)
    assert all(len(a) == 3 for b in (1, 2) for a in got[b])
    for b in (0, 3):
        want = sampled_alone(eng, paths[b], lim, 0.05, full[b])
        assert full[b] > 1 and all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(got[b], want)), b


# ---- end to end: a spline that cuts the corner of the wall of scenes.two_dof_ball()

def corner_paths():
    # along the top of the wall (x in [0.5, 0.7], |y| <= 0.5; the ball's radius is 0.1), then a sharp turn upwards: the
    # spline rings below the straight segment before the turn, into the corner at (0.7, 0.5)
    return [[np.array(p) for p in ((-0.2, y), (0.3, y), (0.9, y), (0.9, 1.5))] for y in (0.63, 0.64, 0.625)]


class RecordingGenerator(HipToppTrajectoryGenerator):
    """Notes the number of waypoints of every path it is given."""

    def generate_trajectories(self, paths):
        paths = list(paths)
        self.lengths = getattr(self, "lengths", []) + [[len(p) for p in paths]]
        return super().generate_trajectories(paths)


def wall_clearance(P):
    P = np.atleast_2d(P)
    return np.hypot(np.maximum(np.abs(P[:, 0] - 0.6) - 0.1, 0), np.maximum(np.abs(P[:, 1]) - 0.5, 0)) - 0.1


def test_constrained_trajectory_around_the_wall_corner():
    model = scenes.two_dof_ball()
    collision = CollisionConstraint(model)
    constraints = [JointLimitConstraint(model), collision]
    gen = RecordingGenerator(0.01, [1.0, 1.0], [2.0, 2.0], engine=collision.engine)
    paths = corner_paths()
    for path in paths:  # the statement: the polyline is free, the spline is not
        W = np.array(path)
        M = R.spline_second_derivatives(W)
        curve = np.array([R.spline_at(W, M, s)[0] for s in np.linspace(0, 1, 601)])
        poly = np.concatenate([W[i] + np.linspace(0, 1, 101)[:, None] * (W[i + 1] - W[i]) for i in range(len(W) - 1)])
        assert wall_clearance(poly).min() > 0.02 and wall_clearance(curve).min() < -0.01
        at = curve[np.argmin(wall_clearance(curve))]
        assert abs(at[0] - 0.7) < 0.05 and 0.5 < at[1] < 0.6  # ... at the corner
    plain = gen.generate_trajectory(paths[0])
    single = []
    assert not collision.valid_configs(np.stack(plain.positions)).all()
    for path in paths:
        traj = generate_constrained_trajectory(path, gen, constraints, max_rounds=32)
        single.append(traj)
        assert traj is not None and len(path) == 4
        P = np.stack(traj.positions)
        assert all(c.valid_configs(P).all() for c in constraints)
        assert wall_clearance(P).min() >= -1e-9
        np.testing.assert_allclose(P[-1], path[-1], atol=1e-9)
        assert gen.lengths[-1][0] > len(path)  # the trajectory returned follows more waypoints than were given
    batch = generate_constrained_trajectories(paths, gen, constraints, max_rounds=32)
    for a, b in zip(single, batch):
        assert b is not None and np.array_equal(np.stack(a.positions), np.stack(b.positions))
        assert np.array_equal(np.stack(a.velocities), np.stack(b.velocities))
        assert np.array_equal(np.stack(a.accelerations), np.stack(b.accelerations))
