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
