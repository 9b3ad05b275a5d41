"""mjpl_jerk_profile* / mjpl_jerk_sample* (mjpl_amd/csrc/mjpl_jerk.h) against their NumPy statement
(tests/jerk_reference.py), and HipJerkTrajectoryGenerator built on them.  Needs the MI355X."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import jerk_reference as J
from mjpl_amd import (CollisionConstraint, HipJerkTrajectoryGenerator, JointLimitConstraint, ModelBuilder, engine,
                      generate_certified_trajectory, generate_constrained_trajectory, scenes)
from mjpl_amd.trajectory.topp_trajectory import sample_count

pytestmark = pytest.mark.gpu

TOL = 1e-9  # relative to an array's largest magnitude: the project's bound for NumPy statements
CASES = J.parity_cases()
IDS = [c[0] for c in CASES]
EDGES = J.edge_cases()
EDGE_IDS = [c[0] for c in EDGES]
NAMES = ("M", "lim", "v", "vp", "tc", "t")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(scenes.one_dof_ball(), device=0)
    yield e
    e.close()


def pack(paths):
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in paths]), off


def run(eng, paths, lim, grid):
    """[(M, lim, v, vp, tc, t, status)] per path of one call."""
    W, off = pack(paths)
    M, L, v, vp, tc, t, status = eng.jerk_profile(W, off, *lim, grid=grid)
    g = eng.topp_offsets(off, grid)[1]
    return [(M[off[b]:off[b + 1]], L[g[b]:g[b + 1]], *(a[g[b]:g[b + 1]] for a in (v, vp, tc, t)), int(status[b]))
            for b in range(len(paths))]


def bits_differing(got, want):
    """The largest distance of two entries in units of the last place (0: the same bits everywhere)."""
    a, b = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    key = lambda x: np.where(x.view(np.int64) < 0, np.int64(-2**63) - x.view(np.int64), x.view(np.int64))
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


def close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{what}: max error {err:.3e} on a scale of {scale:.3e}, {bits_differing(got, want)} ulp")
    assert err <= TOL * max(scale, 1e-300), what


def same_bits(a, b):
    return all(np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for p, q in zip(a[:6], b[:6])) and a[6] == b[6]


def check_against(out, want, name):
    assert out[6] == engine.TOPP_OK == want["status"]
    for what, got in zip(NAMES, out[:6]):
        close(got, want[what], f"{name} {what}")
    v, vp, tc, t = out[2:6]
    assert v[0] == 0 and v[-1] == 0 and vp[-1] == 0 and tc[-1] == 0 and t[0] == 0 and np.all(out[1][-1] == 0)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_parity_with_the_statement(eng, k):
    name, W, *lim, grid = CASES[k]
    check_against(run(eng, [W], lim, grid)[0], J.shared_profile("parity", k), name)


@pytest.mark.parametrize("k", range(len(EDGES)), ids=EDGE_IDS)
def test_parity_on_the_block_edges(eng, k):
    name, W, *lim, grid = EDGES[k]
    out = run(eng, [W], lim, grid)[0]
    assert len(out[2]) == (len(W) - 1) * grid + 1
    check_against(out, J.shared_profile("edge", k), name)


def test_one_interval(eng):
    k = IDS.index("d1-n2-G1")
    _, W, *lim, grid = CASES[k]
    M, L, v, vp, tc, t, status = run(eng, [W], lim, grid)[0]
    assert status == engine.TOPP_OK and len(v) == 2 and np.all(v == 0) and vp[0] > 0 and t[1] > 0 and np.all(M == 0)


@pytest.mark.parametrize("goal, v, grid, T", [(1.0, 1.0, 1, 32.0 ** (1 / 3)), (10.0, 1.0, 2, 12.0), (1.0, 0.5, 2, 2 + np.sqrt(2))])
def test_closed_forms(eng, goal, v, grid, T):
    out = run(eng, [[[0.0], [goal]]], ([v], [1.0], [1.0]), grid)[0]
    assert out[6] == engine.TOPP_OK and abs(out[5][-1] - T) <= 1e-12 * T


def three_paths():
    """Paths of 2, 3 and 17 waypoints of three columns, one set of limits, grid 2."""
    ids = [IDS.index(n) for n in ("d3-n2-G2", "d3-n3-G4", "d3-n17-G1")]
    return [CASES[k][1] for k in ids], CASES[ids[2]][2:5], 2


def test_batches_of_one_five_and_257(eng):
    three, lim, grid = three_paths()
    alone = [run(eng, [p], lim, grid)[0] for p in three]
    assert all(a[6] == engine.TOPP_OK for a in alone)
    for B in (5, 257):  # mixed lengths: four paths per workgroup, more workgroups than one
        out = run(eng, (three * 86)[:B], lim, grid)
        assert all(same_bits(o, alone[k % 3]) for k, o in enumerate(out)), B
    out = run(eng, [three[2]] * 257, lim, grid)
    assert all(same_bits(o, alone[2]) for o in out)


def profile_and_counts(eng, paths, lim, grid, dt):
    W, off = pack(paths)
    prof = eng.jerk_profile(W, off, *lim, grid=grid)
    g = eng.topp_offsets(off, grid)[1]
    T = [prof[5][g[b + 1] - 1] for b in range(len(paths))]
    return W, off, prof, [sample_count(v, dt) if np.isfinite(v) else 0 for v in T]


def sample_with(eng, W, off, prof, counts, lim, grid, dt):
    """[(pos, vel, acc)] per path, from samp_off built on the host out of `counts`."""
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos, vel, acc = eng.jerk_sample(W, off, *prof[:6], dt, soff, *lim, grid=grid)
    return [(pos[soff[b]:soff[b + 1]], vel[soff[b]:soff[b + 1]], acc[soff[b]:soff[b + 1]]) for b in range(len(counts))]


def statement_profile(prof, off, g, b):
    return dict(M=prof[0][off[b]:off[b + 1]], lim=prof[1][g[b]:g[b + 1]], v=prof[2][g[b]:g[b + 1]], vp=prof[3][g[b]:g[b + 1]],
                tc=prof[4][g[b]:g[b + 1]], t=prof[5][g[b]:g[b + 1]])


@pytest.mark.parametrize("name", ["d3-n17-G1", "d7-n3-G1", "d16-n2-G1", "asymmetric", "repeat"])
def test_samples_match_the_statement(eng, name):
    _, W, *lim, grid = CASES[IDS.index(name)]
    dt = 0.05
    Wp, off, prof, full = profile_and_counts(eng, [W], lim, grid, dt)
    pos, vel, acc = sample_with(eng, Wp, off, prof, full, lim, grid, dt)[0]
    want = J.sample(W, statement_profile(prof, off, eng.topp_offsets(off, grid)[1], 0), dt)  # on the profile the GPU returned
    assert len(pos) == len(want[0]) > 1
    for what, got, w in zip(("pos", "vel", "acc"), (pos, vel, acc), want):
        close(got, w, f"{name} {what}")
    assert np.array_equal(pos[-1], W[-1]) and np.all(vel[-1] == 0) and np.all(acc[-1] == 0)  # at rest on the last waypoint


def test_sample_counts_and_paths_without_samples(eng):
    three, lim, grid = three_paths()
    dt = 0.01
    paths = [three[2], three[1], three[2], three[0], three[2], three[2], three[1]]
    counts = [255, 0, 256, 1, 257, 0, 3]  # a path without samples between two with samples, and two block edges of 256
    W, off, prof, full = profile_and_counts(eng, paths, lim, grid, dt)
    assert all(c <= f for c, f in zip(counts, full))
    got = sample_with(eng, W, off, prof, counts, lim, grid, dt)
    for b, c in enumerate(counts):
        assert all(len(a) == c for a in got[b])
        if c:
            Wa, offa, profa, _ = profile_and_counts(eng, [paths[b]], lim, grid, dt)
            want = sample_with(eng, Wa, offa, profa, [c], lim, grid, dt)[0]
            assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(got[b], want)), b
    assert all(a.shape == (0, 3) for a in sample_with(eng, W, off, prof, [0] * len(paths), lim, grid, dt)[0])


def test_statuses(eng):
    three, lim, grid = three_paths()
    alone = [run(eng, [p], lim, grid)[0] for p in three]
    bad = three[2].copy()
    bad[5, 1] = np.nan
    for where in (0, 1, 2):  # the NaN path first, in the middle, last
        paths = [three[1], three[2]]
        paths.insert(where, bad)
        out = run(eng, paths, lim, grid)
        assert out[where][6] == engine.TOPP_NONFINITE and all(np.all(np.isnan(a)) for a in out[where][:6]), where
        good = [o for b, o in enumerate(out) if b != where]
        assert same_bits(good[0], alone[1]) and same_bits(good[1], alone[2]), where
    still = np.tile(three[1][0], (3, 1))
    want = J.profile(still, *lim, grid)
    out = run(eng, [three[1], still, three[2]], lim, grid)
    assert out[1][6] == engine.TOPP_STALLED == want["status"]
    for what, got in zip(NAMES, out[1][:6]):
        assert np.array_equal(got, want[what]), what
    assert same_bits(out[0], alone[1]) and same_bits(out[2], alone[2])
    gen = HipJerkTrajectoryGenerator(0.05, *lim, grid_per_segment=grid, engine=eng, allow_repeated_waypoints=True)
    trajs = gen.generate_trajectories([three[1], still, bad, three[2]])
    assert trajs[1] is None and trajs[2] is None and trajs[0] is not None and trajs[3] is not None
    T = gen.durations([three[1], still, bad])
    assert np.isfinite(T[0]) and np.isnan(T[1]) and np.isnan(T[2])
    with pytest.raises(ValueError):
        HipJerkTrajectoryGenerator(0.05, *lim, engine=eng).generate_trajectory(list(still))  # equal waypoints


def test_sampling_paths_that_are_not_ok_returns(eng):
    three, lim, grid = three_paths()
    bad = three[2].copy()
    bad[1, 0] = np.nan
    paths = [three[2], bad, np.tile(three[1][0], (3, 1)), three[1]]
    W, off, prof, full = profile_and_counts(eng, paths, lim, grid, 0.05)
    assert [int(s) for s in prof[6]] == [engine.TOPP_OK, engine.TOPP_NONFINITE, engine.TOPP_STALLED, engine.TOPP_OK]
    counts = [full[0], 3, 3, full[3]]
    got = sample_with(eng, W, off, prof, counts, lim, grid, 0.05)  # returns MJPL_OK: the binding raises otherwise
    assert all(len(a) == 3 for b in (1, 2) for a in got[b])
    for b in (0, 3):
        Wa, offa, profa, _ = profile_and_counts(eng, [paths[b]], lim, grid, 0.05)
        want = sample_with(eng, Wa, offa, profa, [full[b]], lim, grid, 0.05)[0]
        assert full[b] > 1 and all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(got[b], want)), b


def test_run_to_run_identity(eng):
    three, lim, grid = three_paths()
    paths = three * 3
    first = run(eng, paths, lim, grid)
    for _ in range(2):
        assert all(same_bits(a, b) for a, b in zip(first, run(eng, paths, lim, grid)))


def test_host_and_device_forms_agree(eng):
    paths, lim, grid = three_paths()
    dt = 0.05
    W, off, prof, full = profile_and_counts(eng, paths, lim, grid, dt)
    soff = np.concatenate([[0], np.cumsum(full)]).astype(np.int64)
    pos, vel, acc = eng.jerk_sample(W, off, *prof[:6], dt, soff, *lim, grid=grid)
    M, L, v, vp, tc, t, status = prof
    dW = eng.alloc(W.nbytes).upload(W)
    dM, dL = eng.alloc(M.nbytes), eng.alloc(L.nbytes)
    dv, dvp, dtc, dtt = (eng.alloc(v.nbytes) for _ in range(4))
    dst = eng.alloc(4 * 3)
    dpos, dvel, dacc = (eng.alloc(pos.nbytes) for _ in range(3))
    bufs = (dW, dM, dL, dv, dvp, dtc, dtt, dst, dpos, dvel, dacc)
    try:
        eng.jerk_profile_dev(dW.ptr, off, 3, *lim, grid, dM.ptr, dL.ptr, dv.ptr, dvp.ptr, dtc.ptr, dtt.ptr, dst.ptr)
        eng.jerk_sample_dev(dW.ptr, off, 3, dM.ptr, dL.ptr, dv.ptr, dvp.ptr, dtc.ptr, dtt.ptr, dt, soff, *lim, grid, dpos.ptr, dvel.ptr,
                            dacc.ptr)
        for buf, want in ((dM, M), (dL, L), (dv, v), (dvp, vp), (dtc, tc), (dtt, t), (dpos, pos), (dvel, vel), (dacc, acc)):
            got = buf.download(np.float64, want.size)
            assert np.array_equal(got.view(np.uint64), want.reshape(-1).view(np.uint64))
        assert np.array_equal(dst.download(np.int32, 3), status)
        # the timer runs the same two calls
        mp, ms = eng.time_jerk_dev(dW.ptr, off, 3, dM.ptr, dL.ptr, dv.ptr, dvp.ptr, dtc.ptr, dtt.ptr, dst.ptr, dt, soff, *lim, grid,
                                   dpos.ptr, dvel.ptr, dacc.ptr, 2)
        assert mp.shape == ms.shape == (2,) and np.all(mp > 0) and np.all(ms > 0)
        assert np.array_equal(dpos.download(np.float64, pos.size).view(np.uint64), pos.reshape(-1).view(np.uint64))
    finally:
        for buf in bufs:
            buf.free()


def test_argument_errors(eng):
    W = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]])
    off = np.array([0, 3], np.int64)
    one, lim = np.ones(2), (np.ones(2), np.ones(2), np.ones(2))
    M, L, v, vp, tc, t, status = eng.jerk_profile(W, off, *lim)
    soff = np.array([0, 4], np.int64)

    def code(f, *a, **k):
        with pytest.raises(engine.MjplError) as err:
            f(*a, **k)
        return err.value.code

    ARG, CAP = -1, -4
    assert code(eng.jerk_profile, W, off, *lim, grid=0) == ARG
    assert int(eng.jerk_profile(W, off, *lim, grid=1)[6][0]) == engine.TOPP_OK  # (grid 1 is allowed here)
    assert code(eng.jerk_profile, W, np.array([0, 1, 3], np.int64), *lim) == ARG  # a path of one waypoint
    assert code(eng.jerk_profile, W, np.array([0, 3, 3], np.int64), *lim) == ARG
    for j in range(3):  # a limit of the wrong sign, zero, NaN, infinite
        for bad in (-1.0, 0.0, np.nan, np.inf):
            l = [a.copy() for a in lim]
            l[j][1] = bad
            assert code(eng.jerk_profile, W, off, *l) == ARG, (j, bad)
    W17 = np.zeros((2, 17))
    W17[1] = 1
    assert code(eng.jerk_profile, W17, [0, 2], np.ones(17), np.ones(17), np.ones(17)) == CAP
    for dt in (0.0, -0.1, np.nan):
        assert code(eng.jerk_sample, W, off, M, L, v, vp, tc, t, dt, soff, *lim) == ARG
    # samp_off that falls (two paths)
    W2, off2 = np.concatenate([W, W]), np.array([0, 3, 6], np.int64)
    p2 = eng.jerk_profile(W2, off2, *lim)
    assert code(eng.jerk_sample, W2, off2, *p2[:6], 0.1, np.array([0, 4, 2], np.int64), *lim) == ARG
    # NULL pointers, straight at the ABI
    lib, F64, I64, I32 = eng.lib, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    desc, keep = eng.jerk_desc(2, 2, *lim)
    p = lambda a, T=F64: a.ctypes.data_as(T)
    full = [eng.h, C.byref(desc), p(W), p(off, I64), 1, p(M), p(L), p(v), p(vp), p(tc), p(t), p(status, I32)]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11):
        args = list(full)
        args[k] = None
        assert lib.mjpl_jerk_profile(*args) == ARG, k
        assert lib.mjpl_jerk_profile_dev(*args) == ARG, k
    pos = np.zeros((4, 2))
    full = [eng.h, C.byref(desc), p(W), p(off, I64), 1, p(M), p(L), p(v), p(vp), p(tc), p(t), 0.1, p(soff, I64), p(pos), p(pos), p(pos)]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15):
        args = list(full)
        args[k] = None
        assert lib.mjpl_jerk_sample(*args) == ARG, k
        assert lib.mjpl_jerk_sample_dev(*args) == ARG, k
    null_lim = engine.JerkDesc(2, 2, None, p(one), p(one))
    assert lib.mjpl_jerk_profile(eng.h, C.byref(null_lim), *full[2:4], 1, *full[5:11], p(status, I32)) == ARG
    # nothing to do is not an error
    assert lib.mjpl_jerk_profile(eng.h, C.byref(desc), None, None, 0, None, None, None, None, None, None, None) == 0


def limits_hold_at_the_samples(traj, vlim, alim, jlim):
    vel, acc = np.stack(traj.velocities), np.stack(traj.accelerations)
    jerk = np.diff(np.vstack([np.zeros((1, acc.shape[1])), acc]), axis=0) / traj.dt  # a_{-1} = 0
    print(f"largest velocity / limit {np.max(np.abs(vel) / vlim):.9f}, acceleration {np.max(np.abs(acc) / alim):.9f}, "
          f"finite-difference jerk {np.max(np.abs(jerk) / jlim):.9f}")
    assert np.all(np.abs(vel) <= vlim + 1e-8) and np.all(np.abs(acc) <= alim + 1e-8) and np.all(np.abs(jerk) <= jlim + 1e-8)


def test_reference_trajectory_case(eng):
    # the reference's own generator test: 7 columns, two random waypoints, unit limits, dt 0.002
    rng = np.random.default_rng(5)
    waypoints = [rng.random(7), rng.random(7)]
    gen = HipJerkTrajectoryGenerator(0.002, np.ones(7), np.ones(7), np.ones(7), engine=eng)
    traj = gen.generate_trajectory(waypoints)
    assert traj is not None and traj.dt == 0.002 and np.array_equal(traj.q_init, waypoints[0])
    assert len(traj.positions) == len(traj.velocities) == len(traj.accelerations) == sample_count(gen.durations([waypoints])[0], 0.002)
    limits_hold_at_the_samples(traj, np.ones(7), np.ones(7), np.ones(7))
    np.testing.assert_allclose(traj.positions[-1], waypoints[1], rtol=1e-5, atol=1e-8)
    assert np.abs(traj.velocities[-1]).max() <= 1e-8


def test_limits_hold_at_every_sample_of_a_curved_path(eng):
    _, W, vlim, alim, jlim, _ = CASES[IDS.index("d7-n17-G2")]
    gen = HipJerkTrajectoryGenerator(0.002, vlim, alim, jlim, engine=eng)
    traj = gen.generate_trajectory(list(W))
    assert traj is not None and len(traj.positions) > 1000
    limits_hold_at_the_samples(traj, vlim, alim, jlim)
    np.testing.assert_allclose(traj.positions[-1], W[-1], rtol=1e-5, atol=1e-8)


def test_constrained_trajectory_around_the_wall_corner():
    model = scenes.two_dof_ball()
    collision = CollisionConstraint(model)
    constraints = [JointLimitConstraint(model), collision]
    gen = HipJerkTrajectoryGenerator(0.01, [1.0, 1.0], [2.0, 2.0], [20.0, 20.0], engine=collision.engine)
    # the wall-corner case of tests/test_gpu_trajectory.py: the polyline is free, the spline through it is not
    path = [np.array(p) for p in ((-0.2, 0.63), (0.3, 0.63), (0.9, 0.63), (0.9, 1.5))]
    plain = gen.generate_trajectory(path)
    assert plain is not None and not collision.valid_configs(np.stack(plain.positions)).all()
    traj = generate_constrained_trajectory(path, gen, constraints, max_rounds=32)
    assert traj is not None and len(path) == 4
    P = np.stack(traj.positions)
    assert all(c.valid_configs(P).all() for c in constraints)
    np.testing.assert_allclose(P[-1], path[-1], atol=1e-9)
    limits_hold_at_the_samples(traj, np.array([1.0, 1.0]), np.array([2.0, 2.0]), np.array([20.0, 20.0]))


def test_certified_trajectory_on_the_example_scene():
    mb = ModelBuilder()  # the scene of examples/certified_trajectory.py
    mb.add_body("ball", pos=(0, 0, 1))
    mb.add_joint("ball", "ball_slide_x", "slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("ball", "sphere", (0.01,))
    mb.add_geom("world", "box", (0.001, 0.5, 0.5), pos=(0.9, 0, 1), name="wall")
    cc = CollisionConstraint(mb.compile())
    sweep = dict(cap=0.1, lo=[-2.0], hi=[2.0])
    path = [np.array([x]) for x in (0.0, 0.8, 0.81, 0.0)]
    assert cc.certified_spline(path, **sweep).status == engine.SWEEP_HIT
    gen = HipJerkTrajectoryGenerator(0.01, [1.0], [2.0], [20.0], engine=cc.engine)
    out = generate_certified_trajectory(path, gen, [cc], cc, **sweep)
    assert out is not None
    traj, cert = out
    assert cert.status == engine.SWEEP_FREE and max(float(q[0]) for q in traj.positions) < 0.9
    limits_hold_at_the_samples(traj, np.array([1.0]), np.array([2.0]), np.array([20.0]))
