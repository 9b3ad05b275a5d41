"""Jerk-limited trajectories, the parts that need no GPU: the C ABI of mjpl_jerk_* (declared in include/mjpl_hip.h,
exported by the library, bound by mjpl_amd.engine) and the NumPy statement tests/jerk_reference.py -- closed forms, the
guarantee on a dense sweep of every phase, the consistency of the phases, the spline, float64 against longdouble."""
import ctypes
import os
import re

import numpy as np
import pytest

import jerk_reference as J
import trajectory_reference as R
from mjpl_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_jerk_profile", "mjpl_jerk_profile_dev", "mjpl_jerk_sample", "mjpl_jerk_sample_dev", "mjpl_time_jerk_dev")
CASES = J.parity_cases()
IDS = [c[0] for c in CASES]


def test_abi_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine.ABI, f"{name} is not bound"
    assert "mjpl_jerk_desc" in text
    assert len(engine.ABI["mjpl_jerk_profile"][1]) == len(engine.ABI["mjpl_jerk_profile_dev"][1]) == 12
    assert len(engine.ABI["mjpl_jerk_sample"][1]) == len(engine.ABI["mjpl_jerk_sample_dev"][1]) == 16
    assert len(engine.ABI["mjpl_time_jerk_dev"][1]) == 20
    assert engine.ABI["mjpl_jerk_profile"][1][1] == ctypes.POINTER(engine.JerkDesc)
    assert [f for f, _ in engine.JerkDesc._fields_] == ["nq", "grid", "vlim", "alim", "jlim"]
    for method in ("jerk_profile", "jerk_profile_dev", "jerk_sample", "jerk_sample_dev"):
        assert callable(getattr(engine.Engine, method))


def test_the_class_is_exported_and_validates_like_topp():
    import mjpl_amd
    from mjpl_amd.trajectory import HipJerkTrajectoryGenerator
    assert mjpl_amd.HipJerkTrajectoryGenerator is HipJerkTrajectoryGenerator
    assert "HipJerkTrajectoryGenerator" in mjpl_amd.__all__ and "HipJerkTrajectoryGenerator" in mjpl_amd.trajectory.__all__
    assert HipJerkTrajectoryGenerator.follows_natural_spline is True
    one = np.ones(3)
    gen = HipJerkTrajectoryGenerator(0.01, one, 2 * one, 5 * one, min_velocity=-0.5 * one, min_acceleration=-3 * one)
    assert gen.grid == 2 and np.array_equal(gen.vlim, 0.5 * one) and np.array_equal(gen.alim, 2 * one)  # min(max, -min)
    for bad in (dict(dt=0.0), dict(grid_per_segment=0), dict(max_jerk=[1.0, 0.0, 1.0]), dict(max_jerk=[1.0, 1.0]),
                dict(min_velocity=[0.1, -1, -1]), dict(max_acceleration=[1.0, -1.0, 1.0])):
        kw = dict(dt=0.01, max_velocity=one, max_acceleration=one, max_jerk=one)
        kw.update(bad)
        with pytest.raises(ValueError):
            HipJerkTrajectoryGenerator(**kw)
    # the checks that come before the engine is touched
    with pytest.raises(ValueError):
        gen.generate_trajectory([np.zeros(3)])
    with pytest.raises(ValueError):
        gen.generate_trajectory([np.zeros(3), np.zeros(3), np.ones(3)])
    with pytest.raises(ValueError):
        gen.generate_trajectory([np.zeros(2), np.ones(2)])
    assert gen.generate_trajectories([]) == []


@pytest.mark.parametrize("goal, v, G, T", [(1.0, 1.0, 1, 32.0 ** (1 / 3)), (1.0, 1.0, 2, 32.0 ** (1 / 3)), (10.0, 1.0, 1, 12.0),
                                           (10.0, 1.0, 2, 12.0), (1.0, 0.5, 1, 2 + np.sqrt(2)), (1.0, 0.5, 2, 2 + np.sqrt(2))])
def test_closed_forms(goal, v, G, T):
    one = np.ones(1)
    p = J.profile(np.array([[0.0], [goal]]), v * one, one, one, G)
    assert p["status"] == J.OK
    assert abs(p["t"][-1] - T) <= 1e-12 * T
    assert p["v"][0] == 0 and p["v"][-1] == 0 and p["t"][0] == 0


def test_cube_root():
    for x in (5e-324, 1e-300, 0.3, 1.0, 8.0, 27.0, 1e10, 1e308):
        y = J.cbrt(np.float64(x))
        assert abs(y - np.cbrt(x)) <= 4 * np.spacing(np.cbrt(x)), x
        assert abs(float(J.cbrt(np.longdouble(x))) - np.cbrt(x)) <= 4 * np.spacing(np.cbrt(x)), x
    assert J.cbrt(np.float64(0.0)) == 0 and J.cbrt(np.float64(np.inf)) == np.inf and np.isnan(J.cbrt(np.float64(np.nan)))


def test_section_search():
    h = np.float64(2.0)
    f = lambda x: x * x
    assert J.section_search(f, np.float64(0), np.float64(1.0), h) == 1.0  # feasible at the upper end
    x = J.section_search(f, np.float64(0), np.float64(3.0), h)
    assert f(x) <= h and np.sqrt(2) - x <= 1e-14  # on the feasible side, and as close as the format allows
    assert J.section_search(lambda x: x + np.nan, np.float64(0.5), np.float64(3.0), h) == 0.5  # NaN is infeasible


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_guarantee_and_consistency(k):
    """Velocity, acceleration and the analytic jerk at 20 points of every phase of every interval stay within limit
    (1 + 1e-9); every interval's phases end at (D, v_{i+1}, 0) to 1e-12 of D / of the largest speed."""
    _, W, vlim, alim, jlim, G = CASES[k]
    p = J.shared_profile("parity", k)
    assert p["status"] == J.OK
    N = len(p["v"]) - 1
    assert N == (len(W) - 1) * G
    D, top = 1.0 / N, p["vp"].max()
    worst = np.zeros(3)
    for i in range(N):
        assert np.isfinite(p["lim"][i]).all() and (p["lim"][i] > 0).all()
        assert p["v"][i] <= min(p["lim"][max(i - 1, 0), 0], p["lim"][i, 0]) and max(p["v"][i], p["v"][i + 1]) <= p["vp"][i] <= p["lim"][i, 0]
        assert p["tc"][i] >= 0
        state, start = (np.float64(0), p["v"][i], np.float64(0)), np.float64(0)
        for h, jk in J.interval_phases(p, i):
            assert h >= -1e-15
            for f in np.linspace(0, 1, 20):
                tau = start + f * h
                vel, acc, jerk = J.joint_derivatives(W, p, i, tau)
                worst = np.maximum(worst, [np.max(np.abs(vel) / vlim), np.max(np.abs(acc) / alim), np.max(np.abs(jerk) / jlim)])
            state, start = J.advance(state, h, jk), start + h
        assert abs(state[0] - D) <= 1e-12 * D and abs(state[1] - p["v"][i + 1]) <= 1e-12 * top and abs(state[2]) <= 1e-12 * p["lim"][i, 1]
        assert abs(start - (p["t"][i + 1] - p["t"][i])) <= 1e-12 * p["t"][-1]
    print(f"{IDS[k]}: worst ratios velocity {worst[0]:.12f}, acceleration {worst[1]:.12f}, jerk {worst[2]:.12f}")
    assert np.all(worst <= 1 + 1e-9)
    assert worst.max() > 0.3  # (the sweep looked at a path that moves)


def test_cases_are_what_their_names_say():
    by = {c[0]: c for c in CASES}
    assert {c[1].shape[1] for c in CASES} >= {1, 3, 7, 16} and {len(c[1]) for c in CASES} >= {2, 3, 17} and {c[5] for c in CASES} >= {1, 2, 4}
    W = by["still-column"][1]
    assert np.all(W[:, -1] == W[0, -1]) and not np.all(W[:, 0] == W[0, 0])
    W = by["repeat"][1]
    assert np.any(np.all(W[1:] == W[:-1], axis=1))
    assert {(len(c[1]) - 1) * c[5] for c in J.edge_cases()} == {63, 64, 65, 129}


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_span_is_the_topp_spline(k):
    _, W, *_ = CASES[k]
    M = J.shared_profile("parity", k)["M"]
    assert np.array_equal(M.view(np.uint64), R.spline_second_derivatives(W).view(np.uint64))


def test_float64_against_longdouble():
    """The durations of the float64 and the longdouble statement agree to 1e-10 on the parity cases (a case that does not
    would be dropped from the GPU parity list; at most one in ten may be: none is)."""
    worst = 0.0
    for k in range(len(CASES)):
        T, Tl = J.shared_profile("parity", k)["t"][-1], J.shared_profile("parity", k, np.longdouble)["t"][-1]
        worst = max(worst, abs(float(Tl) - T) / T)
        assert abs(float(Tl) - T) <= 1e-10 * T, IDS[k]
    print(f"float64 against longdouble: worst relative difference of a duration {worst:.3e}")


def test_statuses_of_the_statement():
    one = np.ones(2)
    still = J.profile(np.array([[0.3, 0.4]] * 3), one, one, one, 2)
    assert still["status"] == J.STALLED and np.all(still["v"] == 0) and still["t"][-1] == np.inf and still["t"][0] == 0
    bad = J.profile(np.array([[0.0, 0.0], [np.nan, 1.0], [1.0, 2.0]]), one, one, one, 2)
    assert bad["status"] == J.NONFINITE and all(np.all(np.isnan(bad[k])) for k in ("M", "lim", "v", "vp", "tc", "t"))


def test_samples_of_the_statement():
    k = IDS.index("d3-n17-G1")
    _, W, vlim, alim, jlim, G = CASES[k]
    p = J.shared_profile("parity", k)
    dt = 0.01
    pos, vel, acc = J.sample(W, p, dt)
    assert len(pos) == R.sample_count(p["t"][-1], dt) > 100
    assert np.array_equal(pos[-1], W[-1]) and np.all(vel[-1] == 0) and np.all(acc[-1] == 0)
    assert np.all(np.abs(vel) <= vlim * (1 + 1e-9)) and np.all(np.abs(acc) <= alim * (1 + 1e-9))
    jerk = np.diff(np.vstack([np.zeros((1, 3)), acc]), axis=0) / dt  # the mean of the jerk over a step
    assert np.all(np.abs(jerk) <= jlim + 1e-8)
    M = p["M"]
    curve = np.array([R.spline_at(W, M, s)[0] for s in np.linspace(0, 1, 4001)])
    # every position lies on the spline: no farther from the nearest of the 4001 curve points than half their largest
    # spacing (and the sag of the curve between two of them, below 1e-5 here), in the 1-norm
    spacing = np.abs(np.diff(curve, axis=0)).sum(axis=1).max()
    assert max(np.abs(curve - q).sum(axis=1).min() for q in pos[::37]) <= 0.5 * spacing + 1e-5
