"""Certified trajectories, the parts that need no GPU: the NumPy statement itself (tests/spline_sweep_reference.py) --
the hull travel encloses the cubic, its closed forms, the wall path, soundness on the models of test_sweep_host against
the CPU distances -- the C ABI of mjpl_sweep_splines*, and the loop of generate_certified_trajectories against fake
generators and certifiers."""
import ctypes
import os
import re

import numpy as np
import pytest

import distance_reference as ref
import spline_sweep_reference as ssr
import sweep_reference as sref
import trajectory_reference as tref
from mjpl_amd import build as _build
from mjpl_amd import engine
from mjpl_amd.constraint.collision_constraint import CertifiedPath
from mjpl_amd.trajectory import (HipToppTrajectoryGenerator, Trajectory, TrajectoryGenerator, generate_certified_trajectories,
                                 generate_certified_trajectory)
from test_gpu_contacts import candidate_table
from test_sweep_host import IDS, MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, HIT, UNDECIDED, NONFINITE, RANGE = sref.FREE, sref.HIT, sref.UNDECIDED, sref.NONFINITE, sref.RANGE


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mjpl_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_build.build_hip())
    for name in ("mjpl_sweep_splines", "mjpl_sweep_splines_dev"):
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(engine.ABI[name][1]) == 12
    from mjpl_amd import ClearanceConstraint, CollisionConstraint
    for cls in (ClearanceConstraint, CollisionConstraint):
        assert hasattr(cls, "certified_spline") and hasattr(cls, "certified_splines")
    assert hasattr(engine.Engine, "sweep_splines") and hasattr(engine.Engine, "sweep_splines_dev")
    assert HipToppTrajectoryGenerator.follows_natural_spline is True


def test_repeated_waypoints_are_an_option_of_the_generator():
    path = [np.array([0.0]), np.array([0.8]), np.array([0.8]), np.array([0.0])]
    with pytest.raises(ValueError):
        HipToppTrajectoryGenerator(0.01, [1.0], [2.0])._pack([path])  # the default refusal stays
    W, off = HipToppTrajectoryGenerator(0.01, [1.0], [2.0], allow_repeated_waypoints=True)._pack([path])
    assert W.shape == (4, 1) and list(off) == [0, 4]
    # the statement parameterises such a path: nothing in it needs distinct waypoints
    assert tref.profile(W, [-1.0], [1.0], [-2.0], [2.0], 8)["status"] == tref.OK


# ---- the statement: nodes
def test_piece_eval_is_spline_eval():
    rng = np.random.default_rng(1)
    W = rng.uniform(-2, 2, (6, 4))
    M = tref.spline_second_derivatives(W)
    for k in range(5):
        for B in (0.0, 0.125, 1 / 3, 0.7, 1.0):
            q, q1, _ = tref.spline_eval(W, M, k, B)
            g, g1 = ssr.piece_eval(W[k][None], W[k + 1][None], M[k][None], M[k + 1][None], np.array([[5.0]]), np.array([[B]]))
            assert g[0].tobytes() == q.tobytes() and g1[0].tobytes() == q1.tobytes()


def all_nodes(depths):
    """(t, h) of the root and of every node of depths 1 .. depths."""
    out = [(0.5, 0.5)]
    for k in range(1, depths + 1):
        h = 2.0 ** -(k + 1)
        out += [((2 * m + 1) * h, h) for m in range(2 ** k)]
    return out


def test_the_box_of_a_node_holds_its_cubic():
    rng = np.random.default_rng(7)
    worst, ratios = 0.0, []
    for _ in range(200):
        n, d = int(rng.integers(2, 9)), int(rng.integers(1, 8))
        W = np.cumsum(rng.uniform(-0.6, 0.6, (n, d)), axis=0) + rng.uniform(-1, 1, d)
        M = tref.spline_second_derivatives(W)
        k = int(rng.integers(0, n - 1))
        nodes = all_nodes(int(rng.integers(0, 5)))
        t, h = np.array([x[0] for x in nodes]), np.array([x[1] for x in nodes])
        rep = lambda a: np.repeat(a[None], len(nodes), axis=0)
        row, HD = ssr.node_box(rep(W[k]), rep(W[k + 1]), rep(M[k]), rep(M[k + 1]), np.full(len(nodes), n - 1.0), t, h)
        u = np.linspace(-1.0, 1.0, 401)
        for j in range(len(nodes)):
            B = np.clip(t[j] + h[j] * u, 0.0, 1.0)[:, None]
            q, _ = ssr.piece_eval(W[k], W[k + 1], M[k], M[k + 1], float(n - 1), B)
            off = np.abs(q - row[j])
            assert np.all(off <= HD[j]), (n, d, k, nodes[j])
            ext = off.max(axis=0)
            ratios += list((HD[j] / ext)[ext > 1e-9])
            worst = max(worst, float(np.max(off - HD[j])))
    print(f"largest |q - row| - HD = {worst:.3e}; HD / true extent: median {np.median(ratios):.9f}, worst {np.max(ratios):.2f}")


def test_two_waypoints_give_the_straight_travel():
    rng = np.random.default_rng(3)
    W = rng.uniform(-2, 2, (2, 5))
    Z = np.zeros((1, 5))
    for t, h in all_nodes(4):
        row, HD = ssr.node_box(W[:1], W[1:], Z, Z, np.array([1.0]), np.array([t]), np.array([h]))
        straight = h * np.abs(W[1] - W[0])
        slop = 2.0 ** -40 * (np.abs(W[0]) + np.abs(W[1]))
        assert np.all(HD[0] >= straight - 4 * np.finfo(float).eps * np.abs(W).sum(axis=0))
        assert np.all(HD[0] <= straight * (1 + 2.0 ** -29) + 2 * slop)
        assert np.all(np.abs(row[0] - (W[0] + t * (W[1] - W[0]))) <= 4 * np.finfo(float).eps * np.abs(W).sum(axis=0))
    row, HD = ssr.node_box(W[:1], W[1:], Z, Z, np.array([1.0]), np.array([0.0]), np.array([0.0]))
    assert np.all(HD == 0.0)


# ---- the statement: the loop, in closed form
WALL_PATH = np.array([[0.0], [0.86], [0.86], [0.0]])


def wall_measure(cap):
    """A ball (r 0.01) on a slide along x and a wall 0.899 .. 0.901: the distance in closed form, lever 1."""
    def measure(Q, HD):
        gap = np.minimum(np.abs(Q[:, 0] - 0.9) - 0.001 - 0.01, cap)
        z = np.zeros(len(Q), np.int32)
        return gap - HD[:, 0], z, gap, z
    return measure


@pytest.mark.parametrize("cap", [0.1, 0.05, 1.0])
def test_wall_path_goes_through_the_wall_between_its_waypoints(cap):
    lo, hi = np.array([-2.0]), np.array([2.0])
    M = tref.spline_second_derivatives(WALL_PATH)
    peak = ssr.piece_samples(WALL_PATH, M, 1, 1001).max()
    assert abs(peak - 0.989) < 1e-3  # the spline passes the wall and comes back
    for a, b in zip(WALL_PATH[:-1], WALL_PATH[1:]):  # ... while every straight segment is at least 0.029 clear
        assert 0.9 - 0.011 - max(a[0], b[0]) >= 0.029 - 1e-12
    got = ssr.sweep_splines(wall_measure(cap), [WALL_PATH], 0.0, 8, lo, hi)
    assert list(got["status"]) == [FREE, HIT, FREE]
    assert got["t_hit"][1] == 0.0625 and got["depth"][1] == 3 and got["pair"][1] == 0
    assert wall_measure(cap)(ssr.piece_samples(WALL_PATH, M, 1, 17)[1:2], np.zeros((1, 1)))[2][0] <= 0
    assert np.all(got["clear_lb"][[0, 2]] > 0) and np.isnan(got["clear_lb"][1])
    assert got["M"].tobytes() == M.tobytes()


def test_wall_path_leaves_the_bounds():
    got = ssr.sweep_splines(wall_measure(0.1), [WALL_PATH], 0.0, 8, np.array([-2.0]), np.array([0.95]))
    assert list(got["status"]) == [FREE, RANGE, FREE]
    assert got["pair"][1] == -2 and np.isfinite(got["t_hit"][1])
    M = tref.spline_second_derivatives(WALL_PATH)
    assert tref.spline_eval(WALL_PATH, M, 1, got["t_hit"][1])[0][0] > 0.95
    # a waypoint outside: not measured
    got = ssr.sweep_splines(wall_measure(0.1), [WALL_PATH], 0.0, 8, np.array([-2.0]), np.array([0.5]))
    assert list(got["status"]) == [RANGE, RANGE, RANGE] and np.isnan(got["t_hit"]).all() and np.all(got["pair"] == -1)
    assert np.all(got["nodes"] == 0)
    # a path that touches a bound is never FREE there: its box leaves the bounds at every depth
    got = ssr.sweep_splines(wall_measure(0.1), [np.array([[0.0], [0.5]])], 0.0, 4, np.array([-2.0]), np.array([0.5]))
    assert list(got["status"]) == [UNDECIDED] and got["depth"][0] == 4


def test_nonfinite_path_and_its_neighbours():
    good = np.array([[0.0], [0.3], [0.5]])
    bad = np.array([[0.0], [np.nan], [0.5], [0.6]])
    alone = ssr.sweep_splines(wall_measure(0.1), [good], 0.0, 8)
    got = ssr.sweep_splines(wall_measure(0.1), [good, bad, good], 0.0, 8)
    assert list(got["status"][2:5]) == [NONFINITE] * 3 and np.all(got["nodes"][2:5] == 0)
    for name in ("status", "t_hit", "clear_lb", "pair", "nodes", "depth"):
        assert got[name][:2].tobytes() == alone[name].tobytes() == got[name][5:].tobytes(), name


# ---- the statement on the models, against the CPU distances
PATHS, DEPTH, SAMPLES = 8, 4, 257


def cpu_measure(m, allowed, qidx, base, lo, hi, cap):
    """(measure, clearance): the bubble measurement of sweep_reference on the CPU distances, and clearance(Q) from them."""
    pairs, flags = candidate_table(m, allowed)
    margins = ref.pair_margins(m, pairs)
    Wt = sref.lever_table(m, pairs, qidx, base, lo, hi)

    def distances(Q):
        F = np.tile(base, (len(Q), 1))
        F[:, qidx] = Q
        return ref.reference_distances(m, F, pairs)

    def measure(Q, HD):
        return sref.bubble(distances(Q), margins, flags, Wt, HD, cap)

    def clearance(Q):
        return measure(Q, np.zeros_like(Q))[2:]

    return measure, clearance


def check_soundness(paths, got, clearance, d_min, cap):
    """FREE pieces keep clearance >= max(d_min, clear_lb - 1e-9) at SAMPLES spline samples; HIT pieces are in contact at
    q(t_hit) with the reported pair.  -> (pieces FREE, pieces HIT)."""
    st, at = got["status"], 0
    rows, want, hits = [], [], []
    for W in paths:
        M = tref.spline_second_derivatives(W) if np.isfinite(W).all() else None
        for k in range(len(W) - 1):
            i = at + k
            if st[i] == FREE:
                rows.append(ssr.piece_samples(W, M, k, SAMPLES))
                want.append(max(d_min, got["clear_lb"][i] - 1e-9))
                assert 0 < got["clear_lb"][i] <= cap
            elif st[i] == HIT:
                t = got["t_hit"][i]
                hits.append((W[k] if t == 0.0 else W[k + 1] if t == 1.0 else tref.spline_eval(W, M, k, t)[0], got["pair"][i]))
        at += len(W) - 1
    if rows:
        clear = clearance(np.concatenate(rows))[0].reshape(len(rows), SAMPLES)
        assert np.all(clear >= np.array(want)[:, None])
    if hits:
        clear, cp = clearance(np.stack([q for q, _ in hits]))
        assert np.all((clear <= 0) | (clear < d_min))
        assert np.array_equal(cp, [p for _, p in hits])
    return len(rows), len(hits)


@pytest.mark.parametrize("name,m,allowed,qidx,base,lo,hi", MODELS, ids=IDS)
def test_free_pieces_are_free_and_hits_are_hits(name, m, allowed, qidx, base, lo, hi):
    d_min = 0.01
    cap = d_min + float(np.max(np.asarray(m.geom_margin, float), initial=0.0)) + 0.25
    measure, clearance = cpu_measure(m, allowed, qidx, base, lo, hi, cap)
    paths = ssr.random_walk_paths(lo, hi, PATHS, seed=5)
    got = ssr.sweep_splines(measure, paths, d_min, DEPTH, lo, hi)
    free, hit = check_soundness(paths, got, clearance, d_min, cap)
    st = got["status"]
    print(f"{name}: {len(st)} pieces, FREE {free}, HIT {hit}, UNDECIDED {int((st == UNDECIDED).sum())}, RANGE "
          f"{int((st == RANGE).sum())}; nodes per piece {got['nodes'].mean():.1f}")
    assert free + hit > 0


# ---- the Python loop
class SplineGenerator(TrajectoryGenerator):
    """Positions: the waypoints after the first (enough for the loop; a generator that declares the spline)."""
    follows_natural_spline = True

    def __init__(self):
        self.calls = 0

    def generate_trajectory(self, waypoints):
        self.calls += 1
        pos = [np.asarray(w, float) for w in waypoints[1:]]
        zero = [np.zeros_like(p) for p in pos]
        return Trajectory(0.1, np.asarray(waypoints[0], float), pos, zero, zero)


class UndeclaredGenerator(SplineGenerator):
    follows_natural_spline = False


class ScriptedCertifier:
    """certified_splines from a rule path -> per-piece statuses; records what it was asked."""

    def __init__(self, rule):
        self.rule, self.asked = rule, []

    def certified_splines(self, paths, **params):
        self.asked.append(([len(p) for p in paths], params))
        out = []
        for p in paths:
            st = np.asarray(self.rule(p), np.int32)
            bad = np.flatnonzero(st != FREE)
            status = FREE if not len(bad) else HIT if (st == HIT).any() else int(st[bad[0]])
            out.append(CertifiedPath(status, int(bad[0]) if len(bad) else -1, float("nan"), None,
                                     0.01 if status == FREE else float("nan"), None, 3 * len(st), st))
        return out


def test_certified_trajectory_inserts_into_the_first_piece_that_is_not_free():
    # pieces longer than 0.55 are UNDECIDED / HIT: [0, 0.4, 1.4, 1.6] needs the midpoint 0.9 in piece 1
    rule = lambda p: [HIT if abs(b[0] - a[0]) > 0.75 else UNDECIDED if abs(b[0] - a[0]) > 0.55 else FREE for a, b in zip(p[:-1], p[1:])]
    wps = [np.array([0.0]), np.array([0.4]), np.array([1.4]), np.array([1.6])]
    before = [w.copy() for w in wps]
    cert, gen = ScriptedCertifier(rule), SplineGenerator()
    traj, c = generate_certified_trajectory(wps, gen, [], cert, cap=0.3)
    assert len(wps) == 4 and all(np.array_equal(a, b) for a, b in zip(wps, before)), "the caller's list is not mutated"
    assert c.status == FREE and gen.calls == 2 and [a[0] for a in cert.asked] == [[4], [5]]
    assert cert.asked[0][1] == dict(cap=0.3)
    assert [float(q[0]) for q in traj.positions] == [0.4, (0.4 + 1.4) / 2, 1.4, 1.6]
    # the FIRST piece that is not FREE gets the waypoint, also when a later one is the HIT
    wps = [np.array([0.0]), np.array([0.6]), np.array([1.6])]
    cert = ScriptedCertifier(rule)
    assert generate_certified_trajectory(wps, SplineGenerator(), [], cert, max_rounds=2) is None
    assert [a[0] for a in cert.asked] == [[3], [4]]
    traj, c = generate_certified_trajectory(wps, SplineGenerator(), [], ScriptedCertifier(rule))
    assert [float(q[0]) for q in traj.positions] == [0.3, 0.6, (0.6 + 1.6) / 2, 1.6] and c.status == FREE


def test_certified_trajectories_rounds_types_and_batches():
    never = ScriptedCertifier(lambda p: [HIT] + [FREE] * (len(p) - 2))
    gen = SplineGenerator()
    wps = [np.array([0.0]), np.array([1.0])]
    assert generate_certified_trajectory(wps, gen, [], never, max_rounds=5) is None
    assert gen.calls == 5 and len(never.asked) == 5 and len(wps) == 2
    with pytest.raises(TypeError):
        generate_certified_trajectory(wps, UndeclaredGenerator(), [], never)
    with pytest.raises(ValueError):
        generate_certified_trajectory(wps, gen, [], never, max_rounds=None)
    with pytest.raises(ValueError):
        generate_certified_trajectory(wps, gen, [], never, max_rounds=float("inf"))
    # a batch: every open path of a round in ONE certifier call; a finished path is not asked about again
    rule = lambda p: [UNDECIDED if abs(b[0] - a[0]) > 0.55 else FREE for a, b in zip(p[:-1], p[1:])]
    cert = ScriptedCertifier(rule)
    paths = [[np.array([0.0]), np.array([0.4])], [np.array([0.0]), np.array([0.9])], [np.array([0.0]), np.array([1.9])]]
    out = generate_certified_trajectories(paths, SplineGenerator(), [], cert)
    assert [a[0] for a in cert.asked] == [[2, 2, 2], [3, 3], [4], [5]]
    assert [len(tr.positions) for tr, _ in out] == [1, 2, 4] and all(c.status == FREE for _, c in out)
    assert [len(p) for p in paths] == [2, 2, 2]
    assert generate_certified_trajectories([], SplineGenerator(), [], cert) == []
    # a path that is not finite ends at once
    nf = ScriptedCertifier(lambda p: [NONFINITE] * (len(p) - 1))
    gen = SplineGenerator()
    assert generate_certified_trajectory(wps, gen, [], nf) is None and gen.calls == 1
