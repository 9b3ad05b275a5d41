"""NumPy statement of the certified trajectories (include/mjpl_hip.h: mjpl_sweep_splines*), independent
of the library: the nodes of a spline piece -- row and Bezier-hull travel, one IEEE operation per line of arithmetic, in
the order the kernels of mjpl_amd/csrc/mjpl_sweep.h use -- and the breadth-first loop over a measurement callback, the
rule of sweep_reference.sweep_edges with the two bound tests a curve that can leave [lo, hi] needs.

A path of n waypoints W has the second derivatives M of trajectory_reference.spline_second_derivatives and n - 1 pieces;
piece k is q_k(B) = trajectory_reference.spline_eval(W, M, k, B)[0], B in [0, 1], with r = n - 1."""
import numpy as np

import trajectory_reference as tref
from sweep_reference import FREE, HIT, NONFINITE, RANGE, SWEEP_SLACK, UNDECIDED

HULL_REL = 1.0 + 2.0 ** -30  # the inflation of a hull travel: relative ...
HULL_ABS = 2.0 ** -40        # ... and per unit of the piece's coefficients
PAIR_RANGE = -2              # the pair of a piece whose row left the bounds


def piece_eval(W0, W1, M0, M1, r, B):
    """(q, q') of tref.spline_eval, for arrays of pieces: W0 .. M1 [n, d], r and B [n, 1] (or scalars)."""
    A = 1.0 - B
    q = (A * W0 + B * W1) + ((A * A * A - A) * M0 + (B * B * B - B) * M1) / (6.0 * r * r)
    q1 = (W1 - W0) * r + ((3.0 * B * B - 1.0) * M1 - (3.0 * A * A - 1.0) * M0) / (6.0 * r)
    return q, q1


def node_box(W0, W1, M0, M1, r, t, h):
    """(row, HD) of the nodes (t, h) [n] of the pieces W0 .. M1 [n, d], r [n]: row = q(t); HD holds the cubic on
    [a, b] = [t - h, t + h] in row +- HD -- the largest distance of a Bezier control point of that span from the row,
    inflated for the rounding of the control points.  HD = 0 where h = 0."""
    r, t, h = (np.asarray(v, float)[:, None] for v in (r, t, h))
    a, b = t - h, t + h
    row, _ = piece_eval(W0, W1, M0, M1, r, t)
    P0, d0 = piece_eval(W0, W1, M0, M1, r, a)
    P3, d3 = piece_eval(W0, W1, M0, M1, r, b)
    w = (b - a) / 3.0
    P1 = P0 + w * (d0 / r)
    P2 = P3 - w * (d3 / r)
    far = np.maximum(np.maximum(np.maximum(np.abs(P0 - row), np.abs(P1 - row)), np.abs(P2 - row)), np.abs(P3 - row))
    HD = far * HULL_REL + HULL_ABS * ((np.abs(W0) + np.abs(W1)) + (np.abs(M0) + np.abs(M1)) / (6.0 * r * r))
    return row, np.where(h == 0.0, 0.0, HD)


def pack(paths):
    """(W [rows, d], wp_off int64 [B + 1]) of a list of [n_b, d] waypoint arrays."""
    paths = [np.asarray(p, float) for p in paths]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.concatenate(paths), off


def sweep_splines(measure, paths, d_min, max_depth, lo=None, hi=None):
    """The loop.  paths: a list of [n_b, d] arrays; measure(Q [n, d], HD [n, d]) -> (slack, slack_pair, gap, gap_pair).
    Returns a dict of status, t_hit, clear_lb, pair, nodes, depth per PIECE (piece k of path b at wp_off[b] - b + k), M
    [rows, d], and `margin`: the least decision margin met at the piece's nodes -- |slack - d_min - 1e-9|, |gap - d_min|,
    |gap|, and for the nodes that are not end points (an end point's row is the waypoint, tested as given) |row - bound|
    and |row -+ HD - bound| per column and finite bound -- inf for a piece that is not measured."""
    paths = [np.asarray(p, float) for p in paths]
    d = paths[0].shape[1]
    lo = np.full(d, -np.inf) if lo is None else np.asarray(lo, float)
    hi = np.full(d, np.inf) if hi is None else np.asarray(hi, float)
    W0, W1, M0, M1, R, Ms, ok = [], [], [], [], [], [], []
    for W in paths:
        n = len(W)
        fin = bool(np.isfinite(W).all())
        with np.errstate(invalid="ignore", over="ignore"):
            M = tref.spline_second_derivatives(W)
        fin = fin and bool(np.isfinite(M).all())
        Ms.append(M)
        W0.append(W[:-1]); W1.append(W[1:]); M0.append(M[:-1]); M1.append(M[1:])
        R.append(np.full(n - 1, float(n - 1)))
        ok.append(np.full(n - 1, fin))
    W0, W1, M0, M1, R, finite = (np.concatenate(v) for v in (W0, W1, M0, M1, R, ok))
    E = len(R)
    status = np.zeros(E, np.int32)
    t_hit, clear_lb = np.full(E, np.nan), np.full(E, np.inf)
    pair, nodes, depth = np.full(E, -1, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    margin = np.full(E, np.inf)
    with np.errstate(invalid="ignore"):
        inside = ((W0 >= lo) & (W0 <= hi) & (W1 >= lo) & (W1 <= hi)).all(axis=1)
    status[~finite] = NONFINITE
    status[finite & ~inside] = RANGE
    live = np.flatnonzero(finite & inside)
    undecided, hit = np.zeros(E, bool), np.zeros(E, bool)
    edge = np.repeat(live, 3)
    t = np.tile([0.0, 0.5, 1.0], len(live))
    h = np.tile([0.0, 0.5, 0.0], len(live))
    for k in range(max_depth + 1):
        if len(edge) == 0:
            break
        rows, HD = node_box(W0[edge], W1[edge], M0[edge], M1[edge], R[edge], t, h)
        end = h == 0.0
        if k == 0:  # the end points are the waypoints themselves
            rows[t == 0.0] = W0[edge[t == 0.0]]
            rows[t == 1.0] = W1[edge[t == 1.0]]
        slack, _sp, gap, gp = measure(rows, HD)
        np.add.at(nodes, edge, 1)
        depth[edge] = k
        outside = ~((rows >= lo) & (rows <= hi)).all(axis=1)
        box_out = ((rows - HD < lo) | (rows + HD > hi)).any(axis=1)
        with np.errstate(invalid="ignore"):
            mb = np.minimum(np.minimum(np.abs(rows - lo), np.abs(rows - hi)),
                            np.minimum(np.abs(rows - HD - lo), np.abs(rows + HD - hi))).min(axis=1)
        mb = np.where(end, np.inf, mb)
        mc = np.minimum(np.abs(slack - d_min - SWEEP_SLACK), np.minimum(np.abs(gap - d_min), np.abs(gap)))
        np.minimum.at(margin, edge, np.minimum(mb, np.where(outside, np.inf, mc)))  # (contact is not looked at outside)
        is_hit = outside | (gap <= 0) | (gap < d_min)
        cert = ~is_hit & ~box_out & (slack - d_min >= SWEEP_SLACK)
        rest = ~is_hit & ~cert
        stuck = rest & (end | (k == max_depth))
        split = rest & ~stuck
        for j in np.flatnonzero(is_hit):  # the least t of this depth
            e = edge[j]
            if not hit[e] or t[j] < t_hit[e]:
                hit[e], t_hit[e], pair[e] = True, t[j], PAIR_RANGE if outside[j] else gp[j]
        np.minimum.at(clear_lb, edge[cert], slack[cert])
        undecided[edge[stuck]] = True
        go = split & ~hit[edge]  # a piece hit in this round opens no further nodes
        e2, t2, h2 = edge[go], t[go], h[go] / 2
        edge = np.concatenate([e2, e2])
        t = np.concatenate([t2 - h2, t2 + h2])
        h = np.concatenate([h2, h2])
    measured = finite & inside
    left = measured & hit & (pair == PAIR_RANGE)
    status[measured & hit] = HIT
    status[left] = RANGE
    status[measured & ~hit & undecided] = UNDECIDED
    clear_lb[status != FREE] = np.nan
    t_hit[~(measured & hit)] = np.nan
    pair[~(measured & hit)] = -1
    return dict(status=status, t_hit=t_hit, clear_lb=clear_lb, pair=pair, nodes=nodes, depth=depth, margin=margin,
                M=np.concatenate(Ms))


WALK_LENGTHS = (2, 3, 5, 9)


def random_walk_paths(lo, hi, count, seed, lengths=WALK_LENGTHS):
    """`count` paths with n cycling through `lengths`: a start in the middle 80 % of [lo, hi], then steps of length
    0.05 .. 0.6 in a random direction, clipped to the bounds.  The step is in units of the widest column: column c moves
    by its share (hi_c - lo_c) / max(hi - lo) of it, so that a narrow column (a finger slide of 0.04) is not clipped at
    every step -- a piece that touches a bound is decided within rounding of the bound tests and is left out of the
    comparisons with the kernels (`margin`)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    scale = (hi - lo) / np.max(hi - lo)
    paths = []
    for b in range(count):
        q = lo + rng.uniform(0.1, 0.9, size=len(lo)) * (hi - lo)
        rows = [q]
        for _ in range(lengths[b % len(lengths)] - 1):
            d = rng.normal(size=len(lo))
            q = np.clip(q + rng.uniform(0.05, 0.6) * scale * d / np.linalg.norm(d), lo, hi)
            rows.append(q)
        paths.append(np.array(rows))
    return paths


def piece_samples(W, M, k, count):
    """q_k(B) at `count` evenly spaced B in [0, 1] -> [count, d] (tref.spline_eval itself)."""
    return np.stack([tref.spline_eval(W, M, k, B)[0] for B in np.linspace(0.0, 1.0, count)])
