"""Inputs shared by tests/test_roadmap_host.py and tests/test_gpu_roadmap.py, and checks both apply."""
import numpy as np

import roadmap_reference as ref
from plan_reference import d2

# ---- the headline scene's planning columns (plan_cases.franka_planning())
FRANKA_N, FRANKA_B, FRANKA_STEP = 193, 37, 0.05
# (k, radius): at every pair some nodes have fewer than k neighbours in range and some have more (test_roadmap_host.py)
FRANKA_BUILDS = ((1, 2.0), (5, 3.0), (32, 3.5))
FRANKA_RADIUS_MAX = 3.5
# rows of the nodes: two in collision, one NaN, an exact duplicate (of DUP_OF), one 2^-30 radius from another (NEAR_OF)
ROW_INVALID, ROW_NAN, ROW_DUP, DUP_OF, ROW_NEAR, NEAR_OF = (20, 100), 40, 77, 12, 150, 31
# problems: q_goal == q_init, a NaN, an end in collision, an end farther than every radius from every node
PROB_SAME, PROB_NAN, PROB_INVALID, PROB_FAR = 5, 9, 14, 21


def franka_inputs(lo, hi, valid_configs):
    """(nodes [193, d], QI, QG [37, d]) from ONE seeded uniform stream in [lo, hi], split by valid_configs ([N, d] ->
    bool [N]): the free draws are the nodes and then the ends, the first draws in collision are planted as above."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    d = len(lo)
    rng = np.random.default_rng(5)
    cand = rng.uniform(lo, hi, size=(1024, d))
    corners = lo + (hi - lo) * rng.choice([0.03, 0.97], size=(512, d))
    ok = np.asarray(valid_configs(np.concatenate([cand, corners])), dtype=bool)
    free, bad, far = cand[ok[:1024]], cand[~ok[:1024]], corners[ok[1024:]]
    assert len(free) >= FRANKA_N + 2 * FRANKA_B and len(bad) >= 3
    nodes = free[:FRANKA_N].copy()
    nodes[ROW_INVALID[0]], nodes[ROW_INVALID[1]] = bad[0], bad[1]
    nodes[ROW_NAN, 2] = np.nan
    nodes[ROW_DUP] = nodes[DUP_OF]
    nodes[ROW_NEAR] = nodes[NEAR_OF]
    nodes[ROW_NEAR, 0] += 2.0 ** -30 * FRANKA_BUILDS[1][1]
    ends = free[FRANKA_N:FRANKA_N + 2 * FRANKA_B]
    QI, QG = ends[:FRANKA_B].copy(), ends[FRANKA_B:].copy()
    QG[PROB_SAME] = QI[PROB_SAME]
    QI[PROB_NAN, 3] = np.nan
    QG[PROB_INVALID] = bad[2]
    with np.errstate(invalid="ignore"):
        reach = np.array([np.nanmin(np.sqrt(d2(nodes, q))) for q in far])
    assert (reach > FRANKA_RADIUS_MAX).any(), reach.max()
    QI[PROB_FAR] = far[np.flatnonzero(reach > FRANKA_RADIUS_MAX)[0]]
    return nodes, QI, QG


# ---- scenes.two_dof_ball(): ball r = 0.1, wall x in [0.5, 0.7], |y| <= 0.5.  Two 12 x 12 grids whose coordinates are
# multiples of 2^-4, so that d2 ties exactly.  "split": |y| <= 0.34375, the wall cuts it into two components.  "around":
# spacing 0.125, symmetric in y, the top and the bottom row pass the wall's ends -- the two ways round tie exactly.
BALL_STEP = 0.02
BALL_GRIDS = {"split": dict(x0=0.25, y0=-0.34375, s=0.0625, radius=0.09), "around": dict(x0=-0.25, y0=-0.6875, s=0.125, radius=0.18)}


def ball_grid(name):
    """(nodes [144, 2] in row-major (x, y) order, radius: between sqrt(2) and 2 spacings, so 8 neighbours in range)."""
    g = BALL_GRIDS[name]
    x, y = g["x0"] + g["s"] * np.arange(12), g["y0"] + g["s"] * np.arange(12)
    return np.stack(np.meshgrid(x, y, indexing="ij"), axis=-1).reshape(144, 2), g["radius"]


def ball_queries(name):
    """(QI, QG): across the wall, inside one side (the direct edge), across with the ends on the axis of symmetry, a
    start inside the wall."""
    if name == "split":
        pairs = (((0.28, 0.0), (0.9, 0.1)), ((0.26, -0.3), (0.37, 0.3)), ((0.3, 0.0), (0.9, 0.0)), ((0.6, 0.0), (0.9, 0.0)),
                 ((0.85, -0.2), (0.3, 0.2)))
    else:
        pairs = (((0.3, 0.01), (0.9, 0.02)), ((-0.2, -0.3), (0.2, 0.6)), ((0.25, 0.0), (1.0, 0.0)), ((0.6, 0.0), (0.9, 0.0)),
                 ((1.1, -0.5), (-0.2, 0.5)), ((0.375, 0.0625), (0.875, 0.0625)))
    return np.array([p[0] for p in pairs], float), np.array([p[1] for p in pairs], float)


def check_graph(Q, g, k):
    """The CSR is symmetric, its rows ascend, hold no self loop and no invalid node, and w is the edges' length."""
    N = len(Q)
    row_off, adj, w = g["row_off"], g["adj"], g["w"]
    assert row_off[0] == 0 and (np.diff(row_off) >= 0).all() and len(adj) == len(w) == 2 * N * k
    m = int(row_off[N])
    assert (adj[m:] == -1).all() and not w[m:].any()
    src = np.repeat(np.arange(N), np.diff(row_off))
    dst = adj[:m]
    assert ((dst >= 0) & (dst < N) & (dst != src)).all()
    assert g["node_valid"][src].all() and g["node_valid"][dst].all()
    for v in range(N):
        assert (np.diff(adj[row_off[v]:row_off[v + 1]]) > 0).all(), v
    fwd = dict(zip(zip(src.tolist(), dst.tolist()), w[:m].view(np.uint64).tolist()))
    assert len(fwd) == m
    for (a, b), bits in fwd.items():
        assert fwd[(b, a)] == bits, (a, b)
    assert np.array_equal(w[:m].view(np.uint64), np.sqrt(d2(Q[src], Q[dst])).view(np.uint64))
    r2 = np.float64(g["radius"]) ** 2 if "radius" in g else None
    if r2 is not None:
        dd = d2(Q[src], Q[dst])
        assert ((dd <= r2) & (dd >= r2 * 2.0 ** -40)).all()


def check_paths(Q, QI, QG, res, valid_edges):
    """Every SOLVED path begins and ends bit-equal to its ends, runs over rows of Q, passes valid_edges, and its cost is the
    left-to-right sum along it; every other problem has no rows."""
    rows = {q.tobytes() for q in Q}
    for b in range(len(QI)):
        n = int(res["n_out"][b])
        if res["status"][b] != ref.SOLVED:
            assert n == 0 and not res["P"][b].any() and res["cost"][b] == 0.0, b
            continue
        P = res["P"][b, :n]
        assert n >= 2 and not res["P"][b, n:].any(), b
        assert P[0].tobytes() == QI[b].tobytes() and P[-1].tobytes() == QG[b].tobytes(), b
        assert all(p.tobytes() in rows for p in P[1:-1]), b
        assert np.asarray(valid_edges(P[:-1], P[1:]), dtype=bool).all(), b
        total = np.float64(0.0)
        for seg in np.sqrt(d2(P[:-1], P[1:])):
            total = total + seg
        assert total.tobytes() == np.float64(res["cost"][b]).tobytes(), (b, total, res["cost"][b])
