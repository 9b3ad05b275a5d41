"""NumPy statement of the certified edge checks (include/mjpl_hip.h: mjpl_sweep_*), independent of
the library: the pair lever table from the model's arrays, the bubble measurement over given pair distances, and the
breadth-first bisection loop over a measurement callback."""
import numpy as np

JT_SLIDE, JT_HINGE = 2, 3
FREE, HIT, UNDECIDED, NONFINITE, RANGE = 0, 1, 2, 3, 4
SWEEP_SLACK = 1e-9


def _norm(v):
    return float(np.sqrt(np.sum(np.asarray(v, float) ** 2)))


def geom_levers(model, qidx, qpos_base, lo=None, hi=None):
    """rho [ngeom, nplan]: the lever of planning column c for geom g (0: c is not above g).  Walks from the geom up
    to the column's joint: |geom_pos|, then per body the joints below the column's in reverse order (hinge: 2 |jnt_pos|,
    slide: its travel), the body offset, ... and |jnt_pos| of the column's own hinge, plus rbound.  A planning slide
    above g: 1."""
    qidx = np.arange(model.nq) if qidx is None else np.asarray(qidx)
    base = np.asarray(model.qpos0 if qpos_base is None else qpos_base, float)
    nplan = len(qidx)
    lo = np.full(nplan, -np.inf) if lo is None else np.asarray(lo, float)
    hi = np.full(nplan, np.inf) if hi is None else np.asarray(hi, float)
    col_of = {int(a): c for c, a in enumerate(qidx)}
    parent = np.asarray(model.body_parentid)
    jadr, jnum = np.asarray(model.body_jntadr), np.asarray(model.body_jntnum)
    jtype, jq = np.asarray(model.jnt_type), np.asarray(model.jnt_qposadr)
    jpos = np.asarray(model.jnt_pos, float).reshape(-1, 3)
    bpos = np.asarray(model.body_pos, float).reshape(-1, 3)
    gpos = np.asarray(model.geom_pos, float).reshape(-1, 3)
    q0 = np.asarray(model.qpos0, float)
    rho = np.zeros((model.ngeom, nplan))
    for g in range(model.ngeom):
        stretch = _norm(gpos[g])
        b = int(model.geom_bodyid[g])
        while b > 0:
            for j in range(jadr[b] + jnum[b] - 1, jadr[b] - 1, -1):
                c = col_of.get(int(jq[j]), -1)
                if jtype[j] == JT_SLIDE:
                    if c >= 0:
                        rho[g, c] = 1.0
                        travel = max(abs(lo[c] - q0[jq[j]]), abs(hi[c] - q0[jq[j]]))
                    else:
                        travel = abs(base[jq[j]] - q0[jq[j]])
                    stretch += travel
                else:
                    if c >= 0:
                        rho[g, c] = stretch + _norm(jpos[j]) + float(model.geom_rbound[g])
                    stretch += 2.0 * _norm(jpos[j])
            stretch += _norm(bpos[b])
            b = int(parent[b])
    return rho


def lever_table(model, pairs, qidx=None, qpos_base=None, lo=None, hi=None):
    """W [P, nplan]: rho_c of the one geom of the pair that column c moves; 0 when it moves both or neither."""
    rho = geom_levers(model, qidx, qpos_base, lo, hi)
    pairs = np.asarray(pairs).reshape(-1, 2)
    r1, r2 = rho[pairs[:, 0]], rho[pairs[:, 1]]
    a1, a2 = r1 != 0, r2 != 0
    return np.where(a1 & ~a2, r1, np.where(a2 & ~a1, r2, 0.0))


def bubble(D, margins, allowed, W, HD, cap):
    """(slack, slack_pair, gap, gap_pair) from pair distances D [N, P]: D_p = min(D, cap), B_p = sum_c HD[c] W[p, c] in
    ascending c with zero factors skipped; minima over the non-allowed pairs, lowest index on ties."""
    D = np.minimum(np.asarray(D, float), cap)
    n = D.shape[0]
    keep = np.flatnonzero(~np.asarray(allowed, bool))
    if len(keep) == 0:
        return np.full(n, float(cap)), np.full(n, -1, np.int32), np.full(n, float(cap)), np.full(n, -1, np.int32)
    V = D[:, keep] - margins[keep]
    B = np.zeros_like(V)
    for c in range(W.shape[1]):
        w = W[keep, c][None, :]
        hd = HD[:, c][:, None]
        on = (w != 0) & (hd != 0)
        B = np.where(on, B + np.where(on, hd, 0.0) * np.where(on, w, 0.0), B)
    S = V - B
    ag, as_ = np.argmin(V, axis=1), np.argmin(S, axis=1)
    r = np.arange(n)
    return S[r, as_], keep[as_].astype(np.int32), V[r, ag], keep[ag].astype(np.int32)


def sweep_edges(measure, QA, QB, d_min, max_depth, lo=None, hi=None):
    """The loop.  measure(Q [n, nplan], HD [n, nplan]) -> (slack, slack_pair, gap, gap_pair).  Returns a dict of status,
    t_hit, clear_lb, pair, nodes, depth per edge and `margin`: the least decision margin met at the edge's nodes
    (|slack - d_min - 1e-9|, |gap - d_min|, |gap|), inf for an edge that is not measured."""
    QA, QB = np.asarray(QA, float), np.asarray(QB, float)
    E, nplan = QA.shape
    lo = np.full(nplan, -np.inf) if lo is None else np.asarray(lo, float)
    hi = np.full(nplan, np.inf) if hi is None else np.asarray(hi, float)
    status = np.zeros(E, np.int32)
    t_hit, clear_lb = np.full(E, np.nan), np.full(E, np.inf)
    pair, nodes, depth = np.full(E, -1, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    margin = np.full(E, np.inf)
    finite = np.isfinite(QA).all(axis=1) & np.isfinite(QB).all(axis=1)
    with np.errstate(invalid="ignore"):
        inside = ((QA >= lo) & (QA <= hi) & (QB >= lo) & (QB <= hi)).all(axis=1)
    status[~finite] = NONFINITE
    status[finite & ~inside] = RANGE
    live = np.flatnonzero(finite & inside)
    undecided, hit = np.zeros(E, bool), np.zeros(E, bool)
    # round 0: (edge, t, h, end point)
    edge = np.repeat(live, 3)
    t = np.tile([0.0, 0.5, 1.0], len(live))
    h = np.tile([0.0, 0.5, 0.0], len(live))
    for k in range(max_depth + 1):
        if len(edge) == 0:
            break
        d = QB[edge] - QA[edge]
        rows = QA[edge] + t[:, None] * d
        if k == 0:
            rows[t == 0.0] = QA[edge[t == 0.0]]
            rows[t == 1.0] = QB[edge[t == 1.0]]
        HD = h[:, None] * np.abs(d)
        slack, _sp, gap, gp = measure(rows, HD)
        np.add.at(nodes, edge, 1)
        depth[edge] = k
        np.minimum.at(margin, edge, np.minimum(np.abs(slack - d_min - SWEEP_SLACK), np.minimum(np.abs(gap - d_min), np.abs(gap))))
        is_hit = (gap <= 0) | (gap < d_min)
        cert = ~is_hit & (slack - d_min >= SWEEP_SLACK)
        rest = ~is_hit & ~cert
        stuck = rest & ((h == 0.0) | (k == max_depth))
        split = rest & ~stuck
        for j in np.flatnonzero(is_hit):  # the least t of this depth
            e = edge[j]
            if not hit[e] or t[j] < t_hit[e]:
                hit[e], t_hit[e], pair[e] = True, t[j], gp[j]
        np.minimum.at(clear_lb, edge[cert], slack[cert])
        undecided[edge[stuck]] = True
        go = split & ~hit[edge]  # an edge hit in this round opens no further nodes
        e2, t2, h2 = edge[go], t[go], h[go] / 2
        edge = np.concatenate([e2, e2])
        t = np.concatenate([t2 - h2, t2 + h2])
        h = np.concatenate([h2, h2])
    measured = finite & inside
    status[measured & hit] = HIT
    status[measured & ~hit & undecided] = UNDECIDED
    clear_lb[status != FREE] = np.nan
    t_hit[status != HIT] = np.nan
    pair[status != HIT] = -1
    return dict(status=status, t_hit=t_hit, clear_lb=clear_lb, pair=pair, nodes=nodes, depth=depth, margin=margin)
