"""NumPy statement of mjpl_plan_paths (include/mjpl_hip.h): lockstep bidirectional RRT over B problems, operation for
operation.

The verdicts are two callables: ``valid_configs(Q [N, d]) -> bool [N]``, called at most once with the ends of every
problem whose ends are finite (QI[b] then QG[b], problems in order), and ``valid_edges(QA [E, d], QB [E, d]) -> bool [E]``,
called at most once for the direct edges and at most once per round, with every edge of every live problem: problems in
order, and per problem the connect edge first, then the extensions in candidate order.  Every float64 operation is
written one rounding at a time (no dot products, no sums over an axis), so the kernels can be compared with it bit for bit.
"""
import numpy as np

SOLVED, ROUNDS, NONFINITE, INVALID_END, NODES = 0, 1, 2, 3, 4
_M64 = (1 << 64) - 1


def splitmix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def d2(A: np.ndarray, t: np.ndarray) -> np.ndarray:
    """d2(A[k], t) for every row of A [n, d] (or of t, or of both): the columns added in order from 0.0."""
    A, t = np.asarray(A, np.float64), np.asarray(t, np.float64)
    s = np.zeros(np.broadcast(A[..., 0], t[..., 0]).shape, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(A.shape[-1]):
            v = t[..., c] - A[..., c]
            s = s + v * v
    return s


def nearest(T: np.ndarray, t: np.ndarray):
    """(lowest index k that minimises d2(T[k], t), that d2)."""
    dd = d2(T, t)
    k = int(np.argmin(dd))  # (the first of equal minima)
    return k, dd[k]


def step(a: np.ndarray, t: np.ndarray, epsilon: float) -> np.ndarray:
    m = np.sqrt(d2(a, t))
    if m <= epsilon:
        return t.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return a + ((t - a) / m) * np.float64(epsilon)  # (elementwise: one rounding per operation and column)


def target(lo: np.ndarray, hi: np.ndarray, seed: int, b: int, r: int, l: int) -> np.ndarray:
    """The sample extension candidate l of problem b draws in round r."""
    z = splitmix(splitmix(splitmix(seed & _M64) ^ b) ^ (64 * r + l))
    t = np.zeros(len(lo), np.float64)
    for c in range(len(lo)):
        u = np.float64(z >> 11) * np.float64(2.0 ** -53)
        t[c] = lo[c] + u * (hi[c] - lo[c])
        z = splitmix(z)
    return t


def _chain(T, par, k):
    rows = []
    while k >= 0:
        rows.append(T[k])
        k = par[k]
    return rows


def plan_paths(QI, QG, lo, hi, valid_configs, valid_edges, epsilon, rounds=32, candidates=16, nodes=1024, seed=0):
    """-> dict(P float64 [B, rounds + 2, d], n_out, status, rounds_used, edges int32 [B], tree_nodes int32 [B, 2], trees):
    `trees` is, per problem, None or ([T0 rows], [T0 parents], [T1 rows], [T1 parents]); `junction` [B] the row of a
    solved problem's path that is T0's junction node (the next row is T1's), -1 for the others."""
    QI, QG = np.ascontiguousarray(QI, np.float64), np.ascontiguousarray(QG, np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    B, d = QI.shape
    P = np.zeros((B, rounds + 2, d), np.float64)
    n_out, rounds_used, edges = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tree_nodes = np.zeros((B, 2), np.int32)
    state = [None] * B  # None: live
    trees = [None] * B
    gained = [0] * B
    junction = np.full(B, -1, np.int32)
    # the ends
    for b in range(B):
        if not (np.isfinite(QI[b]).all() and np.isfinite(QG[b]).all()):
            state[b] = NONFINITE
    rest = [b for b in range(B) if state[b] is None]
    if rest:
        ok = np.asarray(valid_configs(np.stack([q for b in rest for q in (QI[b], QG[b])])), dtype=bool)
        for k, b in enumerate(rest):
            if not (ok[2 * k] and ok[2 * k + 1]):
                state[b] = INVALID_END
    rest = [b for b in range(B) if state[b] is None]
    if rest:
        ok = np.asarray(valid_edges(QI[rest], QG[rest]), dtype=bool)
        for k, b in enumerate(rest):
            edges[b] += 1
            if ok[k]:
                state[b] = SOLVED
                P[b, 0], P[b, 1] = QI[b], QG[b]
                n_out[b], junction[b] = 2, 0
            else:
                trees[b] = ([QI[b].copy()], [-1], [QG[b].copy()], [-1])
    # the rounds
    for r in range(rounds):
        g, o = r & 1, 1 - (r & 1)
        work, qa, qb = [], [], []  # (problem, connect (p, n) or None, [(k, q)])
        for b in range(B):
            if state[b] is not None:
                continue
            Tg, To = trees[b][2 * g], trees[b][2 * o]
            ng, no = len(Tg), len(To)
            if ng >= nodes:
                state[b], rounds_used[b] = NODES, r
                continue
            Tga = np.stack(Tg)
            conn = None
            if gained[b] > 0:
                best = None
                for p in range(no - gained[b], no):
                    n, dd = nearest(Tga, To[p])
                    if best is None or dd < best[0]:
                        best = (dd, p, n)
                conn = (best[1], best[2])
                qa.append(To[conn[0]])
                qb.append(Tg[conn[1]])
            ext = []
            for l in range(min(candidates, nodes - ng)):
                t = target(lo, hi, seed, b, r, l)
                k, _ = nearest(Tga, t)
                q = step(Tg[k], t, epsilon)
                ext.append((k, q))
                qa.append(Tg[k])
                qb.append(q)
            work.append((b, conn, ext))
        if not work:
            break
        ok = np.asarray(valid_edges(np.stack(qa), np.stack(qb)), dtype=bool)
        at = 0
        for b, conn, ext in work:
            cnt = (conn is not None) + len(ext)
            v = ok[at:at + cnt]
            at += cnt
            edges[b] += cnt
            T0, par0, T1, par1 = trees[b]
            if conn is not None and v[0]:
                j = {o: conn[0], g: conn[1]}
                rows = _chain(T0, par0, j[0])[::-1] + _chain(T1, par1, j[1])
                junction[b] = len(_chain(T0, par0, j[0])) - 1
                state[b], rounds_used[b], n_out[b] = SOLVED, r + 1, len(rows)
                P[b, :len(rows)] = rows
                continue
            Tg, parg = trees[b][2 * g], trees[b][2 * g + 1]
            good = [kq for kq, vv in zip(ext, v[(conn is not None):]) if vv]
            for k, q in good:
                Tg.append(q)
                parg.append(k)
            gained[b] = len(good)
    status = np.zeros(B, np.int32)
    for b in range(B):
        if state[b] is None:
            status[b], rounds_used[b] = ROUNDS, rounds
        else:
            status[b] = state[b]
        if trees[b] is not None:
            tree_nodes[b] = (len(trees[b][0]), len(trees[b][2]))
    return dict(P=P, n_out=n_out, status=status, rounds_used=rounds_used, edges=edges, tree_nodes=tree_nodes, trees=trees,
                junction=junction)
