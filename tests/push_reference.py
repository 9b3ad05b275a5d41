"""Independent NumPy float64 statement of the push-out iteration (include/mjpl_hip.h: mjpl_push_out*), over a callback
that lists near pairs: ``near(Q) -> (count [n], pair [n, K], dist [n, K], grad [n, K, nq], status [n, K])`` in the
shapes of ``Engine.near_pairs`` without the witnesses.  The callback may be the engine's own list (the GPU test checks
the step arithmetic against this statement) or the reference distances with central differences (the host study).

Per row and iteration it records the decision margin: the smallest |dist_p - margin_p - d_min| over the listed slots,
i.e. how far the row was from a different set of violated slots.  A comparison of two runs is meaningful only on rows
whose margin stays clear of the measuring error.

The solve is ``np.linalg.solve`` (LU), not a Cholesky factorisation.  Nothing of the product's kernels is used.
"""
import numpy as np

GRAD_DEGENERATE = 2  # MJPL_GRAD_DEGENERATE


def push_out(near, Q, margins, d_min, *, overshoot=1e-3, damping=1e-4, step_max=0.2, max_iter=16, lo=None, hi=None,
             watch=()):
    """Q [N, nq], margins [P] (per candidate pair) -> (Q_out [N, nq], iters [N], degenerate bool [N],
    decision margin [N, max_iter], inf where a row was not measured or listed nothing, watched bool [N]: a violated
    slot of the row had, at some iteration, a gradient that is not exactly 0 in one of the columns `watch`)."""
    Q = np.array(Q, dtype=np.float64)
    n, nq = Q.shape
    iters = np.zeros(n, np.int32)
    degenerate = np.zeros(n, bool)
    decision = np.full((n, max_iter), np.inf)
    watched = np.zeros(n, bool)
    watch = np.asarray(watch, dtype=np.int64)
    active = np.arange(n)
    for it in range(max_iter):
        if len(active) == 0:
            break
        count, pair, dist, grad, status = near(Q[active])
        K = pair.shape[1]
        go = []
        for a, i in enumerate(active):
            m = min(int(count[a]), K)
            if m < 0:
                continue  # (a non-finite row: not moved)
            v = dist[a, :m] - margins[pair[a, :m]]
            if m:
                decision[i, it] = np.abs(v - d_min).min()
            viol = np.flatnonzero(v < d_min)
            if len(watch) and len(viol) and not np.all(grad[a, viol][:, watch] == 0):
                watched[i] = True
            if np.any(status[a, viol] == GRAD_DEGENERATE):
                degenerate[i] = True
                continue
            if len(viol) == 0:
                continue
            A = damping * np.eye(nq)
            b = np.zeros(nq)
            for s in viol:
                g = grad[a, s]
                A += np.outer(g, g)
                b += (d_min + overshoot - v[s]) * g
            delta = np.linalg.solve(A, b)
            big = np.abs(delta).max()
            if big > step_max:
                delta = delta * (step_max / big)
            q = Q[i] + delta
            if lo is not None:
                q = np.maximum(q, lo)
            if hi is not None:
                q = np.minimum(q, hi)
            Q[i] = q
            iters[i] = it + 1
            go.append(i)
        active = np.asarray(go, dtype=np.int64)
    return Q, iters, degenerate, decision, watched


def fd_near(distances, pairs_allowed, distmax, K, h=1e-6):
    """A ``near`` callback from any distance function of a batch ([M, nq] -> D [M, P]): the non-allowed pairs below
    distmax in ascending index, gradients by central differences at step h, status 0."""
    allowed = np.asarray(pairs_allowed, bool)

    def near(Q):
        Q = np.asarray(Q, float)
        n, nq = Q.shape
        S = np.repeat(Q[:, None, :], 1 + 2 * nq, axis=1)  # [n, 1 + 2 nq, nq]: the row, then +h / -h per column
        for j in range(nq):
            S[:, 1 + 2 * j, j] += h
            S[:, 2 + 2 * j, j] -= h
        D = np.asarray(distances(S.reshape(-1, nq))).reshape(n, 1 + 2 * nq, -1)
        D0 = D[:, 0]
        G = (D[:, 1::2] - D[:, 2::2]) / (2 * h)  # [n, nq, P]
        count = np.zeros(n, np.int32)
        pair = np.full((n, K), -1, np.int32)
        dist = np.full((n, K), np.nan)
        grad = np.full((n, K, nq), np.nan)
        status = np.full((n, K), -1, np.int32)
        for i in range(n):
            p = np.flatnonzero(~allowed & (D0[i] < distmax))
            count[i] = len(p)
            p = p[:K]
            pair[i, :len(p)] = p
            dist[i, :len(p)] = D0[i, p]
            grad[i, :len(p)] = G[i][:, p].T
            status[i, :len(p)] = 0
        return count, pair, dist, grad, status

    return near
