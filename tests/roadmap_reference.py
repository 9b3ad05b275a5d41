"""NumPy statement of mjpl_roadmap_build and mjpl_roadmap_query (include/mjpl_hip.h), operation for operation.

The verdicts are two callables: ``valid_configs(Q [N, d]) -> bool [N]`` and ``valid_edges(QA [E, d], QB [E, d]) -> bool [E]``.
``build`` calls the first once with every row (zeros in place of a row that holds a NaN or inf) and the second at most
once, with the candidate pairs in ascending (i, j), lower index first.  ``query`` calls the first once with the ends of
every problem (QI[b] then QG[b], problems in order; zeros for a problem with a non-finite end) and the second at most
once: per problem the direct edge, the start attachments in rank order, the goal attachments in rank order.  Every
float64 operation is written one rounding at a time, so the kernels can be compared with it bit for bit.

The search is Dijkstra's algorithm on a heap -- deliberately not the kernels' schedule, which relaxes in sweeps: the
distances are the least fixed point of dist[v] = min(init[v], min_u fl(dist[u] + w(u, v))), which is unique and which
both compute.
"""
import heapq

import numpy as np

from plan_reference import d2

SOLVED, NO_PATH, NONFINITE, INVALID_END, LONG = 0, 1, 2, 3, 4
MAX_K = 32


def nearest_k(Q, ok, x, k, r2, lo2=None, skip=-1):
    """(indices, d2) of the first k by ascending (d2, j) of the rows j with ok[j], j != skip, [lo2 <=] d2(Q[j], x) <= r2."""
    dd = d2(Q, x)
    with np.errstate(invalid="ignore"):
        take = ok & (dd <= r2)
        if lo2 is not None:
            take &= dd >= lo2
    if skip >= 0:
        take[skip] = False
    idx = np.flatnonzero(take)
    order = np.lexsort((idx, dd[idx]))[:k]  # (stable: d2 first, then the index)
    return idx[order], dd[idx[order]]


def build(Q, valid_configs, valid_edges, radius, k):
    """-> dict(node_valid uint8 [N], row_off int32 [N + 1], adj int32 [2 N k], w float64 [2 N k], pairs int [E, 2], pair_valid bool [E])."""
    Q = np.asarray(Q, np.float64)
    N, cap = len(Q), 2 * len(Q) * k
    out = dict(node_valid=np.zeros(N, np.uint8), row_off=np.zeros(N + 1, np.int32), adj=np.full(cap, -1, np.int32),
               w=np.zeros(cap, np.float64), pairs=np.zeros((0, 2), np.int64), pair_valid=np.zeros(0, bool))
    if N == 0:
        return out
    finite = np.isfinite(Q).all(axis=1)
    ok = finite & np.asarray(valid_configs(np.where(finite[:, None], Q, 0.0)), dtype=bool)
    out["node_valid"] = ok.astype(np.uint8)
    r2 = np.float64(radius) * np.float64(radius)
    lo2 = r2 * np.float64(2.0 ** -40)
    pairs = set()
    for i in np.flatnonzero(ok):
        for j in nearest_k(Q, ok, Q[i], k, r2, lo2, skip=i)[0]:
            pairs.add((min(i, j), max(i, j)))
    pairs = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    out["pairs"] = pairs
    if len(pairs) == 0:
        return out
    good = np.asarray(valid_edges(Q[pairs[:, 0]], Q[pairs[:, 1]]), dtype=bool)
    out["pair_valid"] = good
    kept = pairs[good]
    directed = np.concatenate([kept, kept[:, ::-1]])
    directed = directed[np.lexsort((directed[:, 1], directed[:, 0]))]
    n = len(directed)
    out["row_off"] = np.searchsorted(directed[:, 0], np.arange(N + 1), side="left").astype(np.int32)
    out["adj"][:n] = directed[:, 1]
    out["w"][:n] = np.sqrt(d2(Q[directed[:, 0]], Q[directed[:, 1]]))
    return out


def dijkstra(row_off, adj, w, init):
    """The least fixed point of dist[v] = min(init[v], min_{u in adj(v)} fl(dist[u] + w(u, v))), by a heap."""
    dist = np.array(init, np.float64)
    heap = [(float(dist[v]), int(v)) for v in np.flatnonzero(np.isfinite(dist))]
    heapq.heapify(heap)
    done = np.zeros(len(dist), bool)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du != dist[u]:
            continue
        done[u] = True
        for p in range(row_off[u], row_off[u + 1]):
            v = int(adj[p])
            c = np.float64(du) + w[p]
            if c < dist[v]:
                dist[v] = c
                heapq.heappush(heap, (float(c), v))
    return dist


def walk_back(row_off, adj, w, init, dist, g):
    """The nodes from g back to a start attachment, as stated: stop at v if init[v] == dist[v], otherwise go to the
    lowest-index u of row v with fl(dist[u] + w(u, v)) == dist[v].  At most N steps."""
    chain, v = [int(g)], int(g)
    for _ in range(len(dist)):
        if init[v] == dist[v]:
            return chain
        nxt = -1
        for p in range(row_off[v], row_off[v + 1]):
            if dist[adj[p]] + w[p] == dist[v]:
                nxt = int(adj[p])
                break
        assert nxt >= 0, "dist is not a fixed point"
        v = nxt
        chain.append(v)
    raise AssertionError("the walk did not end within N steps")


def query(Q, graph, QI, QG, valid_configs, valid_edges, radius, connections, max_rows):
    """-> dict(P float64 [B, max_rows, d], n_out, status int32 [B], cost float64 [B], edges int, searched bool [B])."""
    Q, QI, QG = np.asarray(Q, np.float64), np.asarray(QI, np.float64), np.asarray(QG, np.float64)
    N, B, d = len(Q), len(QI), QI.shape[1]
    ok, row_off, adj, w = graph["node_valid"].astype(bool), graph["row_off"], graph["adj"], graph["w"]
    res = dict(P=np.zeros((B, max_rows, d)), n_out=np.zeros(B, np.int32), status=np.zeros(B, np.int32), cost=np.zeros(B),
               edges=0, searched=np.zeros(B, bool))
    if B == 0:
        return res
    finite = np.isfinite(QI).all(axis=1) & np.isfinite(QG).all(axis=1)
    ends = np.stack([np.where(finite[:, None], QI, 0.0), np.where(finite[:, None], QG, 0.0)], axis=1).reshape(2 * B, d)
    cv = np.asarray(valid_configs(ends), dtype=bool).reshape(B, 2)
    r2 = np.float64(radius) * np.float64(radius)
    state = np.where(~finite, NONFINITE, np.where(cv.all(axis=1), -1, INVALID_END))
    att, QA, QB, off = {}, [], [], {}
    for b in np.flatnonzero(state == -1):
        s = nearest_k(Q, ok, QI[b], connections, r2)
        g = nearest_k(Q, ok, QG[b], connections, r2)
        att[b] = (s, g)
        off[b] = len(QA)
        QA += [QI[b]] + [QI[b]] * len(s[0]) + [Q[v] for v in g[0]]
        QB += [QG[b]] + [Q[v] for v in s[0]] + [QG[b]] * len(g[0])
    res["edges"] = len(QA)
    verdict = np.asarray(valid_edges(np.array(QA).reshape(-1, d), np.array(QB).reshape(-1, d)), dtype=bool) if QA else np.zeros(0, bool)
    for b in range(B):
        if state[b] != -1:
            res["status"][b] = state[b]
            continue
        e0 = off[b]
        if verdict[e0]:
            res["P"][b, 0], res["P"][b, 1] = QI[b], QG[b]
            res["n_out"][b], res["cost"][b] = 2, np.sqrt(d2(QI[b], QG[b]))
            continue
        (sj, sd), (gj, gd) = att[b]
        sv, gv = verdict[e0 + 1:e0 + 1 + len(sj)], verdict[e0 + 1 + len(sj):e0 + 1 + len(sj) + len(gj)]
        res["searched"][b] = True
        init = np.full(N, np.inf)
        init[sj[sv]] = np.sqrt(sd[sv])
        dist = dijkstra(row_off, adj, w, init)
        total, goal = np.inf, -1
        for j in range(len(gj)):
            if gv[j]:
                c = dist[gj[j]] + np.sqrt(gd[j])
                if c < total:
                    total, goal = c, int(gj[j])
        if goal < 0:
            res["status"][b] = NO_PATH
            continue
        chain = walk_back(row_off, adj, w, init, dist, goal)
        if len(chain) + 2 > max_rows:
            res["status"][b] = LONG
            continue
        n = len(chain) + 2
        res["P"][b, 0], res["P"][b, n - 1] = QI[b], QG[b]
        res["P"][b, 1:n - 1] = Q[chain[::-1]]
        res["n_out"][b], res["cost"][b] = n, total
    return res


def jacobi(row_off, adj, w, init):
    """The same fixed point by plain Jacobi iteration: every sweep reads only the previous sweep's values."""
    dist = np.array(init, np.float64)
    for _ in range(len(dist) + 1):
        new = dist.copy()
        for v in range(len(dist)):
            for p in range(row_off[v], row_off[v + 1]):
                c = dist[adj[p]] + w[p]
                if c < new[v]:
                    new[v] = c
        if np.array_equal(new, dist):
            return dist
        dist = new
    raise AssertionError("no fixed point within N sweeps")


def components(row_off, adj, node_valid):
    """Label of every node's connected component (the lowest node index in it); -1 for an invalid row."""
    N = len(node_valid)
    label = np.full(N, -1, np.int64)
    for s in range(N):
        if not node_valid[s] or label[s] >= 0:
            continue
        label[s] = s
        stack = [s]
        while stack:
            u = stack.pop()
            for v in adj[row_off[u]:row_off[u + 1]]:
                if label[v] < 0:
                    label[v] = s
                    stack.append(int(v))
    return label
