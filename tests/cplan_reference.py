"""NumPy statement of mjpl_plan_paths_constrained (include/mjpl_hip.h): lockstep bidirectional RRT over B problems whose
every tree edge is one projected step of at most epsilon, and whose trees are joined by a bridge -- a chain of projected
steps from the growing tree towards the other tree -- operation for operation.

The verdicts are four callables over planning rows:
  valid_configs(Q [N, d]) -> bool [N] and pose_valid(Q [N, d]) -> bool [N], each called at most once, with the ends of
      every problem whose ends are finite (QI[b] then QG[b], problems in order);
  project(A [N, d], X [N, d]) -> (Y [N, d], ok bool [N]): PoseConstraint.apply with q_old = A[i] on X[i]; called at most
      once per step s of the round's bridge chains (the problems whose chain is still going, in order) and at most once
      for the round's extensions (problems in order, candidates in order);
  valid_edges(QA [E, d], QB [E, d]) -> bool [E], called at most once per round with every edge of every live problem:
      problems in order, and per problem the links, the closing edge, then the non-void extensions in candidate order.
Every float64 operation is written one rounding at a time, so the kernels can be compared with it bit for bit.
"""
import numpy as np

from plan_reference import d2, nearest, step, target

SOLVED, ROUNDS, NONFINITE, INVALID_END, NODES, LONG = 0, 1, 2, 3, 4, 5


def void_rules(a, y, ok, t):
    """cstep's three termination rules on the projection y of step(a, t): True = void."""
    return (not ok) or bool(np.sqrt(d2(a, y)) < 1e-8) or bool(d2(y, t) > d2(a, t))


def _chain_of(T, par, k):
    idx = []
    while k >= 0:
        idx.append(k)
        k = par[k]
    return idx


def plan_paths_constrained(QI, QG, lo, hi, valid_configs, valid_edges, project, pose_valid, epsilon, rounds=64, candidates=16,
                           nodes=1024, chain=8, max_rows=256, seed=0):
    """-> dict(P float64 [B, max_rows, d], n_out, status, rounds_used, edges int32 [B], tree_nodes int32 [B, 2], trees,
    junction, forward): `trees` is, per problem, None or ([T0 rows], [T0 parents], [T1 rows], [T1 parents]); `junction` [B]
    the row of a joined problem's path that is T0's junction node (the next row is T1's), -1 for the others; `forward` is,
    per problem, None or a bool per path segment: True if the segment was validated from its first row to its second."""
    QI, QG = np.ascontiguousarray(QI, np.float64), np.ascontiguousarray(QG, np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    B, d = QI.shape
    P = np.zeros((B, max_rows, d), np.float64)
    n_out, rounds_used, edges = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tree_nodes = np.zeros((B, 2), np.int32)
    state = [None] * B  # None: live
    trees = [None] * B
    gained = [0] * B
    junction = np.full(B, -1, np.int32)
    forward = [None] * B
    # the ends
    for b in range(B):
        if not (np.isfinite(QI[b]).all() and np.isfinite(QG[b]).all()):
            state[b] = NONFINITE
    rest = [b for b in range(B) if state[b] is None]
    if rest:
        ends = np.stack([q for b in rest for q in (QI[b], QG[b])])
        ok = np.asarray(valid_configs(ends), dtype=bool) & np.asarray(pose_valid(ends), dtype=bool)
        for k, b in enumerate(rest):
            if not (ok[2 * k] and ok[2 * k + 1]):
                state[b] = INVALID_END
            else:
                trees[b] = ([QI[b].copy()], [-1], [QG[b].copy()], [-1])
    # the rounds
    for r in range(rounds):
        g, o = r & 1, 1 - (r & 1)
        work = []
        for b in range(B):
            if state[b] is not None:
                continue
            Tg, To = trees[b][2 * g], trees[b][2 * o]
            ng, no = len(Tg), len(To)
            if ng >= nodes:
                state[b], rounds_used[b] = NODES, r
                continue
            Tga = np.stack(Tg)
            best = None
            for p in range(no - max(1, gained[b]), no):  # the bridge target
                n, dd = nearest(Tga, To[p])
                if best is None or dd < best[0]:
                    best = (dd, p, n)
            work.append(dict(b=b, Tga=Tga, ng=ng, p=best[1], n=best[2], t=To[best[1]], c=Tg[best[2]], links=[], closing=False,
                             going=True, ext=[]))
        if not work:
            break
        # the bridge chains: step s of every chain still going, one projection call per s
        for s in range(1, chain + 1):
            todo = []
            for w in work:
                if not w["going"]:
                    continue
                if s > min(chain, nodes - w["ng"]):
                    w["going"] = False
                elif np.sqrt(d2(w["c"], w["t"])) <= epsilon:
                    w["closing"], w["going"] = True, False
                else:
                    todo.append(w)
            if not todo:
                break
            A = np.stack([w["c"] for w in todo])
            Y, ok = project(A, np.stack([step(w["c"], w["t"], epsilon) for w in todo]))
            for i, w in enumerate(todo):
                if void_rules(A[i], Y[i], ok[i], w["t"]):
                    w["going"] = False
                else:
                    w["links"].append(np.array(Y[i], np.float64))
                    w["c"] = w["links"][-1]
        # the extensions, one projection call
        A, X, owner = [], [], []
        for w in work:
            for l in range(min(candidates, nodes - w["ng"] - len(w["links"]))):
                t = target(lo, hi, seed, w["b"], r, l)
                k, _ = nearest(w["Tga"], t)
                A.append(w["Tga"][k])
                X.append(step(w["Tga"][k], t, epsilon))
                owner.append((w, k, t))
        if A:
            A = np.stack(A)
            Y, ok = project(A, np.stack(X))
            for i, (w, k, t) in enumerate(owner):
                if not void_rules(A[i], Y[i], ok[i], t):
                    w["ext"].append((k, np.array(Y[i], np.float64)))
        # one edge launch
        qa, qb = [], []
        for w in work:
            prev = w["Tga"][w["n"]]
            for y in w["links"]:
                qa.append(prev)
                qb.append(y)
                prev = y
            if w["closing"]:
                qa.append(prev)
                qb.append(w["t"])
            for k, y in w["ext"]:
                qa.append(w["Tga"][k])
                qb.append(y)
        ok = np.asarray(valid_edges(np.stack(qa), np.stack(qb)), dtype=bool) if qa else np.zeros(0, bool)
        at = 0
        for w in work:
            b, nl = w["b"], len(w["links"])
            cnt = nl + int(w["closing"]) + len(w["ext"])
            v = ok[at:at + cnt]
            at += cnt
            edges[b] += cnt
            Tg, parg = trees[b][2 * g], trees[b][2 * g + 1]
            lead = 0
            while lead < nl and v[lead]:
                lead += 1
            last = w["n"]
            for y in w["links"][:lead]:
                Tg.append(y)
                parg.append(last)
                last = len(Tg) - 1
            gained[b] = lead
            if w["closing"] and lead == nl and v[nl]:
                T0, par0, T1, par1 = trees[b]
                j = {g: last, o: w["p"]}
                i0, i1 = _chain_of(T0, par0, j[0])[::-1], _chain_of(T1, par1, j[1])
                rounds_used[b] = r + 1
                if len(i0) + len(i1) > max_rows:
                    state[b] = LONG
                    continue
                rows = [T0[k] for k in i0] + [T1[k] for k in i1]
                state[b], n_out[b], junction[b] = SOLVED, len(rows), len(i0) - 1
                P[b, :len(rows)] = rows
                # T0's segments run parent -> child (validated that way), T1's child -> parent; the closing edge runs
                # from the growing tree to the other one
                forward[b] = [True] * (len(i0) - 1) + [g == 0] + [False] * (len(i1) - 1)
                continue
            for (k, y), vv in zip(w["ext"], v[nl + int(w["closing"]):]):
                if vv:
                    Tg.append(y)
                    parg.append(k)
                    gained[b] += 1
    status = np.zeros(B, np.int32)
    for b in range(B):
        if state[b] is None:
            status[b], rounds_used[b] = ROUNDS, rounds
        else:
            status[b] = state[b]
        if trees[b] is not None:
            tree_nodes[b] = (len(trees[b][0]), len(trees[b][2]))
    return dict(P=P, n_out=n_out, status=status, rounds_used=rounds_used, edges=edges, tree_nodes=tree_nodes, trees=trees,
                junction=junction, forward=forward)
