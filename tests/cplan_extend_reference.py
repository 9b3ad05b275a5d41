"""NumPy statement of mjpl_plan_paths_constrained_ext (include/mjpl_hip.h): tests/cplan_reference.py with chained
extensions -- candidate l of a round is no longer ONE projected step from its nearest node towards its target but a chain
of up to `extend` of them, each from the projected row before it, cut at the first void step.  This is what the
reference's _constrained_extend does until it is stopped, taken inside one round.  extend = 1 is cplan_reference in
every output byte.

The verdicts are cplan_reference's four callables.  `project` is called at most once per step s of the round's bridge
chains, then at most once per step s = 1 .. extend of the round's extension chains, with the candidates whose chain is
still going (problems in order, candidates in order); `valid_edges` at most once per round: problems in order, and per
problem the bridge links, the closing edge, then for l ascending chain l's links for s ascending.
Every float64 operation is written one rounding at a time, so the kernels can be compared with it bit for bit.
"""
import numpy as np

from cplan_reference import INVALID_END, LONG, NODES, NONFINITE, ROUNDS, SOLVED, void_rules
from plan_reference import d2, nearest, step, target


def _chain_of(par, k):
    idx = []
    while k >= 0:
        idx.append(k)
        k = par[k]
    return idx


def plan_paths_constrained(QI, QG, lo, hi, valid_configs, valid_edges, project, pose_valid, epsilon, rounds=64, candidates=16,
                           nodes=1024, chain=8, max_rows=256, seed=0, extend=1):
    """-> the dict of cplan_reference.plan_paths_constrained (`trees`, `junction` and `forward` included)."""
    if not 1 <= extend <= 32:
        raise ValueError(f"extend must be 1..32, got {extend}")
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
        # the extension chains: target and nearest node over the tree as it stood at the start of the round, then step s
        # of every chain still going, one projection call per s
        going = []
        for w in work:
            for l in range(min(candidates, nodes - w["ng"] - len(w["links"]))):
                t = target(lo, hi, seed, w["b"], r, l)
                k, _ = nearest(w["Tga"], t)
                c = dict(k=k, t=t, x=w["Tga"][k], links=[])
                w["ext"].append(c)
                going.append(c)
        for s in range(1, extend + 1):
            if not going:
                break
            A = np.stack([c["x"] for c in going])
            Y, ok = project(A, np.stack([step(c["x"], c["t"], epsilon) for c in going]))
            still = []
            for i, c in enumerate(going):
                if not void_rules(A[i], Y[i], ok[i], c["t"]):
                    c["links"].append(np.array(Y[i], np.float64))
                    c["x"] = c["links"][-1]
                    still.append(c)
            going = still
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
            for c in w["ext"]:
                prev = w["Tga"][c["k"]]
                for y in c["links"]:
                    qa.append(prev)
                    qb.append(y)
                    prev = y
        ok = np.asarray(valid_edges(np.stack(qa), np.stack(qb)), dtype=bool) if qa else np.zeros(0, bool)
        at = 0
        for w in work:
            b, nl = w["b"], len(w["links"])
            cnt = nl + int(w["closing"]) + sum(len(c["links"]) for c in w["ext"])
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
                i0, i1 = _chain_of(par0, j[0])[::-1], _chain_of(par1, j[1])
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
            e = nl + int(w["closing"])
            for c in w["ext"]:
                last = c["k"]
                for s, y in enumerate(c["links"]):  # the leading valid links, while the tree has room
                    if not v[e + s] or len(Tg) >= nodes:
                        break
                    Tg.append(y)
                    parg.append(last)
                    last = len(Tg) - 1
                    gained[b] += 1
                e += len(c["links"])
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
