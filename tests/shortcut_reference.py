"""NumPy statement of mjpl_shortcut_paths (include/mjpl_hip.h): batched path shortcutting, operation for operation.

The verdict is a callable ``(QA [E, d], QB [E, d]) -> bool [E]`` (the engine's check_edges on the GPU, the CPU oracle's
or a pure-NumPy one on the host); it is called at most once per round, with every proposed edge of every path, paths in
order and candidates in order within a path.  Every float64 operation is written one rounding at a time (no dot products,
no sums over an axis), so the kernels can be compared with it bit for bit.
"""
import numpy as np

CONVERGED, ROUNDS, NONFINITE = 0, 1, 2
_M64 = (1 << 64) - 1


def splitmix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dist(W: np.ndarray, ra, rb) -> np.ndarray:
    """d(a, b) for arrays of row indices: the columns added in order from 0.0."""
    ra, rb = np.asarray(ra, dtype=np.int64), np.asarray(rb, dtype=np.int64)
    s = np.zeros(ra.shape, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(W.shape[1]):
            t = W[rb, c] - W[ra, c]
            s = s + t * t
        return np.sqrt(s)


def arc_lengths(W: np.ndarray, rows) -> list:
    """L over a list of rows, added in index order."""
    rows = np.asarray(rows, dtype=np.int64)
    seg = dist(W, rows[:-1], rows[1:])
    L = [0.0]
    with np.errstate(over="ignore", invalid="ignore"):
        for v in seg:
            L.append(L[-1] + np.float64(v))
    return L


def candidates_of(m: int, K: int, seed: int, b: int, r: int):
    """(exhaustive, [(l, i, j)]) of a path of m > 2 live waypoints, index b in the call, in round r."""
    npairs = (m - 1) * (m - 2) // 2
    if npairs <= K:
        pairs = [(i, j) for i in range(m - 2) for j in range(i + 2, m)]
        return True, [(l, i, j) for l, (i, j) in enumerate(pairs)]
    out = []
    for l in range(K):
        z = splitmix(splitmix(splitmix(seed & _M64) ^ b) ^ (64 * r + l))
        i = ((z & 0xFFFFFFFF) * (m - 2)) >> 32
        j = i + 2 + (((z >> 32) * (m - 2 - i)) >> 32)
        out.append((l, i, j))
    return False, out


def shortcut_paths(W, wp_off, verdict, rounds=16, candidates=64, seed=0, min_saving=0.0):
    """-> dict(keep uint8 [rows], n_out, status, proposed, accepted int32 [B], length float64 [B], taken): `taken` is,
    per path, the accepted shortcuts as (round, first row, last row), rows counted from the path's first."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    wp_off = np.asarray(wp_off, dtype=np.int64)
    B = len(wp_off) - 1
    live = [list(range(int(wp_off[b + 1] - wp_off[b]))) for b in range(B)]
    state = [None] * B  # None: at work
    proposed, accepted = np.zeros(B, np.int32), np.zeros(B, np.int32)
    taken = [[] for _ in range(B)]
    for b in range(B):
        if not np.isfinite(W[wp_off[b]:wp_off[b + 1]]).all():
            state[b] = NONFINITE
    for r in range(rounds):
        work = []  # (path, exhaustive, [(s, l, i, j)] proposed)
        for b in range(B):
            if state[b] is not None:
                continue
            m = len(live[b])
            if m <= 2:
                state[b] = CONVERGED
                continue
            rows = wp_off[b] + np.asarray(live[b], dtype=np.int64)
            L = arc_lengths(W, rows)
            exhaustive, cands = candidates_of(m, candidates, seed, b, r)
            props = []
            if cands:
                dd = dist(W, rows[[c[1] for c in cands]], rows[[c[2] for c in cands]])
                with np.errstate(over="ignore", invalid="ignore"):
                    for (l, i, j), dij in zip(cands, dd):
                        s = (L[j] - L[i]) - dij
                        if s > min_saving:
                            props.append((s, l, i, j))
            work.append((b, exhaustive, props))
        if not work:
            break
        qa = [wp_off[b] + live[b][i] for b, _, props in work for (_, _, i, _) in props]
        qb = [wp_off[b] + live[b][j] for b, _, props in work for (_, _, _, j) in props]
        ok = np.asarray(verdict(W[qa], W[qb]), dtype=bool) if qa else np.zeros(0, bool)
        at = 0
        for b, exhaustive, props in work:
            good = [p for p, v in zip(props, ok[at:at + len(props)]) if v]
            at += len(props)
            proposed[b] += len(props)
            if exhaustive and not good:
                state[b] = CONVERGED
                continue
            acc = []
            for s, l, i, j in sorted(good, key=lambda p: (-p[0], p[1])):
                if all(j <= i2 or j2 <= i for i2, j2 in acc):
                    acc.append((i, j))
            gone = set()
            for i, j in acc:
                taken[b].append((r, live[b][i], live[b][j]))
                gone.update(range(i + 1, j))
            live[b] = [v for k, v in enumerate(live[b]) if k not in gone]
            accepted[b] += len(acc)
    keep = np.zeros(int(wp_off[-1]) if B else 0, np.uint8)
    n_out, status, length = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float64)
    for b in range(B):
        if state[b] == NONFINITE:
            keep[wp_off[b]:wp_off[b + 1]] = 1
            n_out[b], status[b], length[b] = wp_off[b + 1] - wp_off[b], NONFINITE, np.nan
            continue
        keep[wp_off[b] + np.asarray(live[b], dtype=np.int64)] = 1
        n_out[b] = len(live[b])
        status[b] = ROUNDS if state[b] is None else state[b]
        length[b] = arc_lengths(W, wp_off[b] + np.asarray(live[b], dtype=np.int64))[-1]
    return dict(keep=keep, n_out=n_out, length=length, status=status, proposed=proposed, accepted=accepted, taken=taken)
