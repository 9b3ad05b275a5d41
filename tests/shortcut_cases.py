"""Inputs and invariant checks shared by tests/test_shortcut_host.py and tests/test_gpu_shortcut.py."""
import numpy as np

import shortcut_reference as ref
from mjpl_amd import scenes

# Waypoints per path.  With 64 candidates a round is exhaustive up to 12 live waypoints (55 pairs; 13 have 66), with 7
# up to 5 (6 pairs; 6 have 10), with 1 at 3; the live list is compacted 64 entries at a time.
LENGTHS = (2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 31, 63, 64, 65, 66, 127, 128, 129, 130)


def path_lengths(B: int) -> list:
    return [LENGTHS[b % len(LENGTHS)] for b in range(B)]


def franka_planning():
    """(model, planning columns, base configuration) of the headline scene."""
    model = scenes.franka_p(obstacles=True)
    return model, scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS), model.keyframe("home").qpos.copy()


def random_walks(lo, hi, valid_configs, lengths, seed, step=0.3, tries=16):
    """Seeded random walks of valid configurations inside [lo, hi], in lockstep: a uniform valid start, then steps of
    0.5 .. 1 times `step` in a uniform direction, the first of `tries` draws that valid_configs ([N, d] -> bool [N])
    accepts.  -> list of float64 [n_b, d]."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    lengths = np.asarray(lengths)
    B, d = len(lengths), len(lo)
    cur = np.zeros((B, d))
    need = np.ones(B, bool)
    while need.any():
        idx = np.flatnonzero(need)
        Q = rng.uniform(lo, hi, size=(len(idx), d))
        ok = np.asarray(valid_configs(Q), dtype=bool)
        cur[idx[ok]] = Q[ok]
        need[idx[ok]] = False
    paths = [[cur[b].copy()] for b in range(B)]
    for k in range(1, int(lengths.max())):
        pending = np.flatnonzero(lengths > k)
        while len(pending):
            dirs = rng.normal(size=(len(pending), tries, d))
            dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
            cand = np.clip(cur[pending][:, None, :] + dirs * rng.uniform(0.5, 1.0, size=(len(pending), tries, 1)) * step, lo, hi)
            ok = np.asarray(valid_configs(cand.reshape(-1, d)), dtype=bool).reshape(len(pending), tries)
            first, has = ok.argmax(axis=1), ok.any(axis=1)
            for p, b in enumerate(pending):
                if has[p]:
                    cur[b] = cand[p, first[p]]
                    paths[b].append(cur[b].copy())
            pending = pending[~has]
    return [np.stack(p) for p in paths]


def pack(paths):
    """(W [rows, d], wp_off int64 [B + 1])."""
    return np.concatenate(paths), np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)


def ball_paths():
    """Two paths of scenes.two_dof_ball() (ball r = 0.1, wall x in [0.5, 0.7], |y| <= 0.5): a zigzag through free space
    well left of the wall, and a path over the wall's upper end from (0, 0) to (1.2, 0)."""
    t = np.linspace(0.0, 1.0, 21)
    zigzag = np.stack([-1.5 + 1.2 * t, -1.0 + 2.0 * t + 0.25 * np.where(np.arange(21) % 2 == 1, 1.0, -1.0) * (t > 0) * (t < 1)], axis=1)
    knots = np.array([[0, 0], [0.05, 0.45], [0.2, 0.8], [0.4, 0.95], [0.6, 1.0], [0.8, 0.95], [1.0, 0.8], [1.15, 0.45], [1.2, 0]], float)
    over = [knots[0]]
    for a, b in zip(knots[:-1], knots[1:]):
        over += [a + (b - a) * 0.5, b]
    return [zigzag, np.stack(over)]


def check_invariants(W, wp_off, res, verdict, min_saving=0.0):
    """What every result of the algorithm obeys, whatever the verdict."""
    B = len(wp_off) - 1
    for b in range(B):
        w0, w1 = int(wp_off[b]), int(wp_off[b + 1])
        keep = res["keep"][w0:w1]
        if res["status"][b] == ref.NONFINITE:
            assert keep.all()
            continue
        assert keep[0] == 1 and keep[-1] == 1, b
        rows = w0 + np.flatnonzero(keep)
        assert res["n_out"][b] == len(rows)
        # accepted shortcuts of one round never overlap
        by_round = {}
        for r, i, j in res["taken"][b]:
            assert j >= i + 2
            for i2, j2 in by_round.setdefault(r, []):
                assert j <= i2 or j2 <= i, (b, r)
            by_round[r].append((i, j))
        assert res["accepted"][b] == len(res["taken"][b])
        # the length never grows.  Every accepted shortcut saved s > 0 on the sums of its round; the final sum adds the
        # same segments in another grouping, so it may differ from that by rounding: at most n additions of half an ulp
        n = w1 - w0
        before, after = ref.arc_lengths(W, np.arange(w0, w1))[-1], ref.arc_lengths(W, rows)[-1]
        assert after == res["length"][b]
        assert after <= before * (1.0 + n * 2.0 ** -52), b
        if len(res["taken"][b]):
            assert after < before
        # every surviving segment that is not an original one passed the verdict
        new = [(a, c) for a, c in zip(rows[:-1], rows[1:]) if c != a + 1]
        if new:
            assert np.asarray(verdict(W[[a for a, _ in new]], W[[c for _, c in new]]), dtype=bool).all(), b
        # converged: no single shortcut is both valid and shorter
        if res["status"][b] == ref.CONVERGED and len(rows) > 2:
            L = ref.arc_lengths(W, rows)
            pairs = [(i, j) for i in range(len(rows) - 2) for j in range(i + 2, len(rows))]
            dd = ref.dist(W, rows[[i for i, _ in pairs]], rows[[j for _, j in pairs]])
            shorter = [(i, j) for (i, j), dij in zip(pairs, dd) if (L[j] - L[i]) - dij > min_saving]
            if shorter:
                ok = np.asarray(verdict(W[rows[[i for i, _ in shorter]]], W[rows[[j for _, j in shorter]]]), dtype=bool)
                assert not ok.any(), b


def check_rounds_prefix(W, wp_off, verdict, long_run, R1, **params):
    """The state after rounds = R1 is the state of the longer run after R1 rounds."""
    short = ref.shortcut_paths(W, wp_off, verdict, rounds=R1, **params)
    keep = np.ones(len(W), np.uint8)
    for b, taken in enumerate(long_run["taken"]):
        for r, i, j in taken:
            if r < R1:
                keep[wp_off[b] + i + 1:wp_off[b] + j] = 0
    assert np.array_equal(short["keep"], keep)
    for b, taken in enumerate(long_run["taken"]):
        assert short["taken"][b] == [t for t in taken if t[0] < R1]
