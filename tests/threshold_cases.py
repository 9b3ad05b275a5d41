"""Configurations and edges AT a contact threshold of a whole model (NumPy and the CPU oracle only, no GPU).

tests/test_gpu_filter_adversarial.py drives one geom towards one partner along a slide joint of a model made for it.
The per-model generated libraries exist for the models of tests/spec_models.py only, so here the threshold is found on
THOSE models, along a line between two random configurations:

* draw planning-space configurations uniformly within the joint ranges, split them by the oracle's verdict, pair the
  first `n` valid ones (A) with the first `n` invalid ones (B);
* bisect t in [0, 1] on q(t) = A + t (B - A) until the midpoint equals an end: q_free (valid) and q_hit (invalid) come
  from adjacent doubles t;
* probes: q_free - off u and q_hit + off u, u = (B - A) / |B - A|_inf, for every off of OFFSETS;
* edges (a) ending on a probe, (b) through a probe with their first waypoint on it, (c) short random filler from A.

"Near": a bound on how far any point of a moving geom travels per unit |dq|_inf is L = nq * max(1, lever): a slide moves
it by |dq|, a hinge by |dq| times its distance from the axis, which is at most `lever` -- the longest chain of body
offsets (with the joints' own offsets from their bodies' frames) plus the largest |geom_pos| + rbound.  Both geoms of a
pair may move, so the signed distance of the flipping pair at a probe with L * off <= 1e-5 m is within 2e-5 m of its
threshold: inside any band of 1e-4 m, whatever the binary32 arithmetic does.  Such a probe must reach the exact re-check.

Nothing is left out: build() asserts that it found n valid and n invalid draws and that every row bisected down to
adjacent values of t."""
from dataclasses import dataclass

import numpy as np

OFFSETS = np.array([0.0, 1e-9, 1e-7, 1e-6, 1e-5, 5e-5, 9e-5, 1.1e-4, 2e-4, 1e-3])
STEP = 0.01          # the step of tests/test_gpu_spec.py and tests/test_gpu_spec_generic.py
ROWS = 96
DRAWS = 4000
FILLER = 2000
NEAR_METRES = 1e-5
TYPE_NAMES = {0: "plane", 2: "sphere", 3: "capsule", 6: "box"}
NINE_TYPE_PAIRS = frozenset([("plane", "sphere"), ("plane", "capsule"), ("plane", "box"), ("sphere", "sphere"),
                             ("sphere", "capsule"), ("sphere", "box"), ("capsule", "capsule"), ("capsule", "box"),
                             ("box", "box")])


@dataclass
class Edges:
    qa: np.ndarray
    qb: np.ndarray
    valid: np.ndarray      # the oracle's verdicts ...
    first_bad: np.ndarray  # ... and first-bad indices (valid_edges(..., info=True))


@dataclass
class Cases:
    A: np.ndarray
    B: np.ndarray
    q_free: np.ndarray
    q_hit: np.ndarray
    u: np.ndarray          # (B - A) / |B - A|_inf per row
    offsets: np.ndarray
    Q: np.ndarray          # the probes: for every offset the n free-side rows, then the n hit-side rows
    off: np.ndarray        # offset of each probe
    hit_side: np.ndarray   # bool per probe
    row: np.ndarray        # row of A / B each probe belongs to
    near: np.ndarray       # bool per probe: L * off <= NEAR_METRES
    valid: np.ndarray      # the oracle's verdict per probe
    ending: Edges          # shape (a)
    through: Edges         # shape (b)
    filler: Edges          # shape (c)
    pairs: np.ndarray      # [n, 2] the geom pair whose contact makes q_hit invalid
    types: np.ndarray      # [n, 2] its geom types
    L: float

    def type_histogram(self):
        """{(type, type), smaller geom type first: rows}"""
        names = [tuple(TYPE_NAMES[t] for t in sorted((int(a), int(b)))) for a, b in self.types]
        return {k: names.count(k) for k in sorted(set(names))}


def lever_bound(model) -> float:
    """L of the module docstring."""
    norm = np.linalg.norm
    jnt_off = np.zeros(model.nbody)
    for j in range(model.njnt):
        b = int(model.jnt_bodyid[j])
        jnt_off[b] = max(jnt_off[b], norm(model.jnt_pos[j]))
    chain = np.zeros(model.nbody)
    for b in range(1, model.nbody):  # (parents come first)
        chain[b] = chain[int(model.body_parentid[b])] + norm(model.body_pos[b]) + jnt_off[b]
    moving = np.asarray(model.geom_bodyid) != 0
    reach = norm(np.asarray(model.geom_pos)[moving], axis=1) + np.asarray(model.geom_rbound)[moving]
    lever = chain.max() + reach.max()
    return float(model.nq * max(1.0, lever))


def sample_and_split(orc, model, qidx, n, rng, draws=DRAWS):
    lo, hi = model.jnt_range[qidx, 0], model.jnt_range[qidx, 1]
    Q = rng.uniform(lo, hi, size=(draws, len(qidx)))
    v = orc.valid_configs(Q, nthreads=8).astype(bool)
    assert v.sum() >= n and (~v).sum() >= n, f"{int(v.sum())} valid and {int((~v).sum())} invalid of {draws} draws: fewer than {n}"
    return Q[v][:n].copy(), Q[~v][:n].copy()


def bisect(orc, A, B):
    """-> (q_free, q_hit, t_free, t_hit): the oracle's verdict flips between adjacent doubles t of q(t) = A + t (B - A)."""
    D = B - A
    lo, hi = np.zeros(len(A)), np.ones(len(A))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        done = (mid == lo) | (mid == hi)
        if done.all():
            break
        v = orc.valid_configs(A + mid[:, None] * D, nthreads=8).astype(bool)
        lo = np.where(v & ~done, mid, lo)
        hi = np.where(~v & ~done, mid, hi)
    assert done.all(), "a row did not bisect down to adjacent values"
    assert (np.nextafter(lo, 1.0) == hi).all()
    q_free, q_hit = A + lo[:, None] * D, A + hi[:, None] * D
    assert orc.valid_configs(q_free, nthreads=8).all() and not orc.valid_configs(q_hit, nthreads=8).any()
    return q_free, q_hit, lo, hi


def adjacency_slack(A, B):
    """|q_hit - q_free| per coordinate is at most this: t moves by one ulp(t) <= 2^-53, times |B - A| <= 2 M with
    M = max(|A|, |B|), is at most 2 ulp(M); the product and the sum of q(t) each round once on either side, at most
    another 2 ulp(M)."""
    return 4.0 * np.spacing(np.maximum(np.abs(A), np.abs(B)))


def flipping_pairs(orc, model, allowed, qidx, base, q_hit):
    """Per row the first pair of Oracle.contacts at q_hit that no allowed body pair excuses (the list holds candidate
    pairs only: mj_collision's filters are applied by the oracle), and its geom types."""
    from oracle import pyoracle
    excused = {tuple(r) for r in pyoracle.sorted_allowed(model, list(allowed)).tolist()}
    bid = np.asarray(model.geom_bodyid)
    pairs = np.zeros((len(q_hit), 2), np.int32)
    for i, q in enumerate(q_hit):
        full = np.asarray(base, float).copy()
        full[qidx] = q
        con = [tuple(p) for p in orc.contacts(full).tolist()
               if tuple(sorted((int(bid[p[0]]), int(bid[p[1]])))) not in excused]
        assert con, f"row {i}: invalid without a contact that counts"
        pairs[i] = con[0]
    return pairs, np.asarray(model.geom_type)[pairs]


def _edges(orc, qa, qb, step):
    valid, fb, _ = orc.valid_edges(qa, qb, step, nthreads=8, info=True)
    return Edges(np.ascontiguousarray(qa), np.ascontiguousarray(qb), valid, fb)


def build(oracle_mod, model, allowed, qidx, base, n=ROWS, seed=1, offsets=OFFSETS, step=STEP, filler=FILLER) -> Cases:
    """Under the oracle's trig of the moment (oracle_mod.portable_trig() or libm's)."""
    qidx = np.asarray(qidx, np.int32)
    rng = np.random.default_rng(seed)
    orc = oracle_mod.Oracle(model, allowed, planning_qidx=qidx, qpos_base=base)
    A, B = sample_and_split(orc, model, qidx, n, rng)
    q_free, q_hit, _, _ = bisect(orc, A, B)
    assert (np.abs(q_hit - q_free) <= adjacency_slack(A, B)).all()
    D = B - A
    u = D / np.abs(D).max(axis=1, keepdims=True)
    e = D / np.linalg.norm(D, axis=1, keepdims=True)
    L = lever_bound(model)
    rows, off, side = [], [], []
    for o in offsets:
        for q, s in ((q_free, -1.0), (q_hit, +1.0)):
            rows.append(q + s * o * u)
            off.append(np.full(n, o))
            side.append(np.full(n, s > 0))
    Q = np.ascontiguousarray(np.concatenate(rows))
    off, side = np.concatenate(off), np.concatenate(side)
    row = np.tile(np.arange(n), 2 * len(offsets))
    U, E = u[row], e[row]
    # (a) ends on the probe
    ending = _edges(orc, Q - 3.5 * step * U, Q, step)
    # (b) through the probe, five steps long.  An edge's steps are `step` long in the 2-norm, so it runs along the line's
    # 2-norm unit vector e for a waypoint to fall on the probe.  It runs from the contact side to the free side, the probe
    # its FIRST waypoint (the start of an edge is never checked): run the other way, with the probe three steps in and two
    # more towards B, it would end inside the contact for all but the thinnest contact regions -- "invalid, first bad 0"
    # whatever the probe's verdict, and no waypoint would ever decide an edge.  Here the probe decides: first bad is 1
    # where it is invalid, and the four checks behind it lie on the free side.
    through = _edges(orc, Q + 1.0 * step * E, Q - 4.0 * step * E, step)
    # (c) one to five steps in a random direction from a valid configuration: mostly free, for a certificate to certify
    d = rng.normal(size=(filler, len(qidx)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fa = A[rng.integers(0, n, size=filler)]
    fill = _edges(orc, fa, fa + rng.uniform(1.0, 5.0, size=(filler, 1)) * step * d, step)
    pairs, types = flipping_pairs(orc, model, allowed, qidx, base, q_hit)
    return Cases(A, B, q_free, q_hit, u, np.asarray(offsets, float), Q, off, side, row, L * off <= NEAR_METRES,
                 orc.valid_configs(Q, nthreads=8), ending, through, fill, pairs, types, L)
