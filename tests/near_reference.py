"""Independent NumPy float64 statement of the near-pair list (include/mjpl_hip.h: mjpl_near_pairs*), on top of
tests/distance_reference.py (the signed distances) and tests/gradient_reference.py (the gradient of a listed pair):

* near_pairs: per configuration, the non-allowed candidate pairs whose reference distance is below distmax, in
  ascending candidate index, with that distance.
* central_differences: d D[i, p] / d q_j of ANY distance function of a batch (the reference's, or the engine's
  mjpl_distances) at steps h and h / 2, from one evaluation of the four perturbed batches.

Nothing of the product's kernels is used.
"""
import numpy as np

import distance_reference as ref
import gradient_reference as gref  # noqa: F401  (the gradient of a listed pair: gref.clearance_gradient)


def near_pairs(model, Q, pairs, allowed, distmax, D=None):
    """Full-nq Q [N, nq], candidate pairs [P, 2], allowed flags [P] -> (rows, D): rows[i] = (p, d) with p the
    ascending candidate indices of the non-allowed pairs with D[i, p] < distmax and d = D[i, p]; D [N, P] the
    reference distances (computed here unless given)."""
    D = ref.reference_distances(model, Q, pairs) if D is None else D
    free = ~np.asarray(allowed, bool)
    rows = []
    for i in range(len(D)):
        p = np.flatnonzero(free & (D[i] < distmax))
        rows.append((p.astype(np.int32), D[i, p]))
    return rows, D


def flatten(rows):
    """rows of near_pairs -> (row index [M], candidate index [M], distance [M]) over all listed entries"""
    i = np.concatenate([np.full(len(p), k, np.int64) for k, (p, _) in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    p = np.concatenate([p for p, _ in rows]) if rows else np.zeros(0, np.int32)
    d = np.concatenate([d for _, d in rows]) if rows else np.zeros(0)
    return i, p, d


def central_differences(distances, Q, h):
    """distances: batch [M, nq] -> D [M, P].  Returns (fd_h, fd_h2), each [N, nq, P]: the central difference of every
    pair's distance in every column at step h and at h / 2, from one call on the 4 * nq * N perturbed rows."""
    Q = np.asarray(Q, float)
    n, nq = Q.shape
    steps = np.array([h, -h, h / 2, -h / 2])
    S = np.repeat(Q[:, None, None, :], 4, axis=1).repeat(nq, axis=2)  # [N, 4, nq, nq]
    for j in range(nq):
        S[:, :, j, j] += steps[None, :]
    D = np.asarray(distances(S.reshape(-1, nq)))
    D = D.reshape(n, 4, nq, -1)
    return (D[:, 0] - D[:, 1]) / (2 * h), (D[:, 2] - D[:, 3]) / h
