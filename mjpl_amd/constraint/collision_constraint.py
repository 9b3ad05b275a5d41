"""Collision constraint backed by the MI355X engine -- the drop-in for
``mjpl.CollisionConstraint`` (reference src/mjpl/constraint/collision_constraint.py:8-33).

Scalar ``valid_config`` / ``apply`` keep the reference's semantics exactly (full-nq ``q``,
``apply`` returns the same array object or None), so an instance can be handed to the
reference-shaped planners unchanged, also as the ``collision_interval_check`` constraint
(rrt.py:28, planning/utils.py:12,110).  The batched methods are what the hot path is for.

There is no CPU fallback: constructing one without the HIP library or without a gfx950
device raises.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .. import engine as _engine
from .constraint_interface import Constraint


def contact_hits(bits: np.ndarray, npairs: int) -> np.ndarray:
    """Contact words [N, W] (uint64; bit p % 64 of word p // 64 = candidate pair p touches) -> bool [N, npairs]."""
    bits = np.ascontiguousarray(bits, dtype="<u8")
    if bits.ndim != 2 or bits.shape[1] != (npairs + 63) // 64:
        raise ValueError(f"contact words must be [N, {(npairs + 63) // 64}] for {npairs} candidate pairs, got {bits.shape}")
    flat = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little") if bits.size else \
        np.zeros((bits.shape[0], 64 * bits.shape[1]), np.uint8)
    return flat[:, :npairs].astype(bool)


def contact_csr(bits: np.ndarray, pairs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Contact words [N, W] and the candidate table pairs [P, 2] -> (offsets int64 [N + 1], rows int32 [M, 2]):
    configuration i's contacts are rows[offsets[i]:offsets[i + 1]], in candidate-table order."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    hit = contact_hits(bits, len(pairs))
    offsets = np.zeros(hit.shape[0] + 1, np.int64)
    np.cumsum(hit.sum(axis=1), out=offsets[1:])
    _, p = np.nonzero(hit)  # row-major: configuration by configuration, pairs in table order
    return offsets, pairs[p]


class ClearanceGradient(NamedTuple):
    """One configuration's clearance with its gradient (``CollisionConstraint.clearance_gradient``)."""
    clearance: float                   # min over non-allowed pairs of distance - margin (distmax if none)
    pair: tuple[int, int] | None       # the geom pair attaining it (smaller geom type first), None if none
    gradient: np.ndarray               # dC/dq, float64 [nq]
    fromto: np.ndarray                 # witness points w1 (on pair[0]), w2 (on pair[1]), world frame, float64 [6]
    normal: np.ndarray                 # unit vector from pair[0] towards pair[1], float64 [3]
    status: int                        # engine.GRAD_OK / GRAD_FLAT / GRAD_DEGENERATE / GRAD_NONFINITE


class NearPair(NamedTuple):
    """One geom pair closer than distmax at a configuration (``CollisionConstraint.near_pairs``)."""
    pair: tuple[int, int]              # the geom pair (smaller geom type first)
    distance: float                    # its signed distance (margins not subtracted)
    gradient: np.ndarray               # d distance / dq, float64 [nq]
    fromto: np.ndarray                 # witness points w1 (on pair[0]), w2 (on pair[1]), world frame, float64 [6]
    normal: np.ndarray                 # unit vector from pair[0] towards pair[1], float64 [3]
    status: int                        # engine.GRAD_OK / GRAD_DEGENERATE


class CertifiedEdge(NamedTuple):
    """One edge decided as a whole (``CollisionConstraint.certified_interval``)."""
    status: int                        # engine.SWEEP_FREE / SWEEP_HIT / SWEEP_UNDECIDED / SWEEP_NONFINITE / SWEEP_RANGE
    t_hit: float                       # where a configuration in contact was found (NaN unless HIT)
    clear_lb: float                    # clearance >= this all along the edge (NaN unless FREE)
    pair: tuple[int, int] | None       # the closest geom pair at t_hit (None unless HIT)
    nodes: int                         # bubble measurements spent
    depth: int                         # deepest bisection depth evaluated


class CertifiedPath(NamedTuple):
    """One path's spline decided as a whole (``CollisionConstraint.certified_spline``)."""
    status: int                        # engine.SWEEP_*: HIT if any piece is, else RANGE / NONFINITE, else UNDECIDED, else FREE
    piece: int                         # the lowest piece with that status (-1 when the path is FREE)
    s_hit: float                       # (piece + t_hit) / (n - 1) where the spline is in contact or leaves the bounds (else NaN)
    q_hit: np.ndarray | None           # the configuration there, full nq (None where s_hit is NaN)
    clear_lb: float                    # clearance >= this all along the spline (NaN unless FREE)
    pair: tuple[int, int] | None       # the closest geom pair at s_hit (None unless HIT)
    nodes: int                         # bubble measurements spent on the path
    piece_status: np.ndarray           # engine.SWEEP_* of every piece, int32 [n - 1]


def spline_piece_point(W: np.ndarray, M: np.ndarray, k: int, B: float) -> np.ndarray:
    """q_k(B): piece k of the natural cubic spline through W [n, d] with knot second derivatives M, at the local
    coordinate B in [0, 1] (include/mjpl_hip.h, mjpl_sweep_splines)."""
    r = float(len(W) - 1)
    A = 1.0 - B
    return (A * W[k] + B * W[k + 1]) + ((A * A * A - A) * M[k] + (B * B * B - B) * M[k + 1]) / (6.0 * r * r)


class CollisionRuleset:
    """Which body pairs may touch (reference collision_constraint.py:36-95).

    The engine folds this rule into its static pair list; this class is the host-side
    statement of the same integer logic, for callers that hold a contact list already.
    """

    def __init__(self, model, allowed_collision_bodies: list[tuple[str, str]] = []) -> None:
        self.model = model
        self.allowed_collisions: np.ndarray | None = None
        if allowed_collision_bodies:
            ids = np.array([[model.body(a).id, model.body(b).id] for a, b in allowed_collision_bodies])
            ids.sort(axis=1)  # (a, b) and (b, a) name the same pair
            self.allowed_collisions = ids[None, :, :]
        self._allowed_set = set() if self.allowed_collisions is None else {
            (int(a), int(b)) for a, b in self.allowed_collisions[0]}

    def obeys_ruleset(self, collision_geometries: np.ndarray) -> bool:
        cg = np.asarray(collision_geometries)
        if cg.ndim != 2 or cg.shape[1] != 2:
            raise ValueError("`collision_geometries` must be a nx2 matrix.")
        if cg.shape[0] == 0:
            return True
        if not self._allowed_set:
            return False
        bodies = np.sort(np.asarray(self.model.geom_bodyid)[cg.astype(np.int64)], axis=1)
        return all((int(a), int(b)) in self._allowed_set for a, b in bodies)


class CollisionConstraint(Constraint):
    """Batched collision validation on one MI355X.

    Args:
        model: :class:`mjpl_amd.model.Model` (stands in for ``mujoco.MjModel``).
        allowed_collision_bodies: body-name pairs whose contacts never invalidate a
            configuration; empty means any contact invalidates (collision_constraint.py:86-88).
        device: HIP device ordinal.
    """

    projects = False  # apply() never moves a configuration: batched extension is allowed

    def __init__(self, model, allowed_collision_bodies: list[tuple[str, str]] = [],
                 device: int = 0) -> None:
        self.model = model
        self.cr = CollisionRuleset(model, allowed_collision_bodies)
        self.engine = _engine.Engine(model, allowed_collision_bodies, device=device)
        self._plan_idx = np.arange(model.nq, dtype=np.int32)
        self._plan_base = np.asarray(model.qpos0, dtype=np.float64).copy()
        self._full = True

    # ---- reference surface ---------------------------------------------------------
    def valid_config(self, q: np.ndarray) -> bool:
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (self.model.nq,):
            raise ValueError(f"q must have shape ({self.model.nq},)")
        self._ensure_full()
        return bool(self.engine.check_configs(q[None, :], _engine.AOS)[0])

    def apply(self, q_old: np.ndarray, q: np.ndarray) -> np.ndarray | None:
        return q if self.valid_config(q) else None

    # ---- batched surface -----------------------------------------------------------
    def set_planning(self, qidx, qpos_base) -> None:
        """Batches passed to the ``*_planning`` methods hold only these qpos columns; every
        other joint stays at ``qpos_base`` (planners keep them at q_init, rrt.py:205-206)."""
        self._plan_idx = np.asarray(qidx, dtype=np.int32).copy()
        self._plan_base = np.asarray(qpos_base, dtype=np.float64).copy()
        self._full = False
        self.engine.set_planning(self._plan_idx, self._plan_base)

    def _ensure_full(self):
        if not self._full:
            self.engine.set_planning(np.arange(self.model.nq, dtype=np.int32),
                                     np.asarray(self.model.qpos0, dtype=np.float64))
            self._full = True

    def _ensure_planning(self):
        if self._full:
            self.engine.set_planning(self._plan_idx, self._plan_base)
            self._full = False

    def valid_configs(self, Q: np.ndarray) -> np.ndarray:
        """Full-nq configurations [N, nq] -> bool [N]."""
        self._ensure_full()
        return self.engine.check_configs(np.asarray(Q, dtype=np.float64), _engine.AOS).astype(bool)

    # ---- contacts (``data.contact.geom``) ---------------------------------------------
    # Invariant: CollisionRuleset(model, allowed).obeys_ruleset(c.contacts(q)) == c.valid_config(q) for every q --
    # a pair's contact bit is the per-pair decision the collision check makes.
    def contacts(self, q: np.ndarray) -> np.ndarray:
        """The rows ``data.contact.geom`` holds after mj_kinematics + mj_collision at the full-nq ``q``:
        int32 [ncon, 2], one row per touching geom pair (allowed pairs included, as in MuJoCo's list),
        smaller geom type first, in the oracle's order.  Invariant:
        ``CollisionRuleset(model, allowed).obeys_ruleset(c.contacts(q)) == c.valid_config(q)``."""
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (self.model.nq,):
            raise ValueError(f"q must have shape ({self.model.nq},)")
        return self.contacts_batch(q[None, :])[1]

    def contacts_batch(self, Q: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """``contacts`` for every row of full-nq configurations [N, nq], one launch -> CSR (offsets int64 [N + 1],
        pairs int32 [M, 2]): row i's contacts are pairs[offsets[i]:offsets[i + 1]].  The same invariant holds row by
        row against ``valid_configs``."""
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.model.nq:
            raise ValueError(f"Q must have shape (N, {self.model.nq})")
        self._ensure_full()
        bits = self.engine.contacts(Q, _engine.AOS)
        return contact_csr(bits, self.engine.contact_pairs()[0])

    def colliding_bodies(self, q: np.ndarray, include_allowed: bool = False) -> list[tuple[str, str]]:
        """Which bodies touch at ``q``: sorted, distinct body-name pairs (each pair sorted by name).  Pairs of
        ``allowed_collision_bodies`` are left out unless ``include_allowed``: what remains is why ``valid_config(q)``
        is False (empty iff it is True)."""
        rows = self.contacts(q)
        bid = np.asarray(self.model.geom_bodyid)
        out = set()
        for g1, g2 in rows:
            b1, b2 = sorted((int(bid[g1]), int(bid[g2])))
            if not include_allowed and (b1, b2) in self.cr._allowed_set:
                continue
            out.add(tuple(sorted((self.model.body(b1).name, self.model.body(b2).name))))
        return sorted(out)

    # ---- distances and clearance (``data.contact.dist``, ``mj_geomDistance``) ----------------
    # Exact geometric signed distances (gap > 0, minus the penetration depth when overlapping, margins not
    # subtracted), per candidate pair of ``engine.contact_pairs()``; entries not below ``distmax`` read distmax.
    # Invariant: ``c.clearance(q)[0] > 0`` <=> ``c.valid_config(q)``, away from the threshold.
    def _full_batch(self, Q: np.ndarray) -> np.ndarray:
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.model.nq:
            raise ValueError(f"Q must have shape (N, {self.model.nq})")
        self._ensure_full()
        return Q

    def _full_q(self, q: np.ndarray) -> np.ndarray:
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (self.model.nq,):
            raise ValueError(f"q must have shape ({self.model.nq},)")
        return q[None, :]

    def pair_distances(self, q: np.ndarray, distmax: float = np.inf) -> np.ndarray:
        """Signed distance of every candidate pair at the full-nq ``q`` -> float64 [P] (allowed pairs included)."""
        return self.distances_batch(self._full_q(q), distmax)[0]

    def distances_batch(self, Q: np.ndarray, distmax: float = np.inf) -> np.ndarray:
        """``pair_distances`` for every row of full-nq configurations [N, nq], one launch -> float64 [N, P]."""
        return self.engine.distances(self._full_batch(Q), distmax, _engine.AOS)

    def clearance(self, q: np.ndarray, distmax: float = np.inf) -> tuple[float, tuple[int, int] | None]:
        """How far ``q`` is from being invalid: (min over non-allowed pairs of distance - margin, the geom pair
        attaining it, smaller geom type first), or (distmax, None) if no pair counts.  Invariant:
        ``clearance(q)[0] > 0`` <=> ``valid_config(q)``, away from the threshold."""
        C, pair = self.clearance_batch(self._full_q(q), distmax)
        if pair[0] < 0:
            return float(C[0]), None
        g1, g2 = self.engine.contact_pairs()[0][pair[0]]
        return float(C[0]), (int(g1), int(g2))

    def clearance_batch(self, Q: np.ndarray, distmax: float = np.inf) -> tuple[np.ndarray, np.ndarray]:
        """``clearance`` for every row of [N, nq], one launch -> (C float64 [N], candidate-pair index int32 [N],
        -1 for none).  The same invariant holds row by row against ``valid_configs``."""
        return self.engine.clearance(self._full_batch(Q), distmax, _engine.AOS)

    # ---- clearance gradients and witness points (``mj_geomDistance``'s fromto, dC/dq) ------------
    def clearance_gradient(self, q: np.ndarray, distmax: float = np.inf) -> "ClearanceGradient":
        """The clearance at the full-nq ``q`` with its gradient over nq, witness points and normal ->
        :class:`ClearanceGradient`.  ``clearance_gradient(q).clearance == clearance(q)[0]`` bit for bit, and ``pair``
        is ``clearance(q)[1]`` (g1, g2; fromto[:3] lies on g1, fromto[3:] on g2, normal points from g1 to g2).
        Where the closest pair or feature switches, the gradient is the one-sided one of the pair picked."""
        C, pair, grad, fromto, normal, status = self.clearance_gradient_batch(self._full_q(q), distmax)
        geoms = None
        if pair[0] >= 0:
            g1, g2 = self.engine.contact_pairs()[0][pair[0]]
            geoms = (int(g1), int(g2))
        return ClearanceGradient(float(C[0]), geoms, grad[0], fromto[0], normal[0], int(status[0]))

    def clearance_gradient_batch(self, Q: np.ndarray, distmax: float = np.inf):
        """``clearance_gradient`` for every row of full-nq configurations [N, nq], one launch -> (C [N], candidate-pair
        index [N], grad [N, nq], fromto [N, 6], normal [N, 3], status [N]); C and pair equal clearance_batch's."""
        return self.engine.clearance_grad(self._full_batch(Q), distmax, _engine.AOS)

    def clearance_gradient_planning(self, Qp: np.ndarray, distmax: float = np.inf, layout: int = _engine.AOS):
        """``clearance_gradient_batch`` over the columns of ``set_planning`` (every other joint at its base value):
        grad is [N, nplan], dC/dq over those columns; C and pair equal what a full-nq batch gives there."""
        self._ensure_planning()
        return self.engine.clearance_grad(Qp, distmax, layout)

    # ---- near pairs: every pair within distmax, each with its own distance, witnesses and gradient ----------
    def near_pairs(self, q: np.ndarray, distmax: float) -> "list[NearPair]":
        """Every non-allowed candidate pair whose signed distance at the full-nq ``q`` is below ``distmax``, in
        candidate-table order -> a list of :class:`NearPair`.  ``distance`` is ``pair_distances(q)``'s entry bit for
        bit; ``gradient`` is that pair's own d distance / dq (where ``clearance_gradient`` follows one pair and flips
        where the closest pair switches, this lists each pair with its own).  Nothing is cut: the slots are sized to
        the number of non-allowed pairs.  A non-finite ``q`` raises ValueError (the batch forms report count -1)."""
        pairs, allowed = self.engine.contact_pairs()
        K = max(int((~allowed).sum()), 1)
        count, pair, dist, grad, fromto, normal, status = self.near_pairs_batch(self._full_q(q), distmax, K)
        if count[0] < 0:
            raise ValueError("q holds a non-finite value")
        return [NearPair((int(pairs[p][0]), int(pairs[p][1])), float(dist[0, k]), grad[0, k], fromto[0, k], normal[0, k],
                         int(status[0, k])) for k, p in enumerate(pair[0, :count[0]])]

    def near_pairs_batch(self, Q: np.ndarray, distmax: float, max_pairs: int = 32):
        """``near_pairs`` for every row of full-nq configurations [N, nq], one launch, K = max_pairs slots per row ->
        (count [N], candidate-pair index [N, K], dist [N, K], grad [N, K, nq], fromto [N, K, 6], normal [N, K, 3],
        status [N, K]).  count is not clipped to K (-1: non-finite row); slots past min(count, K) read -1 / NaN."""
        return self.engine.near_pairs(self._full_batch(Q), distmax, max_pairs, _engine.AOS)

    def near_pairs_planning(self, Qp: np.ndarray, distmax: float, max_pairs: int = 32, layout: int = _engine.AOS):
        """``near_pairs_batch`` over the columns of ``set_planning`` (every other joint at its base value): grad is
        [N, K, nplan], over those columns."""
        self._ensure_planning()
        return self.engine.near_pairs(Qp, distmax, max_pairs, layout)

    def valid_interval(self, start: np.ndarray, end: np.ndarray, step_dist: float) -> bool:
        """``_valid_collision_interval(start, end, step_dist, self)`` in one launch
        (planning/utils.py:188-216): interior waypoints only."""
        if step_dist <= 0.0:
            raise ValueError("`step_dist` must be > 0")
        self._ensure_full()
        v = self.engine.check_edges(np.asarray(start, float)[None, :], np.asarray(end, float)[None, :],
                                    step_dist, _engine.AOS, interior_only=True)
        return bool(v[0])

    def valid_intervals(self, starts: np.ndarray, ends: np.ndarray, step_dist: float) -> np.ndarray:
        """Row-wise ``valid_interval``: full-nq edges [N, nq] -> bool [N], one launch."""
        if step_dist <= 0.0:
            raise ValueError("`step_dist` must be > 0")
        self._ensure_full()
        return self.engine.check_edges(np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64),
                                       step_dist, _engine.AOS, interior_only=True).astype(bool)

    # ---- certified edge checks: the whole segment, not samples of it (include/mjpl_hip.h, mjpl_sweep_edges) --------
    def certified_interval(self, start: np.ndarray, end: np.ndarray, d_min: float = 0.0, **params) -> "CertifiedEdge":
        """The straight segment between two full-nq configurations, decided as a whole -> :class:`CertifiedEdge`.
        ``status == engine.SWEEP_FREE``: no configuration of it is in contact (or nearer than ``d_min``), whatever lies
        between two waypoints of ``valid_interval``.  params: cap, max_depth, lo, hi (full nq; a model with slide
        joints needs finite bounds for them)."""
        status, t_hit, clear_lb, pair, nodes, depth = self.certified_intervals(
            self._full_q(start), self._full_q(end), d_min, **params)
        geoms = None
        if pair[0] >= 0:
            g1, g2 = self.engine.contact_pairs()[0][pair[0]]
            geoms = (int(g1), int(g2))
        return CertifiedEdge(int(status[0]), float(t_hit[0]), float(clear_lb[0]), geoms, int(nodes[0]), int(depth[0]))

    def certified_intervals(self, starts: np.ndarray, ends: np.ndarray, d_min: float = 0.0, **params):
        """``certified_interval`` for every row of full-nq edges [N, nq], one call -> (status [N], t_hit [N], clear_lb
        [N], candidate-pair index [N], nodes [N], depth [N])."""
        return self.engine.sweep_edges(self._full_batch(starts), self._full_batch(ends), d_min, _engine.AOS, **params)

    def certified_edges_planning(self, QA: np.ndarray, QB: np.ndarray, d_min: float = 0.0, layout: int = _engine.AOS,
                                 **params):
        """``certified_intervals`` over the columns of ``set_planning`` (every other joint at its base value; lo / hi
        over those columns)."""
        self._ensure_planning()
        return self.engine.sweep_edges(QA, QB, d_min, layout, **params)

    # ---- certified trajectories: the whole spline, not its samples (include/mjpl_hip.h, mjpl_sweep_splines) --------
    def certified_spline(self, waypoints, d_min: float = 0.0, **params) -> "CertifiedPath":
        """The natural cubic spline through full-nq ``waypoints`` -- the curve ``HipToppTrajectoryGenerator`` moves
        along -- decided as a whole -> :class:`CertifiedPath`.  ``status == engine.SWEEP_FREE``: no configuration of it is
        in contact (or nearer than ``d_min``), whatever lies between two samples of a trajectory.  params: cap,
        max_depth, lo, hi (full nq)."""
        return self.certified_splines([waypoints], d_min, **params)[0]

    def certified_splines(self, paths, d_min: float = 0.0, **params) -> "list[CertifiedPath]":
        """``certified_spline`` for every path (each a sequence of at least two full-nq configurations), one call."""
        packed = [self._full_batch(np.array([np.asarray(w, dtype=np.float64).reshape(-1) for w in p])) for p in paths]
        if not packed:
            return []
        if any(len(W) < 2 for W in packed):
            raise ValueError("every path needs at least two waypoints")
        off = np.concatenate([[0], np.cumsum([len(W) for W in packed])]).astype(np.int64)
        status, t_hit, clear_lb, pair, nodes, _depth, M = self.engine.sweep_splines(np.concatenate(packed), off, d_min, **params)
        cand = self.engine.contact_pairs()[0]
        out = []
        for b, W in enumerate(packed):
            p = slice(int(off[b]) - b, int(off[b + 1]) - b - 1)
            st, Mb = status[p], M[off[b]:off[b + 1]]
            verdict, k = _engine.SWEEP_FREE, -1
            for group in ((_engine.SWEEP_HIT,), (_engine.SWEEP_RANGE, _engine.SWEEP_NONFINITE), (_engine.SWEEP_UNDECIDED,)):
                at = np.flatnonzero(np.isin(st, group))
                if len(at):
                    k = int(at[0])
                    verdict = int(st[k])
                    break
            s_hit, q_hit, geoms, lb = float("nan"), None, None, float("nan")
            if k >= 0 and np.isfinite(t_hit[p][k]):
                tk = float(t_hit[p][k])
                s_hit = (k + tk) / (len(W) - 1)
                q_hit = W[k].copy() if tk == 0.0 else W[k + 1].copy() if tk == 1.0 else spline_piece_point(W, Mb, k, tk)
                if pair[p][k] >= 0:
                    geoms = tuple(int(g) for g in cand[pair[p][k]])
            if verdict == _engine.SWEEP_FREE:
                lb = float(clear_lb[p].min())
            out.append(CertifiedPath(verdict, k, s_hit, q_hit, lb, geoms, int(nodes[p].sum()), st.copy()))
        return out

    def valid_configs_planning(self, Q: np.ndarray, layout: int = _engine.AOS) -> np.ndarray:
        self._ensure_planning()
        return self.engine.check_configs(Q, layout).astype(bool)

    def valid_edges_planning(self, QA: np.ndarray, QB: np.ndarray, step_dist: float,
                             layout: int = _engine.AOS, first_bad: bool = False,
                             interior_only: bool = False):
        """Validated edges (endpoint + interior waypoints) over planning columns."""
        if step_dist <= 0.0:
            raise ValueError("`step_dist` must be > 0")
        self._ensure_planning()
        r = self.engine.check_edges(QA, QB, step_dist, layout, first_bad=first_bad,
                                    interior_only=interior_only)
        return (r[0].astype(bool), r[1]) if first_bad else r.astype(bool)
