"""A safety margin as a constraint: every configuration at least ``min_clearance`` from everything.

``CollisionConstraint`` gives a verdict; this constraint also repairs.  ``valid_config`` asks whether the clearance
(min over non-allowed pairs of distance - margin) is at least ``min_clearance``; ``apply`` pushes a configuration that
is too close out to that clearance with ``mjpl_push_out`` (include/mjpl_hip.h: damped least-squares steps on the near
pairs' own gradients), so it *projects*: planners extend one lane at a time through it, as through a
``PoseConstraint``.

It shares the collision constraint's engine -- one engine per model -- and its full / planning switch.  There is no
CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from .collision_constraint import CollisionConstraint
from .constraint_interface import Constraint


class ClearanceConstraint(Constraint):
    """Args:
        collision: the model's :class:`CollisionConstraint`; its engine and allowed pairs are used.
        min_clearance: the clearance every valid configuration has at least (> 0, metres).
        overshoot, damping, step_max, max_iter, max_pairs: the parameters of ``mjpl_push_out``.
        lower, upper: optional bounds over the full nq the push clamps to (e.g. the joint ranges).
    """

    projects = True  # apply() moves a configuration

    def __init__(self, collision: CollisionConstraint, min_clearance: float, *, overshoot: float = 1e-3,
                 damping: float = 1e-4, step_max: float = 0.2, max_iter: int = 16, max_pairs: int = 16,
                 lower=None, upper=None) -> None:
        if not min_clearance > 0:
            raise ValueError("`min_clearance` must be > 0")
        self.collision = collision
        self.model = collision.model
        self.engine = collision.engine
        self.min_clearance = float(min_clearance)
        self.params = dict(overshoot=overshoot, damping=damping, step_max=step_max, max_iter=max_iter,
                           max_pairs=max_pairs)
        nq = self.model.nq
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64).copy()
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64).copy()
        for b in (self.lower, self.upper):
            if b is not None and b.shape != (nq,):
                raise ValueError(f"bounds must have shape ({nq},)")
        # D* = min_clearance + the largest margin of a non-allowed pair: the distmax of every measurement
        pairs, allowed = self.engine.contact_pairs()
        margin = np.asarray(self.model.geom_margin, dtype=np.float64)
        free = pairs[~allowed]
        self.distmax = self.min_clearance + (float(np.maximum(margin[free[:, 0]], margin[free[:, 1]]).max())
                                             if len(free) else 0.0)

    # ---- reference surface ---------------------------------------------------------
    def valid_config(self, q: np.ndarray) -> bool:
        return bool(self.collision.clearance(q, self.distmax)[0] >= self.min_clearance)

    def apply(self, q_old: np.ndarray, q: np.ndarray) -> np.ndarray | None:
        """``q`` itself when it already holds; otherwise a new array, ``q`` pushed out, when the push ends PUSH_OK;
        otherwise None."""
        if self.valid_config(q):
            return q
        out, _clear, _pair, _iters, status = self.apply_batch(np.asarray(q, dtype=np.float64)[None, :])
        return out[0] if status[0] == _engine.PUSH_OK else None

    # ---- batched surface -----------------------------------------------------------
    def valid_configs(self, Q: np.ndarray) -> np.ndarray:
        """Full-nq configurations [N, nq] -> bool [N]."""
        return self.collision.clearance_batch(Q, self.distmax)[0] >= self.min_clearance

    def apply_batch(self, Q: np.ndarray):
        """Every row of full-nq configurations [N, nq] pushed out, one call -> (Q_out [N, nq], clear [N], candidate-pair
        index [N], iters [N], status [N]: engine.PUSH_*).  Rows that hold already come back byte for byte."""
        Q = self.collision._full_batch(Q)
        return self.engine.push_out(Q, self.min_clearance, _engine.AOS, lo=self.lower, hi=self.upper, **self.params)

    def apply_planning(self, Qp: np.ndarray, layout: int = _engine.AOS):
        """``apply_batch`` over the columns of the collision constraint's ``set_planning`` (every other joint at its
        base value); the bounds are ``lower`` / ``upper`` in those columns."""
        self.collision._ensure_planning()
        idx = self.collision._plan_idx
        lo = None if self.lower is None else self.lower[idx]
        hi = None if self.upper is None else self.upper[idx]
        return self.engine.push_out(Qp, self.min_clearance, layout, lo=lo, hi=hi, **self.params)

    # ---- the edge form: the margin between the nodes too (include/mjpl_hip.h, mjpl_sweep_edges) --------------------
    def certified_interval(self, start: np.ndarray, end: np.ndarray, **params):
        """The segment between two full-nq configurations with ``d_min = min_clearance`` and this constraint's bounds
        -> ``CertifiedEdge``: ``status == engine.SWEEP_FREE`` iff every configuration of it keeps the clearance."""
        return self.collision.certified_interval(start, end, self.min_clearance, **self._sweep_params(params))

    def certified_intervals(self, starts: np.ndarray, ends: np.ndarray, **params):
        """Row-wise ``certified_interval`` over full-nq edges [N, nq], one call."""
        return self.collision.certified_intervals(starts, ends, self.min_clearance, **self._sweep_params(params))

    # ---- the trajectory form: the margin all along the spline (include/mjpl_hip.h, mjpl_sweep_splines) ------------
    def certified_spline(self, waypoints, **params):
        """The natural cubic spline through full-nq ``waypoints`` with ``d_min = min_clearance`` and this constraint's
        bounds -> ``CertifiedPath``: ``status == engine.SWEEP_FREE`` iff every configuration of it keeps the clearance."""
        return self.collision.certified_spline(waypoints, self.min_clearance, **self._sweep_params(params))

    def certified_splines(self, paths, **params):
        """``certified_spline`` for every path, one call."""
        return self.collision.certified_splines(paths, self.min_clearance, **self._sweep_params(params))

    def _sweep_params(self, params: dict) -> dict:
        out = dict(lo=self.lower, hi=self.upper)
        out.update(params)
        return out
