"""Certified edge checks as a ``collision_interval_check`` constraint.

``collision_interval_check=(step, constraint)`` makes ``RRT``, ``smooth_path`` and ``cartesian_plan`` ask
``constraint.valid_interval(start, end, step)`` for every edge.  A ``CollisionConstraint`` answers from waypoints
``step`` apart; wrapped in ``CertifiedIntervals`` it answers for the whole segment (``mjpl_sweep_edges``: free bubbles
and bisection), so a thin obstacle between two waypoints cannot be stepped over.  Wrapping a
``ClearanceConstraint`` asks for its ``min_clearance`` all along the edge.  An edge the depth budget leaves undecided
counts as invalid.
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine


class CertifiedIntervals:
    """Args:
        constraint: a ``CollisionConstraint`` or ``ClearanceConstraint`` (anything with ``certified_intervals``).
        params: passed on to every call (cap, max_depth, lo, hi; for a ``CollisionConstraint`` also d_min).
    """

    def __init__(self, constraint, **params) -> None:
        if not hasattr(constraint, "certified_intervals"):
            raise TypeError("`constraint` must offer certified_intervals (CollisionConstraint, ClearanceConstraint)")
        self.constraint = constraint
        self.params = params

    def valid_interval(self, start: np.ndarray, end: np.ndarray, step_dist: float) -> bool:
        return bool(self.valid_intervals(np.asarray(start, dtype=np.float64)[None, :],
                                         np.asarray(end, dtype=np.float64)[None, :], step_dist)[0])

    def valid_intervals(self, starts: np.ndarray, ends: np.ndarray, step_dist: float) -> np.ndarray:
        """Full-nq edges [N, nq] -> bool [N]: status == SWEEP_FREE.  ``step_dist`` plays no part beyond being > 0."""
        if step_dist <= 0.0:
            raise ValueError("`step_dist` must be > 0")
        return self.constraint.certified_intervals(starts, ends, **self.params)[0] == _engine.SWEEP_FREE

    def __getattr__(self, name):  # (valid_config, apply, ... : the wrapped constraint's)
        return getattr(self.constraint, name)
