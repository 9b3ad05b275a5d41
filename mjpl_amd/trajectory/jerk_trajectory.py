"""Jerk-limited trajectories under velocity, acceleration and jerk limits, batched on the GPU.

Stands where the reference has ``RuckigTrajectoryGenerator`` (src/mjpl/trajectory/ruckig_trajectory.py): the trajectory
passes through the waypoints without stopping and every joint's velocity, acceleration and jerk stay within their limits
at every instant.  The path is the natural cubic spline of ``HipToppTrajectoryGenerator``; the parameterisation is a
junction-speed lookahead with jerk-limited S-curve ramps inside every grid interval.  include/mjpl_hip.h
(mjpl_jerk_profile) states it, DESIGN.md 5.14 proves the guarantee.  It is not time-optimal.
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from .topp_trajectory import sample_count
from .trajectory_interface import Trajectory, TrajectoryGenerator


class HipJerkTrajectoryGenerator(TrajectoryGenerator):
    # every position of a trajectory lies on the natural cubic spline through the waypoints at uniform knots: the curve
    # ``certified_splines`` decides (``generate_certified_trajectories`` asks for this declaration)
    follows_natural_spline = True

    def __init__(self, dt: float, max_velocity, max_acceleration, max_jerk, min_velocity=None, min_acceleration=None,
                 grid_per_segment: int = 2, engine: "_engine.Engine | None" = None, device: int = 0,
                 allow_repeated_waypoints: bool = False) -> None:
        """``min_velocity`` / ``min_acceleration`` default to the negated maxima.  The parameterisation works with one
        magnitude per column and limit, ``min(max, -min)``: where the minima are not the negated maxima this is
        conservative (the tighter side binds in both directions), never a violation.  Jerk is limited to
        ``[-max_jerk, max_jerk]``, as in the reference.  ``grid_per_segment``: grid intervals per waypoint segment; 2
        gave durations 3-8 % shorter than 1 on the four paths of the prototype, which is the whole basis of the default.
        ``engine``, ``device`` and ``allow_repeated_waypoints`` are ``HipToppTrajectoryGenerator``'s; a path that does
        not move at all ends TOPP_STALLED and gives None."""
        if not dt > 0:
            raise ValueError("`dt` must be > 0.")
        if grid_per_segment < 1:
            raise ValueError("`grid_per_segment` must be >= 1.")
        self.dt = float(dt)
        self.vmax = np.array(max_velocity, dtype=np.float64).reshape(-1)
        self.amax = np.array(max_acceleration, dtype=np.float64).reshape(-1)
        self.jmax = np.array(max_jerk, dtype=np.float64).reshape(-1)
        self.vmin = -self.vmax if min_velocity is None else np.array(min_velocity, dtype=np.float64).reshape(-1)
        self.amin = -self.amax if min_acceleration is None else np.array(min_acceleration, dtype=np.float64).reshape(-1)
        nq = len(self.vmax)
        if not (len(self.amax) == len(self.jmax) == len(self.vmin) == len(self.amin) == nq):
            raise ValueError("the limits must have one entry per column of the waypoints.")
        if not (np.all(self.vmin < 0) and np.all(self.vmax > 0) and np.all(self.amin < 0) and np.all(self.amax > 0)):
            raise ValueError("limits must satisfy min < 0 < max in every column.")
        if not np.all(self.jmax > 0):
            raise ValueError("`max_jerk` must be > 0 in every column.")
        self.vlim = np.minimum(self.vmax, -self.vmin)
        self.alim = np.minimum(self.amax, -self.amin)
        self.grid = int(grid_per_segment)
        self.device = device
        self._engine = engine
        self.allow_repeated_waypoints = bool(allow_repeated_waypoints)

    @property
    def engine(self) -> "_engine.Engine":
        if self._engine is None:
            from .. import scenes
            self._engine = _engine.Engine(scenes.one_dof_ball(), device=self.device)
        return self._engine

    def _pack(self, paths):
        rows, off = [], [0]
        for k, path in enumerate(paths):
            W = np.array([np.asarray(w, dtype=np.float64).reshape(-1) for w in path], dtype=np.float64)
            if W.ndim != 2 or len(W) < 2:
                raise ValueError(f"path {k}: there must be at least two waypoints.")
            if W.shape[1] != len(self.vmax):
                raise ValueError(f"path {k}: waypoints have {W.shape[1]} columns, the limits {len(self.vmax)}.")
            if not self.allow_repeated_waypoints and np.any(np.all(W[1:] == W[:-1], axis=1)):
                raise ValueError(f"path {k}: two consecutive waypoints are equal.")
            rows.append(W)
            off.append(off[-1] + len(W))
        W = np.concatenate(rows) if rows else np.zeros((0, len(self.vmax)))
        return W, np.array(off, dtype=np.int64)

    def _profile(self, paths):
        W, wp_off = self._pack(paths)
        *prof, status = self.engine.jerk_profile(W, wp_off, self.vlim, self.alim, self.jmax, grid=self.grid)
        g_off = self.engine.topp_offsets(wp_off, self.grid)[1]
        T = prof[-1][g_off[1:] - 1] if len(wp_off) > 1 else np.zeros(0)
        return W, wp_off, prof, status, T

    def durations(self, paths) -> np.ndarray:
        """The duration of every path's motion (NaN where none exists): one launch sequence for the whole batch."""
        paths = list(paths)
        if not paths:
            return np.zeros(0)
        _, _, _, status, T = self._profile(paths)
        return np.where(status == _engine.TOPP_OK, T, np.nan)

    def generate_trajectories(self, paths) -> list[Trajectory | None]:
        """One trajectory per path (None where the path does not move or a waypoint is not finite): the whole batch is
        parameterised in one launch sequence and sampled in a second."""
        paths = list(paths)
        if not paths:
            return []
        W, wp_off, prof, status, T = self._profile(paths)
        ok = status == _engine.TOPP_OK
        counts = np.array([sample_count(T[b], self.dt) if ok[b] else 0 for b in range(len(paths))], dtype=np.int64)
        samp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pos, vel, acc = self.engine.jerk_sample(W, wp_off, *prof, self.dt, samp_off, self.vlim, self.alim, self.jmax,
                                                grid=self.grid)
        out: list[Trajectory | None] = []
        for b in range(len(paths)):
            if not ok[b] or counts[b] == 0:
                out.append(None)
                continue
            s = slice(samp_off[b], samp_off[b + 1])
            out.append(Trajectory(self.dt, W[wp_off[b]].copy(), list(pos[s]), list(vel[s]), list(acc[s])))
        return out

    def generate_trajectory(self, waypoints) -> Trajectory | None:
        return self.generate_trajectories([waypoints])[0]
