"""Time-optimal trajectories under velocity and acceleration limits, batched on the GPU.

Stands where the reference has ``ToppraTrajectoryGenerator`` (src/mjpl/trajectory/toppra_trajectory.py): the path is
a cubic spline through the waypoints at uniform knots, the parameterisation is TOPP-RA's backward and forward sweep
with the acceleration limits collocated at both ends of every grid interval, the motion between grid points has
constant path acceleration.  include/mjpl_hip.h (mjpl_topp_profile) states it; jerk is not limited.
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from .trajectory_interface import Trajectory, TrajectoryGenerator


def sample_count(duration: float, dt: float) -> int:
    """States ``dt`` apart and a last one at the duration itself; a tail shorter than 1e-8 is dropped (the reference's
    ``np.arange(dt, T, dt)`` with T appended unless the last entry is within 1e-8 of it)."""
    return max(int(np.ceil((float(duration) - 1e-8) / float(dt))), 0)


class HipToppTrajectoryGenerator(TrajectoryGenerator):
    # every position of a trajectory lies on the natural cubic spline through the waypoints at uniform knots: the curve
    # ``certified_splines`` decides (``generate_certified_trajectories`` asks for this declaration)
    follows_natural_spline = True

    def __init__(self, dt: float, max_velocity, max_acceleration, min_velocity=None, min_acceleration=None,
                 grid_per_segment: int = 8, engine: "_engine.Engine | None" = None, device: int = 0,
                 allow_repeated_waypoints: bool = False) -> None:
        """``min_velocity`` / ``min_acceleration`` default to the negated maxima.  ``grid_per_segment``: grid intervals
        per waypoint segment.  ``engine``: the Engine whose device and stream do the work (its model plays no part);
        without one a small engine is made on ``device`` at the first call.  ``allow_repeated_waypoints``: two equal
        consecutive waypoints raise ValueError unless this is set.  The spline through them is well defined (it dwells
        near the repeated waypoint and overshoots it), and the midpoint insertion of
        ``generate_certified_trajectories`` makes such paths out of a path that has one; a path that does not move
        at all still ends TOPP_STALLED and gives None."""
        if not dt > 0:
            raise ValueError("`dt` must be > 0.")
        if grid_per_segment < 2:
            raise ValueError("`grid_per_segment` must be >= 2.")
        self.dt = float(dt)
        self.vmax = np.array(max_velocity, dtype=np.float64).reshape(-1)
        self.amax = np.array(max_acceleration, dtype=np.float64).reshape(-1)
        self.vmin = -self.vmax if min_velocity is None else np.array(min_velocity, dtype=np.float64).reshape(-1)
        self.amin = -self.amax if min_acceleration is None else np.array(min_acceleration, dtype=np.float64).reshape(-1)
        nq = len(self.vmax)
        if not (len(self.amax) == len(self.vmin) == len(self.amin) == nq):
            raise ValueError("the limits must have one entry per column of the waypoints.")
        if not (np.all(self.vmin < 0) and np.all(self.vmax > 0) and np.all(self.amin < 0) and np.all(self.amax > 0)):
            raise ValueError("limits must satisfy min < 0 < max in every column.")
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
        lim = (self.vmin, self.vmax, self.amin, self.amax)
        M, x, u, t, status = self.engine.topp_profile(W, wp_off, *lim, grid=self.grid)
        g_off = self.engine.topp_offsets(wp_off, self.grid)[1]
        T = t[g_off[1:] - 1] if len(wp_off) > 1 else np.zeros(0)
        return W, wp_off, (M, x, u, t), status, T

    def durations(self, paths) -> np.ndarray:
        """The duration of every path's fastest motion (NaN where none exists): one launch for the whole batch."""
        _, _, _, status, T = self._profile(paths)
        return np.where(status == _engine.TOPP_OK, T, np.nan)

    def generate_trajectories(self, paths) -> list[Trajectory | None]:
        """One trajectory per path (None where the parameterisation stalls or a waypoint is not finite): the whole
        batch is parameterised in one launch sequence and sampled in a second."""
        paths = list(paths)
        if not paths:
            return []
        W, wp_off, prof, status, T = self._profile(paths)
        ok = status == _engine.TOPP_OK
        counts = np.array([sample_count(T[b], self.dt) if ok[b] else 0 for b in range(len(paths))], dtype=np.int64)
        samp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pos, vel, acc = self.engine.topp_sample(W, wp_off, *prof, self.dt, samp_off, self.vmin, self.vmax, self.amin,
                                                self.amax, grid=self.grid)
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
