"""Trajectories that obey constraints (reference src/mjpl/trajectory/utils.py:8-118): generate, find the first state
that violates a constraint, add a waypoint to the path segment it belongs to, generate again."""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from ..constraint.constraint_interface import Constraint
from ..constraint.utils import apply_constraints, obeys_constraints
from .trajectory_interface import Trajectory, TrajectoryGenerator


def _first_violations(position_lists: list[list[np.ndarray]], constraints: list[Constraint]) -> list[int | None]:
    """Per list of positions the index of the first one that violates a constraint (None: all obey).  When every
    constraint answers ``valid_configs``, all positions of all lists go through one call per constraint."""
    if constraints and all(hasattr(c, "valid_configs") for c in constraints) and any(len(p) for p in position_lists):
        Q = np.concatenate([np.stack(p) for p in position_lists if len(p)])
        valid = np.ones(len(Q), dtype=bool)
        for c in constraints:
            valid &= np.asarray(c.valid_configs(Q), dtype=bool)
        out, at = [], 0
        for p in position_lists:
            v = valid[at:at + len(p)]
            at += len(p)
            out.append(None if v.all() else int(np.argmin(v)))
        return out
    out = []
    for p in position_lists:
        out.append(next((i for i, q in enumerate(p) if not obeys_constraints(q, constraints)), None))
    return out


def _refine(waypoints: list[np.ndarray], traj: Trajectory, i: int, constraints: list[Constraint]) -> bool:
    """Add a waypoint to the segment of ``waypoints`` that state ``i`` of ``traj`` belongs to."""
    timing = _waypoint_timing(waypoints, traj)
    return _add_intermediate_waypoint(waypoints, timing, (i + 1) * traj.dt, constraints)


def generate_constrained_trajectory(waypoints: list[np.ndarray], generator: TrajectoryGenerator,
                                    constraints: list[Constraint], max_rounds: int | None = None) -> Trajectory | None:
    """A trajectory through ``waypoints`` whose every position obeys ``constraints``, or None.

    It assumes that the straight segments between adjacent waypoints obey the constraints (section 3.5 of Richter et
    al., ISRR 2013).  Per round:
      1. generate a trajectory (None ends the search);
      2. find the first position that violates the constraints (none: the trajectory is returned);
      3. give every waypoint a timestamp: the first 0, an interior one ``(argmin of the squared distance over the
         positions + 1) * dt``, the last ``len(positions) * dt``;
      4. in the first segment whose timestamps bracket ``(i + 1) * dt`` insert the midpoint, after
         ``apply_constraints(mid, mid, constraints)``; if that fails, or no segment brackets it, return None.
    ``max_rounds`` bounds the number of trajectories generated (None: no bound, as in the reference); when it is used
    up the result is None.  Unlike the reference this does NOT mutate the caller's list: it works on a copy.
    """
    return generate_constrained_trajectories([waypoints], generator, constraints, max_rounds)[0]


def generate_constrained_trajectories(paths: list[list[np.ndarray]], generator: TrajectoryGenerator,
                                      constraints: list[Constraint],
                                      max_rounds: int | None = None) -> list[Trajectory | None]:
    """:func:`generate_constrained_trajectory` for every path, in lockstep: per round one generation (one
    ``generate_trajectories`` call where the generator has it) and one validation (one ``valid_configs`` call per
    constraint where all have it) over the paths still open.  The result per path is that of the single call."""
    work = [list(p) for p in paths]
    result: list[Trajectory | None] = [None] * len(work)
    open_ids = list(range(len(work)))
    rounds = 0
    while open_ids and (max_rounds is None or rounds < max_rounds):
        rounds += 1
        if hasattr(generator, "generate_trajectories"):
            trajs = generator.generate_trajectories([work[k] for k in open_ids])
        else:
            trajs = [generator.generate_trajectory(work[k]) for k in open_ids]
        alive = [(k, tr) for k, tr in zip(open_ids, trajs) if tr is not None]
        firsts = _first_violations([tr.positions for _, tr in alive], constraints)
        open_ids = []
        for (k, tr), i in zip(alive, firsts):
            if i is None:
                result[k] = tr
            elif _refine(work[k], tr, i, constraints):
                open_ids.append(k)
    return result


def _waypoint_timing(waypoints: list[np.ndarray], trajectory: Trajectory) -> list[float]:
    """A timestamp per waypoint from the trajectory that follows them (step 3 above)."""
    if len(waypoints) < 2:
        raise ValueError("There must be at least two waypoints defined.")
    timestamps = [0.0]
    if len(waypoints) > 2:
        positions = np.stack(trajectory.positions)
        for wp in waypoints[1:-1]:
            d2 = np.sum((positions - wp) ** 2, axis=1)
            timestamps.append((int(np.argmin(d2)) + 1) * trajectory.dt)
    timestamps.append(len(trajectory.positions) * trajectory.dt)
    return timestamps


def _add_intermediate_waypoint(waypoints: list[np.ndarray], timing: list[float], timestamp: float,
                               constraints: list[Constraint] = ()) -> bool:
    """Insert the constrained midpoint of the first segment of ``waypoints`` whose timestamps bracket ``timestamp``
    (so a timestamp equal to an interior waypoint's picks the earlier segment).  False, and nothing added, when no
    segment brackets it or the midpoint cannot be made to obey the constraints."""
    if len(waypoints) != len(timing):
        raise ValueError("`waypoints` and `timing` must be the same length.")
    for i in range(len(waypoints) - 1):
        if timing[i] <= timestamp <= timing[i + 1]:
            return _insert_midpoint(waypoints, i, constraints)
    return False


def _insert_midpoint(waypoints: list[np.ndarray], i: int, constraints: list[Constraint] = ()) -> bool:
    """Insert the constrained midpoint of segment ``i`` of ``waypoints``.  False, and nothing added, when the midpoint
    cannot be made to obey the constraints."""
    mid = (np.asarray(waypoints[i]) + np.asarray(waypoints[i + 1])) / 2
    mid = apply_constraints(mid, mid, list(constraints))
    if mid is None:
        return False
    waypoints.insert(i + 1, mid)
    return True


def generate_certified_trajectory(waypoints: list[np.ndarray], generator: TrajectoryGenerator,
                                  constraints: list[Constraint], certifier, max_rounds: int = 16, **params):
    """A trajectory through ``waypoints`` whose WHOLE curve is certified, with its certificate -> ``(Trajectory,
    CertifiedPath)`` or None.  :func:`generate_certified_trajectories` for one path."""
    return generate_certified_trajectories([waypoints], generator, constraints, certifier, max_rounds, **params)[0]


def generate_certified_trajectories(paths: list[list[np.ndarray]], generator: TrajectoryGenerator,
                                    constraints: list[Constraint], certifier, max_rounds: int = 16, **params) -> list:
    """:func:`generate_constrained_trajectories` with a verdict on the curve between the samples.

    ``generate_constrained_trajectory`` checks the positions ``dt`` apart and assumes the rest; the spline a trajectory
    follows can leave the polyline the planner validated by a lot.  Here, once no sampled position of a path violates
    ``constraints``, its spline goes to ``certifier.certified_splines`` (a ``CollisionConstraint`` or a
    ``ClearanceConstraint``; ``params`` -- cap, max_depth, lo, hi -- are handed on), all such paths of a round in one
    call.  A path whose spline is SWEEP_FREE is done: the result is ``(Trajectory, CertifiedPath)``.  Otherwise the
    midpoint of the first piece that is not FREE is inserted between that piece's two waypoints, after
    ``apply_constraints`` as in the sampled loop, and the path goes another round.  Midpoint insertion need not
    converge, so ``max_rounds`` must be a finite count of generations; when it is used up the result is None, as it is
    when the generator or the insertion fails or a waypoint is not finite.

    The certificate is about the natural cubic spline through the waypoints at uniform knots, so ``generator`` must
    declare that its trajectories follow it (``follows_natural_spline``, as ``HipToppTrajectoryGenerator`` does);
    any other generator raises TypeError.  The caller's lists are not mutated."""
    if not getattr(generator, "follows_natural_spline", False):
        raise TypeError("the certificate is about the natural cubic spline through the waypoints: the generator must declare "
                        "`follows_natural_spline = True`")
    if max_rounds is None or isinstance(max_rounds, bool) or not np.isfinite(max_rounds):
        raise ValueError("`max_rounds` must be finite: midpoint insertion need not converge")
    work = [list(p) for p in paths]
    result: list = [None] * len(work)
    open_ids = list(range(len(work)))
    rounds = 0
    while open_ids and rounds < max_rounds:
        rounds += 1
        if hasattr(generator, "generate_trajectories"):
            trajs = generator.generate_trajectories([work[k] for k in open_ids])
        else:
            trajs = [generator.generate_trajectory(work[k]) for k in open_ids]
        alive = [(k, tr) for k, tr in zip(open_ids, trajs) if tr is not None]
        firsts = _first_violations([tr.positions for _, tr in alive], constraints)
        open_ids, clean = [], []
        for (k, tr), i in zip(alive, firsts):
            if i is None:
                clean.append((k, tr))
            elif _refine(work[k], tr, i, constraints):
                open_ids.append(k)
        certs = certifier.certified_splines([work[k] for k, _ in clean], **params) if clean else []
        for (k, tr), cert in zip(clean, certs):
            if cert.status == _engine.SWEEP_FREE:
                result[k] = (tr, cert)
            elif cert.status != _engine.SWEEP_NONFINITE:
                first = int(np.flatnonzero(np.asarray(cert.piece_status) != _engine.SWEEP_FREE)[0])
                if _insert_midpoint(work[k], first, constraints):
                    open_ids.append(k)
        open_ids.sort()
    return result
