"""The trajectory plug-in type (reference src/mjpl/trajectory/trajectory_interface.py:7-41)."""
from __future__ import annotations

import abc
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Trajectory:
    """``n`` timed states ``dt`` apart: state k (0-based) is the state at ``(k + 1) * dt``, the last one the state at
    the end of the motion.  The duration counts as ``dt * n``."""

    dt: float
    q_init: np.ndarray  # the configuration at t = 0
    positions: list[np.ndarray]
    velocities: list[np.ndarray]
    accelerations: list[np.ndarray]


class TrajectoryGenerator(abc.ABC):
    @abc.abstractmethod
    def generate_trajectory(self, waypoints: list[np.ndarray]) -> Trajectory | None:
        """A trajectory through ``waypoints``, or None when none can be generated."""
