"""Trajectories: a path turned into timed positions, velocities and accelerations (the reference's
``mjpl.trajectory`` surface; the parameterisation and the sampling run on the GPU)."""
from .jerk_trajectory import HipJerkTrajectoryGenerator
from .topp_trajectory import HipToppTrajectoryGenerator
from .trajectory_interface import Trajectory, TrajectoryGenerator
from .utils import (generate_certified_trajectories, generate_certified_trajectory, generate_constrained_trajectories,
                    generate_constrained_trajectory)

__all__ = ("Trajectory", "TrajectoryGenerator", "HipToppTrajectoryGenerator", "HipJerkTrajectoryGenerator", "generate_constrained_trajectory",
           "generate_constrained_trajectories", "generate_certified_trajectory", "generate_certified_trajectories")
