#!/usr/bin/env python3
"""UR5e plan -> shortcut -> trajectory: the reference pipeline's last step on the MI355X.

    python examples/plan_smooth_trajectory.py [-s SEED] [--jerk]

Plans to a random valid configuration, shortcuts the path, and turns it into a time-optimal trajectory under
velocity and acceleration limits whose every position obeys the constraints (waypoints are added where the spline
through the path would leave them).  Prints the duration and how much of each limit the trajectory uses.  With --jerk
the trajectory is jerk-limited instead (HipJerkTrajectoryGenerator): slower, and within all three limits
at every instant.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mjpl_amd as mjpl  # noqa: E402
from mjpl_amd import scenes  # noqa: E402


def main() -> bool:
    ap = argparse.ArgumentParser(description="Plan to a target configuration and generate a trajectory.")
    ap.add_argument("-s", "--seed", type=int, default=3)
    ap.add_argument("--jerk", action="store_true", help="limit jerk too (not time-optimal)")
    args = ap.parse_args()
    seed = args.seed

    model = scenes.ur5e()
    arm_joints = mjpl.all_joints(model)
    cc = mjpl.CollisionConstraint(model)
    constraints = [mjpl.JointLimitConstraint(model), cc]
    q_init = model.keyframe("home").qpos.copy()
    q_goal = mjpl.random_config(model, q_init, arm_joints, seed, constraints)

    planner = mjpl.RRT(model, arm_joints, constraints, seed=seed, goal_biasing_probability=0.1)
    waypoints = planner.plan_to_config(q_init, q_goal)
    if not waypoints:
        print("Planning failed")
        return False
    short = mjpl.smooth_path(waypoints, constraints, eps=planner.epsilon, seed=seed, sparse=True)
    print(f"Path: {len(waypoints)} waypoints, {len(short)} after shortcutting (length {mjpl.path_length(short):.3f})")

    dt = 0.002
    max_velocity = np.full(model.nq, np.pi)
    max_acceleration = np.full(model.nq, 2.0 * np.pi)
    max_jerk = np.full(model.nq, 20.0 * np.pi)
    if args.jerk:
        generator = mjpl.HipJerkTrajectoryGenerator(dt, max_velocity, max_acceleration, max_jerk, engine=cc.engine)
    else:
        generator = mjpl.HipToppTrajectoryGenerator(dt, max_velocity, max_acceleration, engine=cc.engine)
    start = time.time()
    traj = mjpl.generate_constrained_trajectory(short, generator, constraints, max_rounds=64)
    if traj is None:
        print("Trajectory generation failed")
        return False
    vel, acc = np.stack(traj.velocities), np.stack(traj.accelerations)
    print(f"Trajectory generation took {(time.time() - start):.4f}s")
    print(f"Duration {len(traj.positions) * dt:.3f}s in {len(traj.positions)} states of {dt}s")
    print(f"Velocity margin  {1.0 - np.abs(vel / max_velocity).max():+.4f} of the limit (largest use per joint: "
          f"{np.round(np.abs(vel / max_velocity).max(axis=0), 3).tolist()})")
    print(f"Acceleration margin {1.0 - np.abs(acc / max_acceleration).max():+.4f} of the limit (largest use per joint: "
          f"{np.round(np.abs(acc / max_acceleration).max(axis=0), 3).tolist()}"
          + (")" if args.jerk else "; between grid points the discretisation may overshoot by a few percent, DESIGN.md 5.12)"))
    if args.jerk:
        jerk = np.diff(np.vstack([np.zeros((1, model.nq)), acc]), axis=0) / dt
        print(f"Jerk margin {1.0 - np.abs(jerk / max_jerk).max():+.4f} of the limit (mean jerk over every step of {dt}s)")
    print(f"Goal error {np.abs(traj.positions[-1] - q_goal).max():.2e}, final speed {np.abs(vel[-1]).max():.2e}")
    return True


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
