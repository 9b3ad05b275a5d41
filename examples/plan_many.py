#!/usr/bin/env python3
"""Many queries at once on the MI355X: plan_paths -> smooth_paths -> generate_trajectories.

    python examples/plan_many.py [-n PROBLEMS] [-s SEED]

Draws PROBLEMS pairs of valid arm configurations of the Franka among its 16 obstacles (fingers at home), plans all of
them in lockstep (a bidirectional RRT per pair, every edge of every pair validated by one launch per round), shortcuts
the solved paths in lockstep, and parameterises them under velocity and acceleration limits -- three batched calls
where a loop over a single-query planner would make thousands.  Prints what each stage did and how long it took.
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
    ap = argparse.ArgumentParser(description="Plan, shortcut and parameterise many start/goal pairs in three batched calls.")
    ap.add_argument("-n", "--problems", type=int, default=256)
    ap.add_argument("-s", "--seed", type=int, default=0)
    args = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    cc = mjpl.CollisionConstraint(model)
    # the sampling box: the arm's joint ranges; the fingers stay where they are (lo == hi)
    is_arm = np.isin(np.arange(model.nq), arm)
    lo, hi = np.where(is_arm, model.jnt_range[:, 0], home), np.where(is_arm, model.jnt_range[:, 1], home)

    rng = np.random.default_rng(args.seed)
    ends = []
    while len(ends) < 2 * args.problems:
        Q = rng.uniform(lo, hi, size=(2 * args.problems, model.nq))
        ends += [q for q, ok in zip(Q, cc.valid_configs(Q)) if ok]
    q_inits, q_goals = ends[:args.problems], ends[args.problems:2 * args.problems]

    step = 0.01
    t0 = time.time()
    paths, info = mjpl.plan_paths(q_inits, q_goals, cc, step, epsilon=1.0, seed=args.seed, lo=lo, hi=hi, return_info=True)
    t_plan = time.time() - t0
    solved = [p for p in paths if p is not None]
    direct = sum(1 for i in info if i["status"] == "solved" and i["rounds_used"] == 0)
    print(f"plan_paths: {len(solved)} of {len(paths)} solved ({direct} by the direct edge) in {t_plan:.3f}s, "
          f"{sum(i['edges'] for i in info)} edges validated; other statuses: "
          f"{sorted({i['status'] for i in info} - {'solved'}) or 'none'}")
    if not solved:
        return False

    t0 = time.time()
    short = mjpl.smooth_paths(solved, cc, step, seed=args.seed)
    t_smooth = time.time() - t0
    before, after = sum(mjpl.path_length(p) for p in solved), sum(mjpl.path_length(p) for p in short)
    print(f"smooth_paths: {sum(map(len, solved))} -> {sum(map(len, short))} waypoints, length {before:.1f} -> {after:.1f} in {t_smooth:.3f}s")

    dt = 0.002
    generator = mjpl.HipToppTrajectoryGenerator(dt, np.full(model.nq, np.pi), np.full(model.nq, 2.0 * np.pi), engine=cc.engine)
    t0 = time.time()
    trajs = generator.generate_trajectories(short)
    t_traj = time.time() - t0
    made = [t for t in trajs if t is not None]
    print(f"generate_trajectories: {len(made)} of {len(short)} trajectories in {t_traj:.3f}s, "
          f"mean duration {np.mean([len(t.positions) * dt for t in made]):.2f}s")
    return len(made) == len(short)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
