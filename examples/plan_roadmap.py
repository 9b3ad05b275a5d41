#!/usr/bin/env python3
"""Build once, answer many queries on the MI355X: Roadmap -> smooth_paths -> generate_trajectories.

    python examples/plan_roadmap.py [-N NODES] [-n PROBLEMS] [-c CALLS] [-s SEED]

Samples NODES valid arm configurations of the Franka among its 16 obstacles (fingers at home) and joins each to its 8
nearest within a radius wherever the straight edge is collision-free -- the scene's edges are validated once.  Then
CALLS batches of PROBLEMS start/goal pairs are answered on that roadmap, each with one edge launch (the direct edges
and the ends' attachments) and a shortest-path search; the last batch's paths are shortcut in lockstep and
parameterised under velocity and acceleration limits.  Prints what each stage did and how long it took.
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
    ap = argparse.ArgumentParser(description="Build a roadmap once, then answer batches of start/goal pairs on it.")
    ap.add_argument("-N", "--nodes", type=int, default=4096)
    ap.add_argument("-n", "--problems", type=int, default=256)
    ap.add_argument("-c", "--calls", type=int, default=3)
    ap.add_argument("-r", "--radius", type=float, default=2.0)
    ap.add_argument("-s", "--seed", type=int, default=0)
    args = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    cc = mjpl.CollisionConstraint(model)
    # the sampling box: the arm's joint ranges; the fingers stay where they are (lo == hi)
    is_arm = np.isin(np.arange(model.nq), arm)
    lo, hi = np.where(is_arm, model.jnt_range[:, 0], home), np.where(is_arm, model.jnt_range[:, 1], home)

    step = 0.01
    t0 = time.time()
    roadmap = mjpl.Roadmap(cc, step, radius=args.radius, k=8).build_uniform(args.nodes, lo, hi, seed=args.seed)
    t_build = time.time() - t0
    pairs, lengths = roadmap.edges()
    labels = roadmap.components()
    sizes = np.bincount(labels[labels >= 0])
    print(f"Roadmap.build_uniform: {args.nodes} nodes, {len(pairs)} valid edges (mean length {lengths.mean():.2f}), "
          f"{int((sizes > 0).sum())} components (largest {int(sizes.max())}) in {t_build:.3f}s")

    rng = np.random.default_rng(args.seed + 1)
    solved = []
    for call in range(args.calls):
        ends = []
        while len(ends) < 2 * args.problems:
            Q = rng.uniform(lo, hi, size=(2 * args.problems, model.nq))
            ends += [q for q, ok in zip(Q, cc.valid_configs(Q)) if ok]
        q_inits, q_goals = ends[:args.problems], ends[args.problems:2 * args.problems]
        t0 = time.time()
        paths = roadmap.query(q_inits, q_goals)
        t_query = time.time() - t0
        solved = [p for p in paths if p is not None]
        print(f"Roadmap.query {call}: {len(solved)} of {len(paths)} solved ({sum(1 for p in solved if len(p) == 2)} by the direct edge) "
              f"in {t_query:.3f}s")
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
