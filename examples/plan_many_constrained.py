#!/usr/bin/env python3
"""Many constrained queries at once on the MI355X: plan_paths_constrained -> generate_constrained_trajectories.

    python examples/plan_many_constrained.py [-n PROBLEMS] [-s SEED]

"Carry the cup upright", PROBLEMS times: the Franka among its 16 obstacles, the end effector's roll and pitch held
within 0.1 rad of the home pose (a PoseConstraint, enforced by projection on the GPU).  Goals and starts are seeded
uniform samples projected onto the constraint with q_step = inf, as examples/franka_constrained_move_to_pose.py draws
its goal.  All pairs are planned in lockstep -- every tree edge one projected step, the trees joined by a bridge of
projected steps, every edge of every pair validated by one launch per round -- and the solved paths are parameterised
under the same constraints.  smooth_paths is left out on purpose: it is unconstrained and would leave the manifold.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mjpl_amd as mjpl  # noqa: E402
from mjpl_amd import scenes  # noqa: E402

EE_SITE = "ee_site"


def main() -> bool:
    ap = argparse.ArgumentParser(description="Plan and parameterise many start/goal pairs under an end-effector pose constraint.")
    ap.add_argument("-n", "--problems", type=int, default=64)
    ap.add_argument("-s", "--seed", type=int, default=0)
    args = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    # the fingers half open: at home they sit ON their upper limit, and a trajectory's samples of a constant 0.04 may come
    # out an ulp above it, which JointLimitConstraint refuses (the end effector's pose does not depend on them)
    home[~np.isin(np.arange(model.nq), arm)] = 0.02
    collision = mjpl.CollisionConstraint(model)
    pose = mjpl.PoseConstraint(model, EE_SITE, mjpl.site_pose(model, home, EE_SITE, engine=collision.engine),
                               roll=(-0.1, 0.1), pitch=(-0.1, 0.1), engine=collision.engine)
    constraints = [pose, mjpl.JointLimitConstraint(model), collision]
    # the sampling box: the arm's joint ranges; the fingers stay where they are (lo == hi)
    is_arm = np.isin(np.arange(model.nq), arm)
    lo, hi = np.where(is_arm, model.jnt_range[:, 0], home), np.where(is_arm, model.jnt_range[:, 1], home)

    # ends on the manifold: lift q_step while projecting the samples
    rng = np.random.default_rng(args.seed)
    q_step = pose.q_step
    pose.q_step = np.inf
    ends = []
    while len(ends) < 2 * args.problems:
        X = rng.uniform(lo, hi, size=(4 * args.problems, model.nq))
        Y, ok, _ = pose.apply_batch(X, X)
        Y = Y[ok & (Y >= lo).all(axis=1) & (Y <= hi).all(axis=1)]
        ends += [q for q, good in zip(Y, pose.valid_configs(Y) & collision.valid_configs(Y)) if good]
    pose.q_step = q_step
    q_inits, q_goals = ends[:args.problems], ends[args.problems:2 * args.problems]

    step = 0.01
    t0 = time.time()
    # (extend=4: an extension is a chain of up to 4 projected steps -- the row of DESIGN.md 5.18 that solves the most pairs
    # for its time at the other defaults)
    paths, info = mjpl.plan_paths_constrained(q_inits, q_goals, collision, pose, step, epsilon=q_step, seed=args.seed, lo=lo, hi=hi,
                                              return_info=True, extend=4)
    t_plan = time.time() - t0
    solved = [p for p in paths if p is not None]
    print(f"plan_paths_constrained: {len(solved)} of {len(paths)} solved in {t_plan:.3f}s, "
          f"{sum(i['edges'] for i in info)} edges validated, mean {np.mean([len(p) for p in solved]) if solved else 0:.1f} waypoints; "
          f"other statuses: {sorted({i['status'] for i in info} - {'solved'}) or 'none'}")
    if not solved:
        return False
    on_manifold = all(pose.valid_configs(np.stack(p)).all() for p in solved)
    print(f"every waypoint obeys the pose constraint: {on_manifold}")

    dt = 0.002
    generator = mjpl.HipToppTrajectoryGenerator(dt, np.full(model.nq, np.pi), np.full(model.nq, 2.0 * np.pi), engine=collision.engine)
    t0 = time.time()
    trajs = mjpl.generate_constrained_trajectories(solved, generator, constraints, max_rounds=64)
    t_traj = time.time() - t0
    made = [t for t in trajs if t is not None]
    print(f"generate_constrained_trajectories: {len(made)} of {len(solved)} trajectories in {t_traj:.3f}s"
          + (f", mean duration {np.mean([len(t.positions) * dt for t in made]):.2f}s" if made else ""))
    return on_manifold and len(made) > 0


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
