"""Constrained batched planning against a loop over the single-query constrained planner.

The headline Franka scene over the 7 arm columns (fingers at home), the end effector's roll and pitch within 0.1 rad of
the home pose; --problems seeded pairs ON that manifold (uniform draws in the arm's ranges projected with q_step = inf,
kept where collision-valid and pose-valid), epsilon 0.05, q_step 0.05, step_dist 0.01, the defaults otherwise (--extend X:
an extension is a chain of up to X projected steps; the default of 1 is a single step).
Reported: the wall time of Engine.plan_paths_constrained (host form: copies in and out included; one warm-up call, then
the median of --repeats calls and their spread), the share solved, the status counts, mean rounds and rows, the edges
validated, and its phases from device events (option "kernel_timer": propose with count, scan and gather / project /
validate / commit); beside it DeviceBiRRT(pose=...).plan_to_config looped over --serial of the same pairs on the same
engine, per pair and multiplied up to all of them -- arithmetic, not a measurement.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from mjpl_amd import CollisionConstraint, DeviceBiRRT, PoseConstraint, engine, scenes, site_pose

EE_SITE = "ee_site"


def manifold_ends(e, pose, arm, home, lo, hi, B, seed):
    """2 B seeded configurations on the constraint manifold, collision-valid -> (QI, QG) [B, 7] over the arm's columns."""
    rng = np.random.default_rng(seed)
    q_step = pose.q_step
    pose.q_step = np.inf
    rows = np.zeros((0, len(arm)))
    while len(rows) < 2 * B:
        X = np.tile(home, (4 * B, 1))
        X[:, arm] = rng.uniform(lo, hi, size=(4 * B, len(arm)))
        Y, ok, _ = pose.apply_batch(X, X)
        Y = Y[ok & (Y[:, arm] >= lo).all(axis=1) & (Y[:, arm] <= hi).all(axis=1)]
        keep = pose.valid_configs(Y) & e.check_configs(np.ascontiguousarray(Y[:, arm])).astype(bool)
        rows = np.concatenate([rows, Y[keep][:, arm]])
    pose.q_step = q_step
    return rows[:B].copy(), rows[B:2 * B].copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--serial", type=int, default=16, help="pairs given to the DeviceBiRRT loop")
    ap.add_argument("--serial-seconds", type=float, default=5.0, help="max_planning_time of the DeviceBiRRT")
    ap.add_argument("--step-dist", type=float, default=0.01)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--q-step", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=8)
    ap.add_argument("--max-rows", type=int, default=256)
    ap.add_argument("--extend", type=int, default=1, help="steps of an extension chain (1..32)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    c = CollisionConstraint(model)
    e = c.engine
    pose = PoseConstraint(model, EE_SITE, site_pose(model, home, EE_SITE, engine=e), roll=(-0.1, 0.1), pitch=(-0.1, 0.1),
                          q_step=a.q_step, engine=e)
    # (the single-query planner first: it puts the engine on the arm's columns, where both measurements run)
    dev = DeviceBiRRT(model, scenes.FRANKA_ARM_JOINTS, c, home, epsilon=a.epsilon, interval_step=a.step_dist, seed=a.seed,
                      max_planning_time=a.serial_seconds, pose=pose)
    lo, hi = model.jnt_range[arm, 0].copy(), model.jnt_range[arm, 1].copy()
    QI, QG = manifold_ends(e, pose, arm, home, lo, hi, a.problems, a.seed)
    kw = dict(rounds=a.rounds, candidates=a.candidates, nodes=a.nodes, chain=a.chain, max_rows=a.max_rows, seed=a.seed, extend=a.extend)

    def call():
        return e.plan_paths_constrained(pose, QI, QG, lo, hi, a.step_dist, a.epsilon, **kw)

    call()  # warm-up: code objects, scratch, rocPRIM's choice
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        P, n_out, status, rounds_used, edges, tree_nodes = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    e.set_option("kernel_timer", 1)  # (a run of its own: the events are not in the wall times above)
    call()
    phases = {k: e.get_option(f"plan_last_{k}_ms") for k in ("propose", "project", "validate", "commit")}
    rounds_run, edges_run, chunks = (int(e.get_option(f"plan_last_{k}")) for k in ("rounds", "edges", "chunks"))
    e.set_option("kernel_timer", 0)
    solved = status == engine.PLAN_SOLVED
    print(f"batched: median {np.median(wall):.2f} ms, {int(solved.sum())} of {a.problems} solved; now the loop", file=sys.stderr, flush=True)

    # the single-query constrained planner, one pair after the other
    ns = min(a.serial, a.problems)
    serial_ms, serial_solved = [], 0
    for b in range(ns):
        qi, qg = home.copy(), home.copy()
        qi[arm], qg[arm] = QI[b], QG[b]
        t0 = time.perf_counter()
        path = dev.plan_to_config(qi, qg)
        serial_ms.append((time.perf_counter() - t0) * 1e3)
        serial_solved += bool(path)
    per_pair = float(np.mean(serial_ms)) if ns else None
    print(json.dumps({
        "problems": a.problems, "step_dist": a.step_dist, "epsilon": a.epsilon, "q_step": a.q_step, "rounds": a.rounds,
        "candidates": a.candidates, "nodes": a.nodes, "chain": a.chain, "max_rows": a.max_rows, "extend": a.extend,
        "batched_wall_ms_median": float(np.median(wall)), "batched_wall_ms_min": float(np.min(wall)), "batched_wall_ms_max": float(np.max(wall)),
        "status_counts": np.bincount(status, minlength=6).tolist(), "solved_share": float(solved.mean()),
        "rounds_used_mean_solved": float(rounds_used[solved].mean()) if solved.any() else None,
        "rounds_used_max_solved": int(rounds_used[solved].max()) if solved.any() else None,
        "mean_path_rows": float(n_out[solved].mean()) if solved.any() else None,
        "max_path_rows": int(n_out.max()), "largest_tree": int(tree_nodes.max()),
        "chunks": chunks, "rounds_run": rounds_run, "edges_validated": edges_run, "edges_sum": int(edges.sum()),
        "device_ms": phases,
        "serial_pairs": ns, "serial_solved": serial_solved, "serial_solved_batched_same": int(solved[:ns].sum()),
        "serial_ms_per_pair_mean": per_pair, "serial_ms_per_pair_median": float(np.median(serial_ms)) if ns else None,
        "serial_ms_times_problems": per_pair * a.problems if ns else None,
        "serial_over_batched": per_pair * a.problems / float(np.median(wall)) if ns else None,
    }))
    e.close()


if __name__ == "__main__":
    main()
