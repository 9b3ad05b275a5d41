"""Batched planning against a loop over the single-query planner (profiles/README.md).

The headline Franka scene, --problems seeded pairs of valid configurations uniform in the arm's joint ranges (fingers at
home), step_dist 0.01, epsilon 1.0, 16 candidates, 32 rounds.  Reported: the wall time of Engine.plan_paths (host form:
copies in and out included; warmed up, the median of --repeats calls and their spread), the share solved, the rounds
used, the edges validated, and its phases from device events (option "kernel_timer": propose with scan and gather /
validate / commit); beside it DeviceBiRRT.plan_to_config (the planner's defaults, interval_step = step_dist) looped
over --serial of the same problems on the same engine, and that time multiplied up to all of them -- arithmetic, not a
measurement.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from mjpl_amd import CollisionConstraint, DeviceBiRRT, engine, scenes


def random_ends(lo, hi, valid_configs, B, seed):
    """2 B seeded valid configurations uniform in [lo, hi] -> (QI, QG) [B, d]."""
    rng = np.random.default_rng(seed)
    Q = np.zeros((2 * B, len(lo)))
    need = np.ones(2 * B, bool)
    while need.any():
        idx = np.flatnonzero(need)
        cand = rng.uniform(lo, hi, size=(len(idx), len(lo)))
        ok = np.asarray(valid_configs(cand), dtype=bool)
        Q[idx[ok]] = cand[ok]
        need[idx[ok]] = False
    return Q[:B].copy(), Q[B:].copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--serial", type=int, default=64, help="problems given to the DeviceBiRRT loop")
    ap.add_argument("--serial-seconds", type=float, default=5.0, help="max_planning_time of the DeviceBiRRT")
    ap.add_argument("--step-dist", type=float, default=0.01)
    ap.add_argument("--epsilon", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    c = CollisionConstraint(model)
    # (the single-query planner first: it puts the engine on the arm's columns, where both measurements run)
    dev = DeviceBiRRT(model, scenes.FRANKA_ARM_JOINTS, c, home, interval_step=a.step_dist, seed=a.seed, max_planning_time=a.serial_seconds)
    e = c.engine
    lo, hi = model.jnt_range[arm, 0].copy(), model.jnt_range[arm, 1].copy()
    QI, QG = random_ends(lo, hi, lambda Q: e.check_configs(Q), a.problems, a.seed)
    kw = dict(rounds=a.rounds, candidates=a.candidates, nodes=a.nodes, seed=a.seed)

    e.plan_paths(QI, QG, lo, hi, a.step_dist, a.epsilon, **kw)  # warm-up: code objects, scratch, rocPRIM's choice
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        P, n_out, status, rounds_used, edges, tree_nodes = e.plan_paths(QI, QG, lo, hi, a.step_dist, a.epsilon, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
    e.set_option("kernel_timer", 1)  # (a run of its own: the events are not in the wall times above)
    e.plan_paths(QI, QG, lo, hi, a.step_dist, a.epsilon, **kw)
    phases = {k: e.get_option(f"plan_last_{k}_ms") for k in ("propose", "validate", "commit")}
    rounds_run, edges_run, chunks = (int(e.get_option(f"plan_last_{k}")) for k in ("rounds", "edges", "chunks"))
    e.set_option("kernel_timer", 0)
    solved = status == engine.PLAN_SOLVED
    phase_ms = sum(phases.values())
    print(f"batched: median {np.median(wall):.2f} ms, {int(solved.sum())} of {a.problems} solved; now the loop", file=sys.stderr, flush=True)

    # the single-query planner, one problem after the other
    ns = min(a.serial, a.problems)
    serial_ms, serial_solved = [], 0
    for b in range(ns):
        qi, qg = home.copy(), home.copy()
        qi[arm], qg[arm] = QI[b], QG[b]
        t0 = time.perf_counter()
        path = dev.plan_to_config(qi, qg)
        serial_ms.append((time.perf_counter() - t0) * 1e3)
        serial_solved += bool(path)
    serial_total = float(np.sum(serial_ms)) / max(ns, 1) * a.problems
    print(json.dumps({
        "problems": a.problems, "step_dist": a.step_dist, "epsilon": a.epsilon, "rounds": a.rounds, "candidates": a.candidates, "nodes": a.nodes,
        "batched_wall_ms_median": float(np.median(wall)), "batched_wall_ms_min": float(np.min(wall)), "batched_wall_ms_max": float(np.max(wall)),
        "status_counts": np.bincount(status, minlength=5).tolist(), "solved_share": float(solved.mean()),
        "solved_direct_share": float((solved & (rounds_used == 0)).mean()),
        "rounds_used_mean_solved": float(rounds_used[solved].mean()) if solved.any() else None,
        "rounds_used_max_solved": int(rounds_used[solved].max()) if solved.any() else None,
        "mean_path_rows": float(n_out[solved].mean()) if solved.any() else None, "largest_tree": int(tree_nodes.max()),
        "chunks": chunks, "rounds_run": rounds_run, "edges_validated": edges_run, "edges_sum": int(edges.sum()),
        "device_ms": phases, "propose_commit_share": (phases["propose"] + phases["commit"]) / phase_ms if phase_ms > 0 else None,
        "serial_problems": ns, "serial_solved": serial_solved, "serial_solved_batched_same": int(solved[:ns].sum()),
        "serial_ms_per_problem_mean": float(np.mean(serial_ms)) if ns else None, "serial_ms_per_problem_median": float(np.median(serial_ms)) if ns else None,
        "serial_ms_times_problems": serial_total, "serial_over_batched": serial_total / float(np.median(wall)) if ns else None,
    }))
    e.close()


if __name__ == "__main__":
    main()
