"""Batched path shortcutting against the serial loop (profiles/README.md).

The headline Franka scene, --paths seeded random walks of valid configurations of --waypoints waypoints, step_dist 0.01,
the defaults of smooth_paths (16 rounds of 64 candidates).  Reported: the wall time of Engine.shortcut_paths (host
form: copies in and out included; warmed up, the median of --repeats calls and their spread), its phases from device
events (option "kernel_timer": propose with scan and gather / validate / commit), edges validated, the mean length
ratio; beside it smooth_path(..., sparse=True, num_tries=rounds * candidates) on --serial of the same paths with the
same engine, extrapolated to all of them, and the length ratios of both methods on those paths.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from mjpl_amd import CollisionConstraint, scenes, smooth_path
from mjpl_amd.planning.utils import path_length


def random_walks(lo, hi, valid_configs, B, n, seed, step=0.3, tries=16):
    """B seeded random walks of n valid configurations inside [lo, hi], grown in lockstep (one batch per waypoint)."""
    rng = np.random.default_rng(seed)
    d = len(lo)
    cur = np.zeros((B, d))
    need = np.ones(B, bool)
    while need.any():
        idx = np.flatnonzero(need)
        Q = rng.uniform(lo, hi, size=(len(idx), d))
        ok = valid_configs(Q)
        cur[idx[ok]] = Q[ok]
        need[idx[ok]] = False
    out = np.zeros((B, n, d))
    out[:, 0] = cur
    for k in range(1, n):
        pending = np.arange(B)
        while len(pending):
            dirs = rng.normal(size=(len(pending), tries, d))
            dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
            cand = np.clip(cur[pending][:, None, :] + dirs * rng.uniform(0.5, 1.0, size=(len(pending), tries, 1)) * step, lo, hi)
            ok = valid_configs(cand.reshape(-1, d)).reshape(len(pending), tries)
            first, has = ok.argmax(axis=1), ok.any(axis=1)
            cur[pending[has]] = cand[np.flatnonzero(has), first[has]]
            out[pending[has], k] = cur[pending[has]]
            pending = pending[~has]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=64)
    ap.add_argument("--serial", type=int, default=64, help="paths given to the serial smooth_path")
    ap.add_argument("--step-dist", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    # full configurations, the fingers at their home values: what smooth_path and smooth_paths both take, so the one
    # engine stays on the full column set through both measurements
    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    c = CollisionConstraint(model)
    e = c.engine
    is_arm = np.isin(np.arange(model.nq), arm)
    lo, hi = np.where(is_arm, model.jnt_range[:, 0], home), np.where(is_arm, model.jnt_range[:, 1], home)
    walks = random_walks(lo, hi, c.valid_configs, a.paths, a.waypoints, a.seed)
    W = walks.reshape(-1, model.nq)
    off = np.arange(a.paths + 1, dtype=np.int64) * a.waypoints
    kw = dict(rounds=a.rounds, candidates=a.candidates, seed=a.seed)

    e.shortcut_paths(W, off, a.step_dist, **kw)  # warm-up: code objects, scratch, rocPRIM's choice
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        keep, n_out, length, status, proposed, accepted = e.shortcut_paths(W, off, a.step_dist, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
    e.set_option("kernel_timer", 1)  # (a run of its own: the events are not in the wall times above)
    e.shortcut_paths(W, off, a.step_dist, **kw)
    phases = {k: e.get_option(f"shortcut_last_{k}_ms") for k in ("propose", "validate", "commit")}
    rounds_run, edges = int(e.get_option("shortcut_last_rounds")), int(e.get_option("shortcut_last_edges"))
    e.set_option("kernel_timer", 0)
    before = np.array([path_length(list(w)) for w in walks])
    ratio = length / before

    # the serial loop, the way the example scripts call it: same engine, same step
    ns = min(a.serial, a.paths)
    serial_ms, serial_ratio = [], []
    for b in range(ns):
        path = list(walks[b])
        t0 = time.perf_counter()
        short = smooth_path(path, [c], collision_interval_check=(a.step_dist, c), num_tries=a.rounds * a.candidates,
                            seed=a.seed + b, sparse=True)
        serial_ms.append((time.perf_counter() - t0) * 1e3)
        serial_ratio.append(path_length(short) / before[b])
    serial_total = float(np.sum(serial_ms)) / max(ns, 1) * a.paths
    per_round = {k: v / max(rounds_run, 1) for k, v in phases.items()}
    round_ms = sum(per_round.values())
    print(json.dumps({
        "paths": a.paths, "waypoints": a.waypoints, "step_dist": a.step_dist, "rounds": a.rounds, "candidates": a.candidates,
        "batched_wall_ms_median": float(np.median(wall)), "batched_wall_ms_min": float(np.min(wall)), "batched_wall_ms_max": float(np.max(wall)),
        "rounds_run": rounds_run, "edges_validated": edges, "device_ms_per_round": per_round,
        "propose_commit_share_of_round": (per_round["propose"] + per_round["commit"]) / round_ms if round_ms > 0 else None,
        "status_counts": np.bincount(status, minlength=3).tolist(), "mean_length_ratio": float(ratio.mean()),
        "mean_waypoints_out": float(n_out.mean()),
        "serial_paths": ns, "serial_ms_per_path": float(np.mean(serial_ms)) if ns else None, "serial_ms_extrapolated": serial_total,
        "serial_over_batched": serial_total / float(np.median(wall)) if ns else None,
        "length_ratio_serial": float(np.mean(serial_ratio)) if ns else None, "length_ratio_batched_same_paths": float(ratio[:ns].mean()) if ns else None,
    }))
    e.close()


if __name__ == "__main__":
    main()
