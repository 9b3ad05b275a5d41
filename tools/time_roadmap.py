"""Roadmap planning against the lockstep planner on the same pairs.

The headline Franka scene and the --problems seeded pairs of tools/time_plan.py (same seed, step_dist 0.01).  Per roadmap
size N in --nodes (seeded valid configurations uniform in the arm's joint ranges, k = 8): the wall time of
Engine.roadmap_build and its phases from device events (option "kernel_timer": nodes / neighbours / validate / graph), the
candidate edges and the share valid, the components; then the wall time of Engine.roadmap_query per call (host form: the
graph and the ends copied in, the answers copied out; warmed up, the median of --repeats calls), its phases (attach /
validate / search, which holds the walk back), the share solved and the mean sweeps of the problems that searched.  Beside
it Engine.plan_paths on the same pairs in the same session, and the mean path length of both before and after
smooth_paths.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from mjpl_amd import CollisionConstraint, engine, scenes, smooth_paths
from time_plan import random_ends


def components(N, node_valid, row_off, adj):
    label = np.where(node_valid.astype(bool), np.arange(N), -1)
    src = np.repeat(np.arange(N), np.diff(row_off))
    dst = adj[:row_off[-1]]
    while True:
        low = label.copy()
        np.minimum.at(low, src, label[dst])
        ok = low >= 0
        low[ok] = low[low[ok]]
        if np.array_equal(low, label):
            return label
        label = low


def mean_length(paths):
    return float(np.mean([np.linalg.norm(np.diff(np.stack(p), axis=0), axis=1).sum() for p in paths])) if paths else None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--nodes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--connections", type=int, default=8)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--step-dist", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--smooth", type=int, default=512, help="solved problems whose paths are smoothed for the length comparison")
    a = ap.parse_args()

    model = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    home = model.keyframe("home").qpos.copy()
    c = CollisionConstraint(model)
    c.set_planning(arm, home)
    e = c.engine
    lo, hi = model.jnt_range[arm, 0].copy(), model.jnt_range[arm, 1].copy()
    valid = lambda Q: e.check_configs(Q)  # noqa: E731
    QI, QG = random_ends(lo, hi, valid, a.problems, a.seed)
    out = {"problems": a.problems, "step_dist": a.step_dist, "radius": a.radius, "k": a.k, "connections": a.connections, "roadmaps": []}

    def full(rows):
        W = np.tile(home, (len(rows), 1))
        W[:, arm] = rows
        return list(W)

    answers = {}
    for N in a.nodes:
        nodes = np.concatenate(random_ends(lo, hi, valid, (N + 1) // 2, a.seed + 1))[:N]
        e.roadmap_build(nodes, a.radius, a.step_dist, a.k)  # warm-up: code objects, scratch, rocPRIM's choice
        t0 = time.perf_counter()
        node_valid, row_off, adj, w = e.roadmap_build(nodes, a.radius, a.step_dist, a.k)
        build_ms = (time.perf_counter() - t0) * 1e3
        e.set_option("kernel_timer", 1)  # (a run of its own: the events are not in the wall time above)
        e.roadmap_build(nodes, a.radius, a.step_dist, a.k)
        build_phases = dict(zip(("nodes", "neighbours", "validate", "graph"), (e.get_option(f"roadmap_last_phase{i}_ms") for i in range(4))))
        candidates, launches = int(e.get_option("roadmap_last_edges")), int(e.get_option("roadmap_last_chunks"))
        e.set_option("kernel_timer", 0)
        label = components(N, node_valid, row_off, adj)
        sizes = np.bincount(label[label >= 0])
        graph = (nodes, node_valid, row_off, adj, w)
        qkw = dict(connections=a.connections, max_rows=a.max_rows)
        e.roadmap_query(*graph, QI, QG, a.radius, a.step_dist, **qkw)
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            P, n_out, status, cost = e.roadmap_query(*graph, QI, QG, a.radius, a.step_dist, **qkw)
            wall.append((time.perf_counter() - t0) * 1e3)
        e.set_option("kernel_timer", 1)
        e.roadmap_query(*graph, QI, QG, a.radius, a.step_dist, **qkw)
        query_phases = dict(zip(("attach", "validate", "search_and_walk"), (e.get_option(f"roadmap_last_phase{i}_ms") for i in range(3))))
        q_edges, sweeps = int(e.get_option("roadmap_last_edges")), int(e.get_option("roadmap_last_sweeps"))
        e.set_option("kernel_timer", 0)
        solved = status == engine.ROADMAP_SOLVED
        searched = (status == engine.ROADMAP_NO_PATH) | (status == engine.ROADMAP_LONG) | (solved & (n_out > 2))
        answers[N] = (P, n_out, status)
        out["roadmaps"].append({
            "nodes": N, "build_wall_ms": build_ms, "build_device_ms": build_phases, "candidate_edges": candidates, "edge_launches": launches,
            "valid_edges": int(row_off[-1]) // 2, "valid_share": int(row_off[-1]) / 2 / max(candidates, 1), "components": int((sizes > 0).sum()),
            "largest_component": int(sizes.max()) if len(sizes) else 0,
            "query_wall_ms_median": float(np.median(wall)), "query_wall_ms_min": float(np.min(wall)), "query_wall_ms_max": float(np.max(wall)),
            "query_device_ms": query_phases, "query_edges": q_edges, "status_counts": np.bincount(status, minlength=5).tolist(),
            "solved_share": float(solved.mean()), "solved_direct_share": float((solved & (n_out == 2)).mean()),
            "searched": int(searched.sum()), "mean_sweeps": sweeps / max(int(searched.sum()), 1),
            "mean_path_rows": float(n_out[solved].mean()) if solved.any() else None,
        })
        print(f"N {N}: build {build_ms:.1f} ms, query median {np.median(wall):.2f} ms, {int(solved.sum())} of {a.problems} solved", file=sys.stderr, flush=True)

    # the lockstep planner on the same pairs, its defaults of tools/time_plan.py
    pkw = dict(rounds=32, candidates=16, nodes=1024, seed=a.seed)
    e.plan_paths(QI, QG, lo, hi, a.step_dist, 1.0, **pkw)
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        PP, pn, pstatus, *_ = e.plan_paths(QI, QG, lo, hi, a.step_dist, 1.0, **pkw)
        wall.append((time.perf_counter() - t0) * 1e3)
    psolved = pstatus == engine.PLAN_SOLVED
    out["plan_paths"] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)),
                         "solved_share": float(psolved.mean()), "status_counts": np.bincount(pstatus, minlength=5).tolist()}
    for r in out["roadmaps"]:
        r["plan_over_query"] = out["plan_paths"]["wall_ms_median"] / r["query_wall_ms_median"]
        _, _, status = answers[r["nodes"]]
        r["solved_of_plan_rounds"] = int(((status == engine.ROADMAP_SOLVED) & (pstatus == engine.PLAN_ROUNDS)).sum())
        r["plan_solved_roadmap_not"] = int(((status != engine.ROADMAP_SOLVED) & psolved).sum())
        # the calls after which the roadmap has paid for its build
        saved = out["plan_paths"]["wall_ms_median"] - r["query_wall_ms_median"]
        r["break_even_calls"] = r["build_wall_ms"] / saved if saved > 0 else None

    # path lengths before and after smooth_paths, on the problems both solved (the largest roadmap)
    P, n_out, status = answers[a.nodes[-1]]
    both = np.flatnonzero((status == engine.ROADMAP_SOLVED) & psolved)[:a.smooth]
    rm_paths = [full(P[b, :n_out[b]]) for b in both]
    pl_paths = [full(PP[b, :pn[b]]) for b in both]
    out["lengths"] = {"problems": len(both), "roadmap_nodes": a.nodes[-1], "roadmap": mean_length(rm_paths), "plan_paths": mean_length(pl_paths)}
    if len(both):
        out["lengths"]["roadmap_smoothed"] = mean_length(smooth_paths(rm_paths, c, a.step_dist))
        out["lengths"]["plan_paths_smoothed"] = mean_length(smooth_paths(pl_paths, c, a.step_dist))
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
