"""Certified edge checks (mjpl_sweep_edges_dev: free bubbles and bisection over the whole segment) beside the sampled
check (mjpl_check_edges_dev at step 0.01) on the same edges, and beside ONE clearance call (mjpl_clearance_dev) on as
many rows as the sweep evaluated nodes, in the same run: Franka-P + 16 obstacles, the seven arm joints planned from the
home keyframe (AoS), 1 024 / 16 384 / 65 536 edges of length 0.05 and 4 096 edges of length up to 2 rad, d_min 0,
max_depth 8, cap 0.25.

Every entry point is timed the same way as tools/time_near_pairs.py: `iters` calls back to back on the engine's stream
after one warm-up call, wall clock from the first call to the synchronisation after the last, divided by `iters`
(launch costs included; the sweep synchronises once per round by itself); the figure kept is the median of `runs` such
measurements.  One JSON line per batch; `nodes_per_edge` and the FREE / HIT / UNDECIDED shares are the sweep's own."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mjpl_amd import engine, scenes


def per_call_ms(fn, sync, iters, runs):
    fn()
    sync()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(out)


def main(batches=((1024, 0.05), (16384, 0.05), (65536, 0.05), (4096, 2.0)), iters=20, runs=3, max_depth=8, cap=0.25,
         step=0.01):
    m = scenes.franka_p(obstacles=True)
    qidx = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    e = engine.Engine(m)
    e.set_planning(qidx, m.keyframe("home").qpos.copy())
    lo, hi = m.jnt_range[qidx, 0], m.jnt_range[qidx, 1]
    rng = np.random.default_rng(0)
    for E, length in batches:
        qa = rng.uniform(lo, hi, size=(E, len(qidx)))
        d = rng.normal(size=qa.shape)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ln = np.full(E, length) if length <= 0.05 else rng.uniform(0.05, length, size=E)
        qb = np.clip(qa + ln[:, None] * d, lo, hi)
        da, db = e.alloc(qa.nbytes).upload(qa), e.alloc(qb.nbytes).upload(qb)
        st, pr, nd, dp = (e.alloc(E * 4) for _ in range(4))
        th, lb = e.alloc(E * 8), e.alloc(E * 8)
        valid = e.alloc(E)

        def sweep():
            e.sweep_edges_dev(da.ptr, db.ptr, E, engine.AOS, 0.0, st.ptr, th.ptr, lb.ptr, pr.ptr, nd.ptr, dp.ptr, cap=cap,
                              max_depth=max_depth)

        t_sweep = per_call_ms(sweep, e.sync, iters, runs)
        status, nodes = st.download(np.int32, E), nd.download(np.int32, E)
        t_check = per_call_ms(lambda: e.check_edges_dev(da.ptr, db.ptr, E, step, engine.AOS, valid.ptr), e.sync, iters, runs)
        sampled_valid = valid.download(np.uint8, E)
        # one clearance call on as many rows as the sweep evaluated nodes (rows: the edges' end points, repeated)
        R = int(nodes.sum())
        rows = np.resize(np.concatenate([qa, qb]), (R, len(qidx)))
        dr, dc, dcp = e.alloc(rows.nbytes).upload(rows), e.alloc(R * 8), e.alloc(R * 4)
        t_clear = per_call_ms(lambda: e.clearance_dev(dr.ptr, R, engine.AOS, dc.ptr, dcp.ptr, cap), e.sync, iters, runs)
        row = {"scene": "franka_p+16obs", "edges": E, "length": length, "nplan": len(qidx), "max_depth": max_depth, "cap": cap,
               "iters": iters, "runs": runs, "sweep_edges_dev_ms": round(t_sweep, 4),
               "check_edges_dev_ms": round(t_check, 4), "check_step": step, "clearance_dev_same_rows_ms": round(t_clear, 4),
               "nodes": R, "nodes_per_edge": round(R / E, 2), "max_depth_reached": int(dp.download(np.int32, E).max()),
               "free": round(float((status == engine.SWEEP_FREE).mean()), 4),
               "hit": round(float((status == engine.SWEEP_HIT).mean()), 4),
               "undecided": round(float((status == engine.SWEEP_UNDECIDED).mean()), 4),
               "sampled_valid": round(float(sampled_valid.mean()), 4),
               "free_but_sampled_invalid": int(((status == engine.SWEEP_FREE) & (sampled_valid == 0)).sum()),
               "hit_but_sampled_valid": int(((status == engine.SWEEP_HIT) & (sampled_valid == 1)).sum())}
        print(json.dumps(row), flush=True)
        for b in (da, db, st, pr, nd, dp, th, lb, valid, dr, dc, dcp):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
