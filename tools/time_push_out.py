"""Push-out (mjpl_push_out_dev: configurations moved to a minimum clearance) beside ONE near-pair call
(mjpl_near_pairs_dev without witnesses) at the push's own (D*, K) on the same batches in the same run: Franka-P + 16
obstacles, uniform configurations over the joint ranges (full qpos, AoS, nplan = 9), 1 024 / 16 384 / 65 536 of them,
d_min = 0.02 and the default parameters (K = 16, 16 iterations at most).

A push costs one near-pair launch over the rows still active plus one step kernel per iteration, one 4-byte read of
the active count between iterations (a stream synchronisation each), and one clearance launch at the end; the
near-pair call over all rows is the unit to read it against.  Timed as tools/time_near_pairs.py times: `iters` calls
back to back after one warm-up call, wall clock from the first enqueue to the synchronisation after the last, divided
by `iters`; the figure kept is the median of `runs` such measurements.  One JSON line per batch size: `mean_iters` is
the mean number of steps per row, `iterations` the most steps any row took (= near-pair launches of the call, less
one if no row stopped early), `needing` the rows that were moved, `ok` / `stuck` / `degenerate` the status counts."""
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


def main(sizes=(1024, 16384, 65536), d_min=0.02, K=16, iters=20, runs=3):
    m = scenes.franka_p(obstacles=True)
    e = engine.Engine(m)
    pairs, allowed = e.contact_pairs()
    margin = np.asarray(m.geom_margin, float)
    dstar = d_min + float(np.maximum(margin[pairs[~allowed, 0]], margin[pairs[~allowed, 1]]).max())
    rng = np.random.default_rng(0)
    for N in sizes:
        Q = rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(N, m.nq))
        Q[:, 7:] = 0.04
        dq, dout = e.alloc(Q.nbytes).upload(Q), e.alloc(Q.nbytes)
        dc, dp, dit, dst = e.alloc(N * 8), e.alloc(N * 4), e.alloc(N * 4), e.alloc(N * 4)
        nc, npair, nd, nst = e.alloc(N * 4), e.alloc(N * K * 4), e.alloc(N * K * 8), e.alloc(N * K * 4)
        ng = e.alloc(N * K * m.nq * 8)
        t = {
            "push_out_dev_ms": per_call_ms(
                lambda: e.push_out_dev(dq.ptr, N, engine.AOS, d_min, dout.ptr, dc.ptr, dp.ptr, dit.ptr, dst.ptr,
                                       max_pairs=K), e.sync, iters, runs),
            "near_pairs_dev_nowitness_ms": per_call_ms(
                lambda: e.near_pairs_dev(dq.ptr, N, engine.AOS, dstar, K, nc.ptr, npair.ptr, nd.ptr, ng.ptr, nst.ptr),
                e.sync, iters, runs),
        }
        steps, status = dit.download(np.int32, N), dst.download(np.int32, N)
        row = {"scene": "franka_p+16obs", "configs": N, "nplan": m.nq, "d_min": d_min, "distmax": round(dstar, 6), "K": K,
               "iters": iters, "runs": runs, "mean_iters": round(float(steps.mean()), 3), "iterations": int(steps.max()),
               "needing": int((steps > 0).sum()), "ok": int((status == engine.PUSH_OK).sum()),
               "stuck": int((status == engine.PUSH_STUCK).sum()),
               "degenerate": int((status == engine.PUSH_DEGENERATE).sum())}
        row.update({k: round(v, 4) for k, v in t.items()})
        row["push_over_near"] = round(t["push_out_dev_ms"] / t["near_pairs_dev_nowitness_ms"], 2)
        print(json.dumps(row), flush=True)
        for b in (dq, dout, dc, dp, dit, dst, nc, npair, nd, nst, ng):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
