"""Near pairs (mjpl_near_pairs_dev: every non-allowed pair below distmax with its distance, witnesses and gradient)
against all pair distances (mjpl_distances_dev) and the clearance with the winner's gradient (mjpl_clearance_grad_dev)
on the same batches in the same run: Franka-P + 16 obstacles, uniform configurations over the joint ranges (full qpos,
AoS, nplan = 9), 1 024 / 16 384 / 65 536 of them, (distmax, K) = (0.05, 16) and (0.1, 32), with and without witnesses
(fromto and normal NULL).

Every entry point is timed the same way as tools/time_clearance_grad.py: `iters` calls enqueued back to back on the
engine's stream after one warm-up call, wall clock from the first enqueue to the synchronisation after the last,
divided by `iters` (launch costs included); the figure kept is the median of `runs` such measurements.  One JSON line
per batch size and setting; `mean_count` / `max_count` are the near pairs per configuration the call found."""
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


def main(sizes=(1024, 16384, 65536), settings=((0.05, 16), (0.1, 32)), iters=50, runs=3):
    m = scenes.franka_p(obstacles=True)
    e = engine.Engine(m)
    P = len(e.contact_pairs()[0])
    rng = np.random.default_rng(0)
    for N in sizes:
        Q = rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(N, m.nq))
        Q[:, 7:] = 0.04
        dq = e.alloc(Q.nbytes).upload(Q)
        dd = e.alloc(N * P * 8)
        dc, dp, ds = e.alloc(N * 8), e.alloc(N * 4), e.alloc(N * 4)
        dg, df, dn = e.alloc(N * m.nq * 8), e.alloc(N * 48), e.alloc(N * 24)
        for distmax, K in settings:
            nc, npair, nd, nst = e.alloc(N * 4), e.alloc(N * K * 4), e.alloc(N * K * 8), e.alloc(N * K * 4)
            ng, nf, nn = e.alloc(N * K * m.nq * 8), e.alloc(N * K * 48), e.alloc(N * K * 24)

            def near(witnesses):
                e.near_pairs_dev(dq.ptr, N, engine.AOS, distmax, K, nc.ptr, npair.ptr, nd.ptr, ng.ptr, nst.ptr,
                                 nf.ptr if witnesses else None, nn.ptr if witnesses else None)

            t = {
                "distances_dev_ms": per_call_ms(lambda: e.distances_dev(dq.ptr, N, engine.AOS, dd.ptr, distmax),
                                                e.sync, iters, runs),
                "clearance_grad_dev_ms": per_call_ms(
                    lambda: e.clearance_grad_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, dg.ptr, ds.ptr, df.ptr, dn.ptr,
                                                 distmax), e.sync, iters, runs),
                "near_pairs_dev_ms": per_call_ms(lambda: near(True), e.sync, iters, runs),
                "near_pairs_dev_nowitness_ms": per_call_ms(lambda: near(False), e.sync, iters, runs),
            }
            count = nc.download(np.int32, N)
            row = {"scene": "franka_p+16obs", "configs": N, "pairs": P, "nplan": m.nq, "distmax": distmax, "K": K,
                   "iters": iters, "runs": runs, "mean_count": round(float(count.mean()), 2), "max_count": int(count.max())}
            row.update({k: round(v, 4) for k, v in t.items()})
            print(json.dumps(row), flush=True)
            for b in (nc, npair, nd, nst, ng, nf, nn):
                b.free()
        for b in (dq, dd, dc, dp, ds, dg, df, dn):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
