"""Clearance with its gradient and witness points (mjpl_clearance_grad_dev) against the clearance alone
(mjpl_clearance_dev) on the same batches: Franka-P + 16 obstacles, uniform configurations over the joint ranges
(full qpos, AoS, nplan = 9), 1 024 / 16 384 / 65 536 of them, distmax = inf.

Both entry points are timed the same way as tools/time_distances.py: `iters` calls enqueued back to back on the
engine's stream after one warm-up call, wall clock from the first enqueue to the synchronisation after the last,
divided by `iters` (launch costs included).  One JSON line per batch size; `ratio` is grad over clearance."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mjpl_amd import engine, scenes


def per_call_ms(fn, sync, iters):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / iters


def main(sizes=(1024, 16384, 65536), iters=50):
    m = scenes.franka_p(obstacles=True)
    e = engine.Engine(m)
    P = len(e.contact_pairs()[0])
    rng = np.random.default_rng(0)
    inf = float("inf")
    for N in sizes:
        Q = rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(N, m.nq))
        Q[:, 7:] = 0.04
        dq = e.alloc(Q.nbytes).upload(Q)
        dc, dp, ds = e.alloc(N * 8), e.alloc(N * 4), e.alloc(N * 4)
        dg, df, dn = e.alloc(N * m.nq * 8), e.alloc(N * 48), e.alloc(N * 24)
        t = {
            "clearance_dev_ms": per_call_ms(lambda: e.clearance_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, inf),
                                            e.sync, iters),
            "clearance_grad_dev_ms": per_call_ms(
                lambda: e.clearance_grad_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, dg.ptr, ds.ptr, df.ptr, dn.ptr, inf),
                e.sync, iters),
            "clearance_grad_dev_nowitness_ms": per_call_ms(
                lambda: e.clearance_grad_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, dg.ptr, ds.ptr, None, None, inf),
                e.sync, iters),
        }
        row = {"scene": "franka_p+16obs", "configs": N, "pairs": P, "nplan": m.nq, "iters": iters}
        row.update({k: round(v, 4) for k, v in t.items()})
        row["ratio"] = round(t["clearance_grad_dev_ms"] / t["clearance_dev_ms"], 2)
        print(json.dumps(row), flush=True)
        for b in (dq, dc, dp, ds, dg, df, dn):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
