"""Signed distances and clearance (mjpl_distances_dev, mjpl_clearance_dev) against the collision check
(mjpl_check_configs_dev) and per-pair contacts (mjpl_contacts_dev) on the same batches: Franka-P + 16 obstacles,
uniform configurations over the joint ranges (full qpos, AoS), 1 024 / 16 384 / 65 536 of them.

Every entry point is timed the same way: `iters` calls enqueued back to back on the engine's stream after one
warm-up call, wall clock from the first enqueue to the synchronisation after the last, divided by `iters` (launch
costs included).  One JSON line per batch size; `ratio_*` is a time over the check's."""
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
    P, W = len(e.contact_pairs()[0]), e.contact_words()
    rng = np.random.default_rng(0)
    inf = float("inf")
    for N in sizes:
        Q = rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(N, m.nq))
        Q[:, 7:] = 0.04
        dq = e.alloc(Q.nbytes).upload(Q)
        dv, db, dd = e.alloc(N), e.alloc(N * W * 8), e.alloc(N * P * 8)
        dc, dp = e.alloc(N * 8), e.alloc(N * 4)
        t = {
            "check_configs_dev_ms": per_call_ms(lambda: e.check_configs_dev(dq.ptr, N, engine.AOS, dv.ptr), e.sync, iters),
            "contacts_dev_ms": per_call_ms(lambda: e.contacts_dev(dq.ptr, N, engine.AOS, db.ptr), e.sync, iters),
            "distances_dev_ms": per_call_ms(lambda: e.distances_dev(dq.ptr, N, engine.AOS, dd.ptr, inf), e.sync, iters),
            "clearance_dev_inf_ms": per_call_ms(lambda: e.clearance_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, inf),
                                                e.sync, iters),
            "clearance_dev_0.05_ms": per_call_ms(lambda: e.clearance_dev(dq.ptr, N, engine.AOS, dc.ptr, dp.ptr, 0.05),
                                                 e.sync, iters),
        }
        row = {"scene": "franka_p+16obs", "configs": N, "pairs": P, "iters": iters}
        row.update({k: round(v, 4) for k, v in t.items()})
        check = t["check_configs_dev_ms"]
        row.update({"ratio_" + k[:-3]: round(v / check, 2) for k, v in t.items() if k != "check_configs_dev_ms"})
        print(json.dumps(row), flush=True)
        for b in (dq, dv, db, dd, dc, dp):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
