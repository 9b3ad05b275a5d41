"""Per-pair contacts (mjpl_contacts_dev) against the collision check (mjpl_check_configs_dev) on the same batches:
Franka-P + 16 obstacles, uniform configurations over the joint ranges (full qpos, AoS), 1 024 / 16 384 / 65 536 of them.

Both are timed the same way: `iters` calls enqueued back to back on the engine's stream, wall clock from the first
enqueue to the synchronisation after the last, divided by `iters` (launch costs included).  The check also reports
mjpl_time_configs_dev's own event timing.  One JSON line per batch size."""
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
    for N in sizes:
        Q = rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(N, m.nq))
        Q[:, 7:] = 0.04
        dq = e.alloc(Q.nbytes).upload(Q)
        dv, db = e.alloc(N), e.alloc(N * W * 8)
        check = per_call_ms(lambda: e.check_configs_dev(dq.ptr, N, engine.AOS, dv.ptr), e.sync, iters)
        contacts = per_call_ms(lambda: e.contacts_dev(dq.ptr, N, engine.AOS, db.ptr), e.sync, iters)
        check_ev = float(np.mean(e.time_configs_dev(dq.ptr, N, engine.AOS, dv.ptr, iters)))
        print(json.dumps({"scene": "franka_p+16obs", "configs": N, "pairs": P, "words": W, "iters": iters,
                          "check_configs_dev_ms": round(check, 4), "check_configs_dev_event_ms": round(check_ev, 4),
                          "contacts_dev_ms": round(contacts, 4), "ratio": round(contacts / check, 2)}), flush=True)
        for b in (dq, dv, db):
            b.free()
    e.close()


if __name__ == "__main__":
    main()
