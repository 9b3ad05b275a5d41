"""Time the certified trajectories (mjpl_sweep_splines_dev) on device-resident batches, beside mjpl_sweep_edges_dev on
the polyline segments of the same paths.

    python tools/time_spline_sweep.py [--paths 4096] [--waypoints 64] [--max-depth 8] [--cap 0.25] [--iters 10] [--out FILE]

Franka-P + 16 obstacles, the seven arm joints planned from the home keyframe.  Random-walk paths as the tests draw them
(tests/spline_sweep_reference.py: steps 0.05 .. 0.6 in units of the widest column, clipped to the joint ranges).  After a
warm-up of three calls, `iters` calls each between two device events (mjpl_time_sweep_dev); one JSON line with the median
per-call time, the nodes per piece and the rounds (deepest depth + 1), and the same figures for mjpl_sweep_edges_dev on
the segments waypoint k -> k + 1: the straight-line sweep is the only comparable there is, and it decides another curve.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shares(status, engine):
    return {k: round(float((status == v).mean()), 4) for k, v in (("free", engine.SWEEP_FREE), ("hit", engine.SWEEP_HIT),
                                                                  ("undecided", engine.SWEEP_UNDECIDED), ("range", engine.SWEEP_RANGE))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--cap", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import spline_sweep_reference as ssr
    from mjpl_amd import engine, scenes

    m = scenes.franka_p(obstacles=True)
    qidx = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    e = engine.Engine(m, device=0)
    e.set_planning(qidx, m.keyframe("home").qpos.copy())
    lo, hi = m.jnt_range[qidx, 0].copy(), m.jnt_range[qidx, 1].copy()
    B, n = a.paths, a.waypoints
    W, off = ssr.pack(ssr.random_walk_paths(lo, hi, B, seed=11, lengths=(n,)))
    P = B * (n - 1)
    first = np.ones(len(W), bool)
    first[off[1:] - 1] = False  # every row but a path's last starts a segment
    QA, QB = W[first], W[np.roll(first, 1)]
    kw = dict(cap=a.cap, max_depth=a.max_depth, lo=lo, hi=hi)

    dW, dM, dA, dB = e.alloc(W.nbytes).upload(W), e.alloc(W.nbytes), e.alloc(QA.nbytes).upload(QA), e.alloc(QB.nbytes).upload(QB)
    st, pr, nd, dp = (e.alloc(P * 4) for _ in range(4))
    th, lb = e.alloc(P * 8), e.alloc(P * 8)
    outs = (st.ptr, th.ptr, lb.ptr, pr.ptr, nd.ptr, dp.ptr)
    result = {"tool": "time_spline_sweep", "scene": "franka_p+16obs", "paths": B, "waypoints": n, "pieces": P, "nplan": len(qidx),
              "max_depth": a.max_depth, "cap": a.cap, "iters": a.iters, "arch": e.info()["arch"]}
    for name, args in (("sweep_splines_dev", (dW.ptr, dM.ptr, off, B)), ("sweep_edges_dev", (dA.ptr, dB.ptr, None, P))):
        e.time_sweep_dev(*args, engine.AOS, 0.0, *outs, 3, **kw)  # warm-up
        ms = e.time_sweep_dev(*args, engine.AOS, 0.0, *outs, a.iters, **kw)
        status, nodes, depth = st.download(np.int32, P), nd.download(np.int32, P), dp.download(np.int32, P)
        result[name] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                        "nodes_per_piece": round(float(nodes.mean()), 2), "rounds": int(depth.max()) + 1, **shares(status, engine)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for b in (dW, dM, dA, dB, st, pr, nd, dp, th, lb):
        b.free()
    e.close()


if __name__ == "__main__":
    main()
