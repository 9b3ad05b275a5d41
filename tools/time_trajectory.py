"""Time the trajectory kernels (mjpl_topp_profile_dev + mjpl_topp_sample_dev) on device-resident batches.

    python tools/time_trajectory.py [--paths 4096] [--waypoints 64] [--nq 7] [--grid 8] [--dt 0.002]
                                     [--window 0.6] [--cpu-paths 0] [--jerk] [--jerk-grid 2] [--out FILE]

Random-walk paths (steps 0.05-0.5 per column, as the parity cases of tests/trajectory_reference.py), limits
vmax ~ U[0.5, 2], amax ~ U[0.5, 3].  After a warm-up the calls are repeated, each between device events
(mjpl_time_topp_dev), until the window (seconds of device time) is full; the result is one JSON line with the median
per-call times and paths/s.  --cpu-paths K also times the NumPy statement (tests/trajectory_reference.py) on the first
K paths on this host's CPU -- a reading aid, not a baseline: it is the executable statement, written to be read.
--jerk times mjpl_jerk_profile_dev + mjpl_jerk_sample_dev (mjpl_time_jerk_dev) in the same run, on the same paths and
velocity / acceleration limits with jmax ~ U[5, 20] at --jerk-grid, and adds both pairs' ratios and the mean duration
ratio jerk / TOPP under "jerk" (DESIGN.md 5.14).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_jerk(eng, a, W, off, vmax, amax, jmax, topp, T_topp, ok_topp):
    """The jerk-limited pair on the paths the TOPP pair was just timed on: the same warm-up, events and window."""
    from mjpl_amd import engine
    from mjpl_amd.trajectory.topp_trajectory import sample_count
    B, d, G = a.paths, a.nq, a.jerk_grid
    lim = (vmax, amax, jmax)
    M, L, v, vp, tc, t, status = eng.jerk_profile(W, off, *lim, grid=G)
    g = eng.topp_offsets(off, G)[1]
    T = t[g[1:] - 1]
    ok = status == engine.TOPP_OK
    counts = np.array([sample_count(T[b], a.dt) if ok[b] else 0 for b in range(B)], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ns = int(soff[-1])
    dW = eng.alloc(W.nbytes).upload(W)
    dM, dL, dst = eng.alloc(W.nbytes), eng.alloc(L.nbytes), eng.alloc(4 * B)
    dv, dvp, dtc, dt_ = (eng.alloc(v.nbytes) for _ in range(4))
    dpos, dvel, dacc = (eng.alloc(max(ns * d * 8, 8)) for _ in range(3))
    args = (dW.ptr, off, d, dM.ptr, dL.ptr, dv.ptr, dvp.ptr, dtc.ptr, dt_.ptr, dst.ptr, a.dt, soff, *lim, G, dpos.ptr, dvel.ptr, dacc.ptr)
    mp, ms = eng.time_jerk_dev(*args, 3)  # warm-up
    per = float(mp[-1] + ms[-1]) / 1e3
    prof_ms, samp_ms, spent = [], [], 0.0
    while spent < a.window:
        k = int(min(max((a.window - spent) / per + 1, 1), 64))
        mp, ms = eng.time_jerk_dev(*args, k)
        prof_ms += mp.tolist()
        samp_ms += ms.tolist()
        spent += float(mp.sum() + ms.sum()) / 1e3
    same = np.array_equal(dv.download(np.float64, v.size).view(np.uint64), v.view(np.uint64))
    both = ok & ok_topp
    pm, sm = float(np.median(prof_ms)), float(np.median(samp_ms))
    return {
        "grid": G, "grid_points": int(g[-1]), "samples": ns, "paths_ok": int(ok.sum()), "mean_duration_s": float(T[ok].mean()),
        "calls": len(prof_ms), "window_s": spent, "profile_ms_median": pm, "profile_ms_min": float(np.min(prof_ms)),
        "sample_ms_median": sm, "sample_ms_min": float(np.min(samp_ms)), "paths_per_s_profile": B / (pm / 1e3),
        "sample_gbytes_per_s_written": 3 * ns * d * 8 / (sm / 1e3) / 1e9,
        "topp_sample_gbytes_per_s_written": 3 * topp["samples"] * d * 8 / (topp["sample_ms_median"] / 1e3) / 1e9,
        "profile_ms_over_topp": pm / topp["profile_ms_median"], "sample_ms_over_topp": sm / topp["sample_ms_median"],
        "mean_duration_ratio_over_topp": float(np.mean(T[both] / T_topp[both])), "device_form_equals_host_form": bool(same),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=64)
    ap.add_argument("--nq", type=int, default=7)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--dt", type=float, default=0.002)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--cpu-paths", type=int, default=0)
    ap.add_argument("--jerk", action="store_true")
    ap.add_argument("--jerk-grid", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import trajectory_reference as R
    from mjpl_amd import engine, scenes
    from mjpl_amd.trajectory.topp_trajectory import sample_count

    rng = np.random.default_rng(11)
    B, n, d, G = a.paths, a.waypoints, a.nq, a.grid
    steps = rng.uniform(0.05, 0.5, (B, n - 1, d)) * rng.choice([-1.0, 1.0], (B, n - 1, d))
    W = np.concatenate([np.zeros((B, 1, d)), np.cumsum(steps, axis=1)], axis=1).reshape(B * n, d)
    vmax, amax = rng.uniform(0.5, 2, d), rng.uniform(0.5, 3, d)
    lim = (-vmax, vmax, -amax, amax)
    off = np.arange(B + 1, dtype=np.int64) * n

    eng = engine.Engine(scenes.one_dof_ball(), device=0)
    M, x, u, t, status = eng.topp_profile(W, off, *lim, grid=G)  # (sizes the samples; also the warm-up of the host form)
    g = eng.topp_offsets(off, G)[1]
    T = t[g[1:] - 1]
    ok = status == engine.TOPP_OK
    counts = np.array([sample_count(T[b], a.dt) if ok[b] else 0 for b in range(B)], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ns = int(soff[-1])

    dW = eng.alloc(W.nbytes).upload(W)
    dM, dst = eng.alloc(W.nbytes), eng.alloc(4 * B)
    dx, du, dt_ = (eng.alloc(x.nbytes) for _ in range(3))
    dpos, dvel, dacc = (eng.alloc(max(ns * d * 8, 8)) for _ in range(3))
    args = (dW.ptr, off, d, dM.ptr, dx.ptr, du.ptr, dt_.ptr, dst.ptr, a.dt, soff, *lim, G, dpos.ptr, dvel.ptr, dacc.ptr)
    mp, ms = eng.time_topp_dev(*args, 3)  # warm-up
    per = float(mp[-1] + ms[-1]) / 1e3
    prof_ms, samp_ms, spent = [], [], 0.0
    while spent < a.window:
        k = int(min(max((a.window - spent) / per + 1, 1), 64))
        mp, ms = eng.time_topp_dev(*args, k)
        prof_ms += mp.tolist()
        samp_ms += ms.tolist()
        spent += float(mp.sum() + ms.sum()) / 1e3
    same = np.array_equal(dx.download(np.float64, x.size).view(np.uint64), x.view(np.uint64))
    out = {
        "tool": "time_trajectory", "paths": B, "waypoints": n, "nq": d, "grid": G, "dt": a.dt,
        "grid_points": int(g[-1]), "samples": ns, "paths_ok": int(ok.sum()), "mean_duration_s": float(T[ok].mean()),
        "calls": len(prof_ms), "window_s": spent,
        "profile_ms_median": float(np.median(prof_ms)), "profile_ms_min": float(np.min(prof_ms)),
        "sample_ms_median": float(np.median(samp_ms)), "sample_ms_min": float(np.min(samp_ms)),
        "paths_per_s_profile": B / (float(np.median(prof_ms)) / 1e3),
        "paths_per_s_profile_and_sample": B / (float(np.median(prof_ms) + np.median(samp_ms)) / 1e3),
        "device_form_equals_host_form": bool(same), "arch": eng.info()["arch"],
    }
    if a.jerk:
        out["jerk"] = time_jerk(eng, a, W, off, vmax, amax, rng.uniform(5, 20, d), out, T, ok)
    if a.cpu_paths > 0:
        k = min(a.cpu_paths, B)
        t0 = time.perf_counter()
        for b in range(k):
            p = R.profile(W[b * n:(b + 1) * n], *lim, G)
        t1 = time.perf_counter()
        R.sample(W[(k - 1) * n:k * n], p, a.dt)
        t2 = time.perf_counter()
        out["numpy_statement_cpu"] = {"paths": k, "profile_s_per_path": (t1 - t0) / k, "sample_s_last_path": t2 - t1,
                                      "paths_per_s_profile": k / (t1 - t0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
