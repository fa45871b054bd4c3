#!/usr/bin/env python3
"""Scoring a track: the CPU evaluators (metrics.add + metrics.adi, a KD-tree per pose pair, workers=-1) against ONE
Engine.pose_errors call (se3tn_pose_errors_host) on the same seeded points and poses.

Prints one JSON line with, for (n = 2,000, P = 2,620) -- a YCB points.xyz -- and (n = 2,000, P = 8,000): seconds of the CPU loop (and of
the same loop with workers=1), seconds of the device call (median of --calls calls after one warm-up; every call runs under its own watchdog, which ends the
process if the call does not return), and the largest difference between the two results.  The process is pinned to at most 16
CPUs before anything is timed.

    python scripts/pose_errors_report.py [--n 2000] [--points 2620,8000] [--calls 5] [--call-timeout 60]
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n, P, seed):
    """A model of P points in a 0.1 m ball and n (pred, gt) pairs with errors from a micrometre to tens of centimetres."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(P, 3))
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * 0.1 * rng.uniform(0.2, 1.0, (P, 1))
    gts = np.tile(np.eye(4), (n, 1, 1))
    gts[:, :3, :3] = Rotation.from_rotvec(rng.normal(0, 1.0, (n, 3))).as_matrix()
    gts[:, :3, 3] = rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 1.0]
    d = 10.0 ** rng.uniform(-6, -0.5, n)
    delta = np.tile(np.eye(4), (n, 1, 1))
    delta[:, :3, :3] = Rotation.from_rotvec(rng.normal(0, 1.0, (n, 3)) * np.minimum(1.0, 2.5 * d)[:, None]).as_matrix()
    delta[:, :3, 3] = rng.normal(0, 1.0, (n, 3)) * d[:, None]
    return pts, gts @ delta, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--points", default="2620,8000")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--call-timeout", type=float, default=60.0, help="seconds one device call may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("--calls must be at least 5")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)

    import se3tracknet_amd as se3
    eng = se3.Engine(a.device, 1)
    cases = []
    for P in [int(x) for x in a.points.split(",")]:
        pts, preds, gts = scene(a.n, P, 7 + P)
        t0 = time.perf_counter()
        c_add, c_adds = se3.metrics.pose_errors(preds, gts, pts)            # the loop over metrics.add / metrics.adi, workers=-1
        cpu_s = time.perf_counter() - t0
        print("P = %d: CPU loop %.2f s" % (P, cpu_s), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        w_add, w_adds = se3.metrics.pose_errors(preds, gts, pts, workers=1)   # the same loop with one query thread per tree
        cpu1_s = time.perf_counter() - t0
        assert np.array_equal(w_add, c_add) and np.array_equal(w_adds, c_adds)
        print("P = %d: CPU loop, workers=1, %.2f s" % (P, cpu1_s), file=sys.stderr, flush=True)
        mp = eng.model_points(pts)
        times = []
        for k in range(a.calls + 1):                                        # the first call is the warm-up (staging grows there)
            faulthandler.dump_traceback_later(a.call_timeout, exit=True)
            t0 = time.perf_counter()
            d_add, d_adds = eng.pose_errors(mp, preds, gts)
            dt = time.perf_counter() - t0
            faulthandler.cancel_dump_traceback_later()
            if k:
                times.append(dt)
        mp.close()
        dev_s = float(np.median(times))
        cases.append({"n": a.n, "P": P, "cpu_s": round(cpu_s, 4), "cpu_s_workers_1": round(cpu1_s, 4), "device_s": round(dev_s, 6), "device_s_min": round(min(times), 6),
                      "device_s_max": round(max(times), 6), "calls": a.calls, "speedup": round(cpu_s / dev_s, 1),
                      "max_abs_diff_add": float(np.abs(d_add - c_add).max()), "max_abs_diff_adds": float(np.abs(d_adds - c_adds).max()),
                      "distance_evaluations_per_s": round(a.n * float(P) * P / dev_s, 0)})
    eng.close()
    print(json.dumps({"what": "pose_errors", "cpus": len(cpus), "cpu_evaluator": "metrics.add + metrics.adi (cKDTree, workers=-1)",
                      "device_call": "Engine.pose_errors (se3tn_pose_errors_host)", "cases": cases}))


if __name__ == "__main__":
    main()
