#!/usr/bin/env python3
"""Re-acquiring a lost object: the device search (se3tn_score_poses + se3tn_rank_poses) against the numpy oracle of the tests
(tests/pose_search_oracle.py: the same rule, vectorised float64) on the same seeded data and the same host.

Data: a model of --points points (2,620: a YCB points.xyz), a 480 x 640 depth frame holding the model splatted at its true pose
before a wall at 900 mm with holes, and the default lattice of Tracker.recover around a lost pose (9,317 candidates: +-50 mm in
10 mm steps, identity and +-15 degrees about each camera axis).

Prints one JSON line:
  device_us         score + rank (k = --top) on device pointers, HIP events around --reps back-to-back iterations on one stream,
                    per iteration; median [min, max] of --windows windows after a warm-up window
  host_call_ms      one Engine.score_poses(..., top=k) call from host arrays (se3tn_search_poses_host: upload of the poses and the
                    whole frame, the two launches, read-back, wait), host clock, median of --windows calls after a warm-up call
  oracle_s          the numpy oracle's score + sort of the same candidates (chunks of 1,024 poses), once
  equal             the device's k indices and records equal the oracle's
The process is pinned to at most 16 CPUs before anything is timed.  Every timed section runs under a watchdog that ends the process
if it does not return.

    python scripts/pose_search_report.py [--points 2620] [--top 8] [--tol 5] [--reps 50] [--windows 9]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640
K = np.array([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1.0]])   # the YCB-Video camera


def scene(P, seed):
    """model points on an ellipsoid (radii 60 x 45 x 35 mm), the depth frame and (true pose, lost pose)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(P, 3))
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * np.array([0.06, 0.045, 0.035])
    true = np.eye(4)
    true[:3, :3] = Rotation.from_rotvec([0.4, -0.3, 0.2]).as_matrix()
    true[:3, 3] = [0.03, -0.02, 0.7]
    lost = true.copy()
    lost[:3, :3] = Rotation.from_rotvec([0.1, 0.2, -0.15]).as_matrix() @ true[:3, :3]
    lost[:3, 3] += [0.033, -0.024, 0.046]
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (900 + 0.05 * (xx - W / 2) + 0.03 * (yy - H / 2)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.04] = 0
    # the visible surface: a dense sample of the ellipsoid at the true pose, nearest point per pixel, splatted 5 x 5
    d = rng.normal(size=(200000, 3))
    dense = d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([0.06, 0.045, 0.035])
    c = dense @ true[:3, :3].T + true[:3, 3]
    u = np.rint(c[:, 0] * K[0, 0] / c[:, 2] + K[0, 2]).astype(int)
    vv = np.rint(c[:, 1] * K[1, 1] / c[:, 2] + K[1, 2]).astype(int)
    z = np.rint(c[:, 2] * 1000).astype(np.int64)
    surf = np.full((H, W), 65535, np.int64)
    for du in range(-2, 3):
        for dv in range(-2, 3):
            ok = (u + du >= 0) & (u + du < W) & (vv + dv >= 0) & (vv + dv < H)
            np.minimum.at(surf, (vv[ok] + dv, u[ok] + du), z[ok])
    depth[surf < 65535] = surf[surf < 65535].astype(np.uint16)
    return pts, depth, true, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2620)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--tol", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a timed section may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.windows < 5:
        ap.error("--windows must be at least 5")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)

    import ctypes as C
    import torch
    import pose_search_oracle as PSO
    import se3tracknet_amd as se3
    if not torch.cuda.is_available():
        sys.exit("pose_search_report: no GPU -- nothing is measured without one")
    pts, depth, true, lost = scene(a.points, 7 + a.points)
    cands = se3.pose_lattice(lost)
    n, k = len(cands), a.top

    t0 = time.perf_counter()
    want = np.concatenate([PSO.score(pts, cands[i:i + 1024], depth, K, a.tol) for i in range(0, n, 1024)])
    want_idx = PSO.rank(want, k)
    oracle_s = time.perf_counter() - t0
    print("oracle: %.2f s; best candidate %d, %d inliers of %d, %.1f mm from the true translation" % (
        oracle_s, want_idx[0], want["inlier_pts"][want_idx[0]], a.points,
        1000 * np.linalg.norm(cands[want_idx[0]][:3, 3] - true[:3, 3])), file=sys.stderr, flush=True)

    eng = se3.Engine(a.device, 1)
    mp = eng.model_points(pts)
    # the host entry point
    host_ms = []
    for w in range(a.windows + 1):                                        # the first call is the warm-up (staging grows there)
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        t0 = time.perf_counter()
        idx, fit = eng.score_poses(mp, cands, depth, K, a.tol, top=k)
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        if w:
            host_ms.append(dt * 1e3)
    equal = bool(np.array_equal(idx, want_idx) and fit.tobytes() == want[want_idx].tobytes())
    # the device entry points, HIP events
    dev = "cuda:%d" % a.device
    poses_d = torch.from_numpy(np.ascontiguousarray(cands.reshape(n, 16))).to(dev)
    depth_d = torch.from_numpy(depth.view(np.int16)).to(dev)
    fit_d = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    idx_d = torch.zeros((k,), dtype=torch.int32, device=dev)
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def once():
        rc = eng.lib.se3tn_score_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, a.tol,
                                       C.c_void_p(fit_d.data_ptr()), st)
        rc = rc or eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()), st)
        assert rc == 0, eng.lib.se3tn_last_error()

    dev_us, score_us = [], []
    for w in range(a.windows + 1):
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            once()
        e1.record()
        e1.synchronize()
        if w:
            dev_us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        # the score launch alone
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            assert eng.lib.se3tn_score_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp,
                                             a.tol, C.c_void_p(fit_d.data_ptr()), st) == 0
        e1.record()
        e1.synchronize()
        faulthandler.cancel_dump_traceback_later()
        if w:
            score_us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    equal = equal and bool(np.array_equal(idx_d.cpu().numpy(), want_idx)
                           and fit_d.cpu().numpy().view(PSO.DTYPE).reshape(n).tobytes() == want.tobytes())
    mp.close()
    eng.close()
    med = lambda x: float(np.median(x))   # noqa: E731
    print(json.dumps({"what": "pose_search", "cpus": len(cpus), "n": n, "P": a.points, "frame": [H, W], "k": k, "tol_mm": a.tol,
                      "reps_per_window": a.reps, "windows": a.windows,
                      "device_us": round(med(dev_us), 2), "device_us_min": round(min(dev_us), 2), "device_us_max": round(max(dev_us), 2),
                      "score_only_us": round(med(score_us), 2), "projections_per_s": round(n * a.points / (med(score_us) * 1e-6), 0),
                      "host_call_ms": round(med(host_ms), 3), "host_call_ms_min": round(min(host_ms), 3), "host_call_ms_max": round(max(host_ms), 3),
                      "oracle_s": round(oracle_s, 3), "oracle_over_device": round(oracle_s / (med(dev_us) * 1e-6), 0),
                      "oracle_over_host_call": round(oracle_s / (med(host_ms) * 1e-3), 1), "equal": equal,
                      "best_inliers": int(want["inlier_pts"][want_idx[0]]),
                      "best_mm_from_truth": round(float(1000 * np.linalg.norm(cands[want_idx[0]][:3, 3] - true[:3, 3])), 2)}))
    if not equal:
        sys.exit("pose_search_report: the device result differs from the oracle")


if __name__ == "__main__":
    main()
