#!/usr/bin/env python3
"""Searching a product lattice of poses (se3tn_score_pose_grid) on the device: two cases, one JSON line each.

Data (that of scripts/pose_search_report.py): a model of --points points on an ellipsoid with its analytic normals, a 480 x 640 depth
frame holding the model splatted at its true pose before a wall at 900 mm with holes.

  (i)  "recover_lattice": the default 9,317-candidate lattice of Tracker.recover (7 rotations x 1,331 translations) from HOST arrays,
       through se3tn_search_pose_grid_host (the factors travel: 32 KB) and through se3tn_search_poses_host (the poses travel:
       1.2 MB) -- the second is the baseline, the call that existed before.  Same process, calls interleaved, facing off so that both
       compute the same records (checked).  Also both score kernels alone on device pointers, HIP events.
  (ii) "acquire_stage1": the stage-1 grid of Tracker.acquire, rotation_grid(40, 12) x 1,150 depth seeds = 552,000 candidates, facing
       on: score + rank on device pointers (HIP events) and the whole host call.  A sub-grid of 8 x 64 candidates is held to the numpy
       oracle (tests/pose_grid_oracle.py); the full grid in numpy would take minutes.

Each figure: median [min, max] of --windows timings after a warm-up.  The process is pinned to at most 16 CPUs before anything is
timed.  Every timed section runs under a watchdog that ends the process if it does not return.

    python scripts/pose_grid_report.py [--points 2620] [--top 8] [--tol 5] [--reps 20] [--windows 9]
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

RADII = np.array([0.06, 0.045, 0.035])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2620)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--tol", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
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
    import pose_grid_oracle as PGO
    import pose_search_oracle as PSO
    import se3tracknet_amd as se3
    from pose_search_report import H, W, K, scene
    if not torch.cuda.is_available():
        sys.exit("pose_grid_report: no GPU -- nothing is measured without one")
    pts, depth, true, lost = scene(a.points, 7 + a.points)
    nrm = pts / RADII ** 2                                  # the ellipsoid's gradient: outward, not of unit length
    k = a.top
    eng = se3.Engine(a.device, 1)
    mp = eng.model_points(pts, nrm)
    dev = "cuda:%d" % a.device
    depth_d = torch.from_numpy(depth.view(np.int16)).to(dev)
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    med = lambda x: float(np.median(x))   # noqa: E731
    stat = lambda name, x, nd: {name: round(med(x), nd), name + "_min": round(min(x), nd), name + "_max": round(max(x), nd)}   # noqa: E731

    def timed(fn):
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        return dt * 1e3, out

    def events(fn, reps):
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        faulthandler.cancel_dump_traceback_later()
        return e0.elapsed_time(e1) * 1e3 / reps

    def grid_call(rots_d, trans_d, fit_d, facing):
        assert eng.lib.se3tn_score_pose_grid(eng._h, mp._h, rots_d.numel() // 9, C.c_void_p(rots_d.data_ptr()), trans_d.numel() // 3,
                                             C.c_void_p(trans_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, a.tol, facing,
                                             C.c_void_p(fit_d.data_ptr()), st) == 0, eng.lib.se3tn_last_error()

    def rank_call(fit_d, n, idx_d):
        assert eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()), st) == 0

    # ---- (i) the recover lattice from host arrays, both entry points ------------------------------------------------------------------
    rots, trans = se3.recover.lattice_factors(lost)
    cands = se3.pose_lattice(lost)
    n = len(cands)
    grid_ms, poses_ms = [], []
    for w in range(a.windows + 1):                          # the first round is the warm-up (the staging grows there)
        dt_g, got_g = timed(lambda: eng.score_pose_grid(mp, rots, trans, depth, K, a.tol, top=k))
        dt_p, got_p = timed(lambda: eng.score_poses(mp, cands, depth, K, a.tol, top=k))
        if w:
            grid_ms.append(dt_g); poses_ms.append(dt_p)
    equal = bool(np.array_equal(got_g[0], got_p[0]) and got_g[1].tobytes() == got_p[1].tobytes())
    rots_d, trans_d = torch.from_numpy(rots.reshape(-1, 9).copy()).to(dev), torch.from_numpy(np.ascontiguousarray(trans)).to(dev)
    poses_d = torch.from_numpy(np.ascontiguousarray(cands.reshape(n, 16))).to(dev)
    fit_d = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    fit_p = torch.zeros((n, 8), dtype=torch.int32, device=dev)

    def poses_call():
        assert eng.lib.se3tn_score_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, a.tol,
                                         C.c_void_p(fit_p.data_ptr()), st) == 0

    grid_us, poses_us, facing_us = [], [], []
    for w in range(a.windows + 1):
        g = events(lambda: grid_call(rots_d, trans_d, fit_d, 0), a.reps)
        p = events(poses_call, a.reps)
        f = events(lambda: grid_call(rots_d, trans_d, fit_d, 1), a.reps)
        if w:
            grid_us.append(g); poses_us.append(p); facing_us.append(f)
    grid_call(rots_d, trans_d, fit_d, 0)
    equal = equal and bool(torch.equal(fit_d, fit_p))
    line = {"what": "pose_grid", "case": "recover_lattice", "cpus": len(cpus), "n_rot": len(rots), "n_trans": len(trans), "n": n, "P": a.points,
            "frame": [H, W], "k": k, "tol_mm": a.tol, "windows": a.windows, "reps_per_window": a.reps,
            "upload_bytes_grid": int(rots.nbytes + trans.nbytes + depth.nbytes), "upload_bytes_poses": int(cands.nbytes + depth.nbytes)}
    line.update(stat("grid_host_call_ms", grid_ms, 3)); line.update(stat("poses_host_call_ms", poses_ms, 3))
    line.update(stat("grid_score_us", grid_us, 2)); line.update(stat("poses_score_us", poses_us, 2)); line.update(stat("grid_score_facing_us", facing_us, 2))
    line.update(host_call_speedup=round(med(poses_ms) / med(grid_ms), 3), score_kernel_speedup=round(med(poses_us) / med(grid_us), 3),
                equal=equal)
    print(json.dumps(line), flush=True)

    # ---- (ii) the stage-1 grid of acquire, facing on ------------------------------------------------------------------------------------
    rots2 = se3.recover.rotation_grid(40, 12)
    seeds = se3.recover.depth_seeds(depth, K, 16, 0.03)[:1150]
    n2 = len(rots2) * len(seeds)
    rots2_d, seeds_d = torch.from_numpy(rots2.reshape(-1, 9).copy()).to(dev), torch.from_numpy(np.ascontiguousarray(seeds)).to(dev)
    fit2_d = torch.zeros((n2, 8), dtype=torch.int32, device=dev)
    idx2_d = torch.zeros((k,), dtype=torch.int32, device=dev)
    score2_us, both2_us, host2_ms = [], [], []
    reps2 = max(a.reps // 5, 2)
    for w in range(a.windows + 1):
        s = events(lambda: grid_call(rots2_d, seeds_d, fit2_d, 1), reps2)
        b = events(lambda: (grid_call(rots2_d, seeds_d, fit2_d, 1), rank_call(fit2_d, n2, idx2_d)), reps2)
        dt, got2 = timed(lambda: eng.score_pose_grid(mp, rots2, seeds, depth, K, a.tol, facing=True, top=k))
        if w:
            score2_us.append(s); both2_us.append(b); host2_ms.append(dt)
    fit2 = fit2_d.cpu().numpy().view(PSO.DTYPE).reshape(len(rots2), len(seeds))
    sub_r, sub_t = np.arange(0, len(rots2), 60), np.arange(0, len(seeds), 18)
    want = PGO.score(pts, nrm, rots2[sub_r], seeds[sub_t], depth, K, a.tol, 1).reshape(len(sub_r), len(sub_t))
    equal2 = bool(np.ascontiguousarray(fit2[sub_r][:, sub_t]).tobytes() == want.tobytes()
                  and np.array_equal(got2[0], idx2_d.cpu().numpy()) and got2[1].tobytes() == fit2.reshape(-1)[got2[0]].tobytes())
    best = int(got2[0][0])
    line = {"what": "pose_grid", "case": "acquire_stage1", "cpus": len(cpus), "n_rot": len(rots2), "n_trans": len(seeds), "n": n2, "P": a.points,
            "frame": [H, W], "k": k, "tol_mm": a.tol, "facing": 1, "windows": a.windows, "reps_per_window": reps2,
            "upload_bytes": int(rots2.nbytes + seeds.nbytes + depth.nbytes), "as_poses_bytes": int(n2 * 128)}
    line.update(stat("score_us", score2_us, 1)); line.update(stat("score_rank_us", both2_us, 1)); line.update(stat("host_call_ms", host2_ms, 3))
    line.update(projections_per_s=round(n2 * a.points / (med(score2_us) * 1e-6), 0), checked_against_oracle=int(want.size), equal=equal2,
                best_inliers=int(got2[1]["inlier_pts"][0]), best_facing_points=int(got2[1]["points"][0]),
                best_mm_from_truth=round(float(1000 * np.linalg.norm(seeds[best % len(seeds)] - true[:3, 3])), 2))
    print(json.dumps(line), flush=True)
    mp.close()
    eng.close()
    if not (equal and equal2):
        sys.exit("pose_grid_report: a device result differs from its reference")


if __name__ == "__main__":
    main()
