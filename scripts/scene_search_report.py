#!/usr/bin/env python3
"""The lattice search among tracked objects (se3tn_score_pose_grid_scene, se3tn_search_pose_grid_scene_host) on the device: one JSON
line.

Data (that of scripts/pose_grid_report.py): a model of --points points on an ellipsoid with its analytic normals, a 480 x 640 depth
frame holding the model splatted at its true pose before a wall at 900 mm with holes; the default 9,317-candidate lattice of
Tracker.recover (7 rotations x 1,331 translations) around the lost pose, facing on.  The occluder is the slab of
tests/color_fit_scene.py held 80 mm in front of the object, 30 mm aside: its render, composed by se3tn_scene_fit, is the scene frame.

  kernels   the scene-aware kernel against the plain se3tn_score_pose_grid kernel on the same lattice, model and frame: device
            pointers, HIP events, the two interleaved window by window in one process.
  host      the one-call entry (Engine.search_pose_grid_scene) against the step-by-step composition in the same process:
            Engine.scene_fit(..., scene=True) from the host frame (se3tn_scene_fit_host, the scene read back), then
            Engine.score_pose_grid(..., scene=scene, top=k) (upload, device search, se3tn_rank_poses, read-back).  Both must return the
            same indices and records (checked), and the device records are held to the numpy oracle (tests/scene_search_oracle.py) on
            a sub-grid.

Each figure: median [min, max] of --windows timings after a warm-up.  The process is pinned to at most 16 CPUs before anything is
timed.  Every timed section runs under a watchdog that ends the process if it does not return.

    python scripts/scene_search_report.py [--points 2620] [--top 8] [--tol 5] [--reps 20] [--windows 9]
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
    import color_fit_scene as CS
    import scene_search_oracle as SSO
    import se3tracknet_amd as se3
    from pose_search_report import H, W, K, scene as make_scene
    if not torch.cuda.is_available():
        sys.exit("scene_search_report: no GPU -- nothing is measured without one")
    pts, depth, true, lost = make_scene(a.points, 7 + a.points)
    nrm = pts / RADII ** 2                                  # the ellipsoid's gradient: outward, not of unit length
    k = a.top
    eng = se3.Engine(a.device, 2)
    mp = eng.model_points(pts, nrm)
    slab = se3.HipRenderer(eng, CS.box_mesh())
    occ = [(slab, CS.OBJECT_WIDTH_MM)]
    occ_pose = np.eye(4)
    occ_pose[:3, :3] = true[:3, :3]
    occ_pose[:3, 3] = true[:3, 3] + np.array([0.03, 0.0, -0.08])
    occ_poses = occ_pose[None]
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

    rots, trans = se3.recover.lattice_factors(lost)
    n = len(rots) * len(trans)
    _, _, scene = eng.scene_fit(occ, occ_poses, depth, K, tol_mm=a.tol, scene=True)
    scene_d = torch.from_numpy(scene.view(np.int16)).to(dev)
    rots_d, trans_d = torch.from_numpy(rots.reshape(-1, 9).copy()).to(dev), torch.from_numpy(np.ascontiguousarray(trans)).to(dev)
    fit_p = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    fit_s = torch.zeros((n, 8), dtype=torch.int32, device=dev)

    def plain_call():
        assert eng.lib.se3tn_score_pose_grid(eng._h, mp._h, len(rots), C.c_void_p(rots_d.data_ptr()), len(trans), C.c_void_p(trans_d.data_ptr()),
                                             C.c_void_p(depth_d.data_ptr()), H, W, Kp, a.tol, 1, C.c_void_p(fit_p.data_ptr()), st) == 0

    def scene_call():
        assert eng.lib.se3tn_score_pose_grid_scene(eng._h, mp._h, len(rots), C.c_void_p(rots_d.data_ptr()), len(trans),
                                                   C.c_void_p(trans_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), C.c_void_p(scene_d.data_ptr()),
                                                   H, W, Kp, a.tol, 1, C.c_void_p(fit_s.data_ptr()), st) == 0

    # ---- the two kernels, interleaved ---------------------------------------------------------------------------------------------------
    plain_us, scene_us = [], []
    for w in range(a.windows + 1):                          # the first round is the warm-up
        p = events(plain_call, a.reps)
        s = events(scene_call, a.reps)
        if w:
            plain_us.append(p); scene_us.append(s)
    got = fit_s.cpu().numpy().view(SSO.DTYPE).reshape(len(rots), len(trans))
    sub_r, sub_t = np.arange(0, len(rots), 3), np.arange(0, len(trans), 21)
    want = SSO.score(pts, nrm, rots[sub_r], trans[sub_t], depth, scene, K, a.tol, 1).reshape(len(sub_r), len(sub_t))
    equal = bool(np.ascontiguousarray(got[sub_r][:, sub_t]).tobytes() == want.tobytes())

    # ---- the host call against its step-by-step composition ----------------------------------------------------------------------------
    def steps():
        _, _, sc = eng.scene_fit(occ, occ_poses, depth, K, tol_mm=a.tol, scene=True)
        return eng.score_pose_grid(mp, rots, trans, depth, K, a.tol, facing=True, top=k, scene=sc)

    one_ms, steps_ms = [], []
    for w in range(a.windows + 1):                          # the first round is the warm-up (the staging grows there)
        dt_o, got_o = timed(lambda: eng.search_pose_grid_scene(mp, rots, trans, depth, K, occ, occ_poses, tol_mm=a.tol, facing=True, top=k))
        dt_s, got_s = timed(steps)
        if w:
            one_ms.append(dt_o); steps_ms.append(dt_s)
    equal = equal and bool(np.array_equal(got_o[0], got_s[0]) and got_o[1].tobytes() == got_s[1].tobytes()
                           and got_o[1].tobytes() == got.reshape(-1)[got_o[0]].tobytes())
    best = int(got_o[0][0])
    line = {"what": "scene_search", "cpus": len(cpus), "n_rot": len(rots), "n_trans": len(trans), "n": n, "P": a.points, "frame": [H, W], "k": k,
            "tol_mm": a.tol, "facing": 1, "n_occ": 1, "scene_px": int((scene > 0).sum()), "windows": a.windows, "reps_per_window": a.reps}
    line.update(stat("plain_score_us", plain_us, 2)); line.update(stat("scene_score_us", scene_us, 2))
    line.update(stat("one_call_ms", one_ms, 3)); line.update(stat("step_by_step_ms", steps_ms, 3))
    line.update(scene_over_plain=round(med(scene_us) / med(plain_us), 3), one_call_speedup=round(med(steps_ms) / med(one_ms), 3),
                checked_against_oracle=int(want.size), equal=equal, best_inliers=int(got_o[1]["inlier_pts"][0]),
                best_hidden=int(got_o[1]["hidden_pts"][0]), best_facing_points=int(got_o[1]["points"][0]),
                best_mm_from_truth=round(float(1000 * np.linalg.norm(trans[best % len(trans)] - true[:3, 3])), 2))
    print(json.dumps(line), flush=True)
    mp.close()
    eng.close()
    if not equal:
        sys.exit("scene_search_report: a device result differs from its reference")


if __name__ == "__main__":
    main()
