#!/usr/bin/env python3
"""Aligning pose hypotheses to the depth frame (se3tn_align_poses) on the device: one JSON line.

Data (that of scripts/pose_grid_report.py): a model of --points points on an ellipsoid with its analytic normals, a 480 x 640 depth
frame holding the model splatted at its true pose before a wall at 900 mm with holes.  The workload: --poses hypotheses (seeded
perturbations of the true pose of up to 8 degrees and 8 mm per axis), --iters iterations each, stop 0 so that every pose runs them all.

  device entry   se3tn_align_poses on device pointers, a host clock around the call and a stream synchronise;
  kernel alone   the same call --reps times back to back between two HIP events, per call;
  host entry     se3tn_align_poses_host from host arrays: upload, launch, read-back, synchronise;
  for scale      the numpy oracle (tests/pose_align_oracle.py) on the same host, and one Tracker.on_track_batch of --poses poses
                 (random-init weights, the built-in rasteriser on a small mesh) in the same process.

The device result is held to the oracle, bytes.  Each figure: median [min, max] of --windows timings after a warm-up.  The process is
pinned to at most 16 CPUs before anything is timed.  Every timed section runs under a watchdog that ends the process if it does not
return.

The thread count per pose is a constant of csrc/pose_align_plan.h.  To time the other variant build a second library --
    hipcc <the flags csrc/Makefile gives pose_align.hip> -DSE3TN_PA_THREADS=1024 -c csrc/pose_align.hip -o /tmp/pa1024.o
    hipcc -shared -fPIC --offload-arch=gfx950 -o /tmp/lib1024.so <the other objects of csrc/build> /tmp/pa1024.o
-- and run this script once per library, alternating:  SE3TN_LIB=/tmp/lib1024.so python scripts/pose_align_report.py --threads 1024

    python scripts/pose_align_report.py [--points 2620] [--poses 8] [--iters 20] [--reps 20] [--windows 31] [--threads N]
"""
import argparse
import faulthandler
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

RADII = np.array([0.06, 0.045, 0.035])


def plan_threads():
    src = open(os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc", "pose_align_plan.h")).read()
    return int(re.search(r"#define SE3TN_PA_THREADS (\d+)", src).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2620)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=31)
    ap.add_argument("--threads", type=int, default=None, help="label of the library under SE3TN_LIB (default: the plan header's constant)")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a timed section may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.windows < 30:
        ap.error("--windows must be at least 30")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)

    import ctypes as C
    import torch
    from scipy.spatial.transform import Rotation
    import pose_align_oracle as PAO
    import pose_grid_scene as SC
    import se3tracknet_amd as se3
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    from pose_search_report import H, W, K, scene
    if not torch.cuda.is_available():
        sys.exit("pose_align_report: no GPU -- nothing is measured without one")
    L = se3._lib
    pts, depth, true, _ = scene(a.points, 7 + a.points)
    nrm = pts / RADII ** 2                                  # the ellipsoid's gradient: outward ...
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]             # ... of unit length: a normal of length L weights its point by L^2, and
                                                            # the gradient's 300 to 800 would run into the clamp of fx() at 256
    rng = np.random.default_rng(83)
    hyps = np.tile(true, (a.poses, 1, 1))
    for T in hyps:
        T[:3, :3] = Rotation.from_rotvec(np.deg2rad(rng.uniform(-8, 8, 3))).as_matrix() @ T[:3, :3]
        T[:3, 3] += rng.uniform(-0.008, 0.008, 3)
    n = a.poses
    prm = dict(gate_mm=20, iters=a.iters, min_pairs=12, damping=1e-6, stop=0.0)
    eng = se3.Engine(a.device, 1)
    mp = eng.model_points(pts, nrm)
    dev = "cuda:%d" % a.device
    depth_d = torch.from_numpy(depth.view(np.int16)).to(dev)
    poses_d = torch.from_numpy(np.ascontiguousarray(hyps.reshape(n, 16))).to(dev)
    out_d = torch.zeros((n, 16), dtype=torch.float64, device=dev)
    rec_d = torch.zeros((n, 40), dtype=torch.uint8, device=dev)
    sums_d = torch.zeros((n, 28), dtype=torch.int64, device=dev)
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    cp = L.AlignParams(prm["gate_mm"], prm["iters"], prm["min_pairs"], 0, prm["damping"], prm["stop"])
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

    def device_call():
        assert eng.lib.se3tn_align_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, C.byref(cp),
                                         C.c_void_p(out_d.data_ptr()), C.c_void_p(rec_d.data_ptr()), C.c_void_p(sums_d.data_ptr()), st) == 0

    def device_entry():
        device_call()
        torch.cuda.synchronize()

    # for scale: one on_track_batch of n poses -- random-init weights, the built-in rasteriser on the L mesh of the tests
    info = dict(Fx.DATASET_INFO, object_width=180.0, camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, max_samples=n, device=a.device)
    trk.renderer = se3.HipRenderer(trk.engine, SC.l_mesh())
    rgb = np.ascontiguousarray(Fx.structured_frame(7, H, W)[0])

    dev_ms, kern_us, host_ms, track_ms = [], [], [], []
    for w in range(a.windows + 1):                          # the first round is the warm-up (the staging grows there)
        dt_d, _ = timed(device_entry)
        k_us = events(device_call, a.reps)
        dt_h, got_h = timed(lambda: eng.align_poses(mp, hyps, depth, K, sums=True, **prm))
        dt_t, _ = timed(lambda: trk.on_track_batch(list(hyps), [rgb] * n, [depth] * n))
        if w:
            dev_ms.append(dt_d); kern_us.append(k_us); host_ms.append(dt_h); track_ms.append(dt_t)
    oracle_ms = []
    for w in range(3):
        dt_o, want = timed(lambda: PAO.align(pts, nrm, hyps, depth, K, **prm))
        oracle_ms.append(dt_o)
    rec = rec_d.cpu().numpy().view(L.ALIGN_REC_DTYPE).reshape(n)
    equal = bool(out_d.cpu().numpy().tobytes() == want[0].tobytes() and rec.tobytes() == want[1].tobytes()
                 and sums_d.cpu().numpy().tobytes() == want[2].tobytes()
                 and all(np.asarray(g).tobytes() == w_.tobytes() for g, w_ in zip(got_h, want)))
    errs = np.array([PAO.pose_error(o, true) for o in want[0]])
    line = {"what": "pose_align", "threads": a.threads or plan_threads(), "lib": os.path.basename(L.LIB_PATH), "cpus": len(cpus), "n": n, "P": a.points,
            "frame": [H, W], "iters": a.iters, "stop": 0.0, "gate_mm": 20, "windows": a.windows, "reps_per_window": a.reps}
    line.update(stat("device_entry_ms", dev_ms, 4)); line.update(stat("kernel_us", kern_us, 2)); line.update(stat("host_entry_ms", host_ms, 4))
    line.update(stat("numpy_oracle_ms", oracle_ms, 1)); line.update(stat("on_track_batch_ms", track_ms, 3))
    line.update(kernel_us_per_iteration=round(med(kern_us) / a.iters, 2), iterations=[int(v) for v in rec["iterations"]],
                pairs_first_last=[int(rec["pairs0"].min()), int(rec["pairs"].min())], worst_mm_from_truth=round(float(1000 * errs[:, 0].max()), 3),
                worst_deg_from_truth=round(float(errs[:, 1].max()), 4), equal=equal)
    print(json.dumps(line), flush=True)
    mp.close()
    eng.close()
    if not equal:
        sys.exit("pose_align_report: a device result differs from the oracle")


if __name__ == "__main__":
    main()
