#!/usr/bin/env python3
"""The scene fit (se3tn_scene_fit / _host / se3tn_scene_stats) on the device, beside the per-object fit stage: one JSON line per number
of objects.

Data: --objects trackers (random-init weights; the ellipsoid and the icosphere of the multi-object tests, alternating) in front of a
480 x 640 camera; the frame is the scene the library itself composes from their meshes at the poses, +- 2 mm of integer noise, over
a wall at 900 mm, 4 % holes.

  host entry     MultiTracker.scene_fit on the numpy frame -> se3tn_scene_fit_host: upload, n renders in four launches, the kernel,
                 read-back of the records;
  device entry   Engine.scene_fit on the frame as a device tensor -> se3tn_scene_fit, and the read-back of the records;
  kernel call    Engine.scene_stats on layers rendered beforehand (se3tn_scene_stats into a device buffer, then a synchronise): the
                 launch and the wait included;
  kernel alone   --trace DIR: a child process of --reps device-entry calls under `rocprofv3 --kernel-trace --stats` (a run of its own:
                 tracing slows the host), scene_fit_kernel's durations read from the trace: median [min, max] of ALL its launches.  A
                 child that ends with a non-zero status ends the script: nothing more is started on the device after it;
  fit stage      MultiTracker.on_track with fit_check on and with it off, alternating in the same process: the difference of the
                 medians is what the per-object check costs a frame (four raster launches, one stats launch, one more wait).

The three routes' records are held equal.  Each figure: median [min, max] of --windows timings after a warm-up round; a host clock around
a call that ends in a device synchronise.  The process is pinned to at most 16 CPUs before anything is timed.  Every timed section runs
under a watchdog that ends the process if it does not return.

    python scripts/scene_fit_report.py [--objects 3 8] [--windows 31] [--trace DIR] [--reps 40]
"""
import argparse
import csv
import faulthandler
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
WIDTH_MM = 150.0
TOL = 10


def setup(n, device):
    import se3tracknet_amd as se3
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    from oracle import synth_track as ST
    K = np.asarray(Fx.K_YCB, np.float64)
    meshes = [ST.make_object(4), Fx.icosphere(3, 0.05, 1)]
    info = dict(Fx.DATASET_INFO, object_width=WIDTH_MM, camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
    models = []
    for s in range(2):                                                   # two models, used alternately (a model may appear several times)
        mean, std = Fx.mean_std(s)
        trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(s, head_gain=0.01)}, max_samples=1, device=device)
        trk.renderer = se3.HipRenderer(trk.engine, meshes[s])
        models.append(trk)
    mt = se3.MultiTracker([models[i % 2] for i in range(n)], device=device)
    # neighbours overlap: 60 mm apart at depths 40 mm apart, two rows
    poses = np.stack([Fx.pose(50 + i, (-0.09 + 0.06 * (i % 4), -0.03 + 0.07 * (i // 4), 0.62 + 0.04 * (i % 3))) for i in range(n)])
    zero = np.zeros((H, W), np.uint16)
    scene = mt.engine.scene_fit(mt._objs, poses, zero, K, tol_mm=TOL, scene=True)[2]
    rng = np.random.default_rng(9)
    dep = np.where(scene > 0, scene.astype(np.int64) + rng.integers(-2, 3, scene.shape), 900)
    dep[rng.random((H, W)) < 0.04] = 0
    rgb = np.ascontiguousarray(Fx.structured_frame(7, H, W)[0])
    return se3, mt, poses, rgb, np.ascontiguousarray(dep.astype(np.uint16)), K, meshes


def kernel_from_trace(trace_dir):
    """durations (us) of scene_fit_kernel in the kernel-trace CSVs under trace_dir"""
    out = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "scene_fit_kernel" in r["Kernel_Name"]:
                out.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--windows", type=int, default=31)
    ap.add_argument("--reps", type=int, default=40, help="device-entry calls of the traced child process")
    ap.add_argument("--trace", default=None, help="directory for the kernel trace of a child process (kernel alone)")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)   # the traced child: --child n runs --reps calls of n objects
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a timed section may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.windows < 30 and not a.child:
        ap.error("--windows must be at least 30")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)
    import torch
    if not torch.cuda.is_available():
        sys.exit("scene_fit_report: no GPU -- nothing is measured without one")

    if a.child:
        se3, mt, poses, rgb, dep, K, meshes = setup(a.child, a.device)
        dep_dev = torch.from_numpy(dep.view(np.int16)).cuda()
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        for _ in range(a.reps):
            mt.scene_fit(poses, dep_dev, tol_mm=TOL)
        faulthandler.cancel_dump_traceback_later()
        return

    med = lambda x: float(np.median(x))   # noqa: E731
    stat = lambda name, x, nd: {name: round(med(x), nd), name + "_min": round(min(x), nd), name + "_max": round(max(x), nd)}   # noqa: E731

    def timed(fn):
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        return dt * 1e3, out

    bad = False
    for n in a.objects:
        se3, mt, poses, rgb, dep, K, meshes = setup(n, a.device)
        dep_dev = torch.from_numpy(dep.view(np.int16)).cuda()
        # the layers of the kernel call: every object's rectangle of the full-frame render, on the device
        painters = [se3.HipRenderer(mt.engine, m, mode="pyrender", frame_size=(H, W)) for m in meshes]
        rects = [se3.frame_rect(P, K, WIDTH_MM, H, W) or (0, 0, 0, 0) for P in poses]
        layers = [painters[i % 2].render_frame_rect(P, K, r, device=True)[1] if r[2] > r[0] else None for i, (P, r) in enumerate(zip(poses, rects))]
        buf = torch.empty((n, 48), dtype=torch.uint8, device="cuda")
        host_ms, dev_ms, call_ms, on_ms, off_ms = [], [], [], [], []
        for w in range(a.windows + 1):                      # the first round is the warm-up (the buffers grow there)
            dt_h, rec_h = timed(lambda: mt.scene_fit(poses, dep, tol_mm=TOL))
            dt_d, rec_d = timed(lambda: mt.scene_fit(poses, dep_dev, tol_mm=TOL))
            dt_k, _ = timed(lambda: mt.engine.scene_stats(layers, rects, dep_dev, TOL, ids=False, scene=False, out=buf))
            mt.fit_check = TOL
            dt_on, _ = timed(lambda: mt.on_track(poses, rgb, dep))
            mt.fit_check = None
            dt_off, _ = timed(lambda: mt.on_track(poses, rgb, dep))
            if w:
                host_ms.append(dt_h); dev_ms.append(dt_d); call_ms.append(dt_k); on_ms.append(dt_on); off_ms.append(dt_off)
        rec_k = buf.cpu().numpy().reshape(-1).view(se3._lib.SCENE_FIT_DTYPE)
        equal = bool(rec_h.tobytes() == rec_d.tobytes() == rec_k.tobytes())
        bad |= not equal
        line = {"what": "scene_fit", "lib": os.path.basename(se3._lib.LIB_PATH), "cpus": len(cpus), "n": n, "frame": [H, W], "tol_mm": TOL,
                "windows": a.windows, "faces": [int(len(t.renderer.mesh["faces"])) for t in mt.trackers[:2]]}
        line.update(stat("scene_fit_host_ms", host_ms, 4)); line.update(stat("scene_fit_device_ms", dev_ms, 4))
        line.update(stat("scene_stats_call_ms", call_ms, 4))
        line.update(stat("on_track_fit_on_ms", on_ms, 4)); line.update(stat("on_track_fit_off_ms", off_ms, 4))
        line.update(fit_stage_ms=round(med(on_ms) - med(off_ms), 4), visible_px=[int(v) for v in rec_h["visible_px"]],
                    hidden_px=[int(v) for v in rec_h["hidden_px"]], inlier_px=[int(v) for v in rec_h["inlier_px"]], equal=equal)
        if a.trace:
            prof = shutil.which("rocprofv3")
            if prof is None:
                line["kernel_us"] = "rocprofv3 not found: not measured"
            else:
                d = os.path.join(a.trace, "n%d" % n)
                os.makedirs(d, exist_ok=True)
                cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "scene", "--", sys.executable, os.path.abspath(__file__),
                       "--child", str(n), "--reps", str(a.reps), "--device", str(a.device)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:     # the child failed on the device (a fault, an abort, its watchdog): nothing more is started on it
                    print(json.dumps(line), flush=True)
                    sys.stderr.write(r.stderr[-4000:])
                    sys.exit("scene_fit_report: the traced child process of %d objects ended with status %d -- stopping here" % (n, r.returncode))
                v = kernel_from_trace(d)
                if not v:
                    line["kernel_us"] = "no scene_fit_kernel launch in the trace under %s: not measured" % d
                else:                     # every launch of the child counts, its first ones (the clock still ramping up) included
                    line.update(kernel_us=round(med(v), 2), kernel_us_min=round(min(v), 2), kernel_us_max=round(max(v), 2), kernel_launches=len(v))
        print(json.dumps(line), flush=True)
        mt.close()
        del mt
    if bad:
        sys.exit("scene_fit_report: the records of the host entry, the device entry and the kernel call differ")


if __name__ == "__main__":
    main()
