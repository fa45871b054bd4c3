#!/usr/bin/env python3
"""Verifying pose hypotheses by colour (se3tn_verify_poses_host) on the device: one JSON line per number of hypotheses.

Data: the 20,480-face icosphere of the renderer tests (random vertex colours) on the window route, a 480 x 640 frame holding that
model's full-frame render at its true pose (another gain and offset, +-4 mm of depth noise) before a textured wall at 900 mm with holes.
The workload: --poses hypotheses (seeded perturbations of the true pose of up to 8 degrees and 8 mm per axis; every third one with
another rotation altogether).

  one call       Tracker.verify -> se3tn_verify_poses_host: windows, n renders in four launches, staging, the compare kernel, read-back;
  step by step   the same records through render_window per pose + Engine.color_stats (Tracker.verify with one_call = False), in the same
                 process, alternating with the one call;
  for scale      Tracker.on_track_batch of the same poses (random-init weights): verify is its front half, so this is the natural ceiling;
  kernel alone   --trace DIR: a child process of --reps one calls under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the
                 host), the colour kernel's durations read from the kernel trace it leaves in DIR: median [min, max] of ALL its launches.
                 A child that ends with a non-zero status ends the script: nothing more is started on the device after it.

The one call's records are held to the step-by-step path's, bytes.  Each figure: median [min, max] of --windows timings after a warm-up;
a host clock around a call that ends in a device synchronise.  The process is pinned to at most 16 CPUs before anything is timed.  Every
timed section runs under a watchdog that ends the process if it does not return.

    python scripts/color_fit_report.py [--poses 8 24] [--windows 31] [--trace DIR] [--reps 40]
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
WIDTH_MM = 170.0
TOL = 10


def setup(n, device):
    import se3tracknet_amd as se3
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    from scipy.spatial.transform import Rotation
    K = np.asarray(Fx.K_YCB, np.float64)
    mesh = Fx.icosphere(5, 0.05, 0)                                     # 20,480 faces
    info = dict(Fx.DATASET_INFO, object_width=WIDTH_MM, camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, max_samples=n, device=device)
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    true = Fx.pose(11, (0.02, -0.015, 0.6))
    painter = se3.HipRenderer(trk.engine, dict(mesh, kd=(1.0, 1.0, 1.0)), mode="pyrender", frame_size=(H, W))
    orgb, odep = painter.render_frame(true, K)
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.ascontiguousarray(Fx.structured_frame(7, H, W)[0]).copy()
    dep = (900 + 0.2 * (xx - W / 2) + 0.1 * (yy - H / 2)).astype(np.uint16)
    dep[rng.random((H, W)) < 0.04] = 0
    on = odep > 0
    rgb[on] = np.clip(orgb[on].astype(np.int64) * 3 // 4 + 30, 0, 255).astype(np.uint8)
    dep[on] = odep[on] + rng.integers(-4, 5, int(on.sum())).astype(np.uint16)
    hyps = np.tile(true, (n, 1, 1))
    for k, T in enumerate(hyps):
        if k % 3 == 2:
            T[:3, :3] = Fx.pose(40 + k, (0, 0, 1))[:3, :3]
        elif k:
            T[:3, :3] = Rotation.from_rotvec(np.deg2rad(rng.uniform(-8, 8, 3))).as_matrix() @ T[:3, :3]
        if k:
            T[:3, 3] += rng.uniform(-0.008, 0.008, 3)
    return se3, trk, hyps, np.ascontiguousarray(rgb), np.ascontiguousarray(dep)


def kernel_from_trace(trace_dir):
    """durations (us) of the colour kernel (fit_stats_kernel<true>; color_fit_kernel in builds before the two crop-record kernels became
    one) in the kernel-trace CSVs under trace_dir, by number of pairs (grid y)"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "color_fit_kernel" in r["Kernel_Name"] or "fit_stats_kernel<true>" in r["Kernel_Name"] or "fit_stats_kernel<true, false>" in r["Kernel_Name"]:
                out.setdefault(int(r["Grid_Size_Y"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[8, 24])
    ap.add_argument("--windows", type=int, default=31)
    ap.add_argument("--reps", type=int, default=40, help="one calls of the traced child process")
    ap.add_argument("--trace", default=None, help="directory for the kernel trace of a child process (kernel alone)")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)   # the traced child: --child n runs --reps one calls of n poses
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a timed section may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.windows < 30 and not a.child:
        ap.error("--windows must be at least 30")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)
    import torch
    if not torch.cuda.is_available():
        sys.exit("color_fit_report: no GPU -- nothing is measured without one")

    if a.child:
        se3, trk, hyps, rgb, dep = setup(a.child, a.device)
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        for _ in range(a.reps):
            trk.verify(hyps, rgb, dep, tol_mm=TOL)
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

    def stepwise(trk, hyps, rgb, dep):
        trk.one_call = False
        try:
            return trk.verify(hyps, rgb, dep, tol_mm=TOL)
        finally:
            trk.one_call = True

    bad = False
    for n in a.poses:
        se3, trk, hyps, rgb, dep = setup(n, a.device)
        one_ms, step_ms, track_ms = [], [], []
        for w in range(a.windows + 1):                      # the first round is the warm-up (the staging grows there)
            dt_o, got = timed(lambda: trk.verify(hyps, rgb, dep, tol_mm=TOL))
            dt_s, want = timed(lambda: stepwise(trk, hyps, rgb, dep))
            dt_t, _ = timed(lambda: trk.on_track_batch(list(hyps), [rgb] * n, [dep] * n))
            if w:
                one_ms.append(dt_o); step_ms.append(dt_s); track_ms.append(dt_t)
        equal = bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]))
        bad |= not equal
        line = {"what": "color_fit", "lib": os.path.basename(se3._lib.LIB_PATH), "cpus": len(cpus), "n": n, "faces": int(len(trk.renderer.mesh["faces"])),
                "frame": [H, W], "tol_mm": TOL, "windows": a.windows}
        line.update(stat("verify_one_call_ms", one_ms, 4)); line.update(stat("verify_step_by_step_ms", step_ms, 4))
        line.update(stat("on_track_batch_ms", track_ms, 4))
        line.update(compared_px=[int(v) for v in got[1]["px"]], score=[round(float(v), 4) for v in got[2]], equal=equal)
        if a.trace:
            prof = shutil.which("rocprofv3")
            if prof is None:
                line["kernel_us"] = "rocprofv3 not found: not measured"
            else:
                d = os.path.join(a.trace, "n%d" % n)
                os.makedirs(d, exist_ok=True)
                cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "verify", "--", sys.executable, os.path.abspath(__file__),
                       "--child", str(n), "--reps", str(a.reps), "--device", str(a.device)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:     # the child failed on the device (a fault, an abort, its watchdog): nothing more is started on it
                    print(json.dumps(line), flush=True)
                    sys.stderr.write(r.stderr[-4000:])
                    sys.exit("color_fit_report: the traced child process of %d poses ended with status %d -- stopping here" % (n, r.returncode))
                v = kernel_from_trace(d).get(n if n <= 32 else 32, [])
                if not v:
                    line["kernel_us"] = "no colour-kernel launch in the trace under %s: not measured" % d
                else:                     # every launch of the child counts, its first ones (the clock still ramping up) included
                    line.update(kernel_us=round(med(v), 2), kernel_us_min=round(min(v), 2), kernel_us_max=round(max(v), 2), kernel_launches=len(v))
        print(json.dumps(line), flush=True)
        del trk
    if bad:
        sys.exit("color_fit_report: the one call's records differ from the step-by-step path's")


if __name__ == "__main__":
    main()
