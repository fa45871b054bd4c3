#!/usr/bin/env python3
"""K different objects in one camera frame: K separate Tracker.on_track calls (se3tn_on_track each) against ONE MultiTracker.on_track
(se3tn_on_track_objects), for K = 1..5 and 8.  The objects alternate between the two trained stand-ins (tests/golden/synth_tracker.npz,
30-degree regime; synth_tracker_5deg.npz, 5-degree regime: other weights, mean / std and normalisers) on the synthetic ellipsoid mesh,
each with its own pose near a common anchor.  Pose feedback as in tracking; ms per camera frame, median of `frames` frames after
`warmup`.  Both sides compute the same bits per object (tests/test_gpu_multi_object.py); the loop checks it on the first frames.
Prints one JSON line per K.

`multi_object_latency.py pyrender`: the same comparison on the full-frame (pyrender) route -- the reference's default configuration,
one textured model per class: textured spheres of 81,920 / 20,480 / 5,120 faces with textures of 64 x 128 / 128 x 256 / 256 x 256
texels (object i takes mesh i % 3), each with its own weights, on one 480 x 640 frame.  The poses are HELD (as `track_latency.py
pyrender` holds them, and for the same reason: with synthetic weights a fed-back pose leaves the frame, and an empty render costs
nothing), so every frame renders the rectangles it starts with.  --passes N repeats the whole K list N times (run-to-run spread).

`multi_object_latency.py live`: the live-camera front end for K = 1, 3, 5, 7 objects of one 480 x 640 frame with holes: per frame
grab_depth + grab_color + on_track of LiveMultiTracker, ONE library call (one_call=True: se3tn_on_track_objects_live) beside the
composition (one_call=False: engine.fill_depth through the host, the channel swap, MultiTracker.on_track), interleaved frame by frame
in the same process.  Both compute the same bits (tests/test_gpu_multi_object_live.py); the loop checks it on the first frames.
`--trace DIR` then counts the kernel launches of ONE frame at K = 3 per leg: one and two frames of the leg, each in a child process of
its own under `rocprofv3 --kernel-trace` (no counters), and the difference of the two dispatch counts."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import se3tracknet_amd as se3
from oracle import closed_loop as CL
from oracle import fixtures as Fx
from oracle import free_run as FR
from oracle import synth_track as ST


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ks", default=None, help="default 1,2,3,4,5,8 (live: 1,3,5,7)")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--trace", default=None, help="live: directory for the kernel traces of one frame per leg")
    ap.add_argument("--trace-child", default=None, help=argparse.SUPPRESS)   # LEG:FRAMES, what the traced child runs
    ap.add_argument("route", nargs="?", default="vispy", choices=("vispy", "pyrender", "live"))
    args = ap.parse_args()
    if args.ks is None:
        args.ks = "1,3,5,7" if args.route == "live" else "1,2,3,4,5,8"
    pyrender = args.route == "pyrender"
    models = []
    for regime in ("ycbineoat_30deg", "ycb_video_5deg"):
        sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights(regime))
        models.append((sd, mean, std) + tuple(CL.REGIMES[regime]))
    mesh = ST.make_object(4)
    textured = []
    if pyrender:
        for subdiv, tex_hw in ((6, (64, 128)), (5, (128, 256)), (4, (256, 256))):
            ms = Fx.textured_sphere(subdiv, 0.06, tex_hw)
            textured.append(dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"], uv=ms["uv"], texture=ms["texture"], kd=ms["kd"]))
    ks = [3] if args.trace_child else [int(k) for k in args.ks.split(",")]
    trackers = []
    for i in range(max(ks)):
        sd, mean, std, tn, rn = models[i % 2]
        info = dict(Fx.DATASET_INFO, object_width=ST.OBJECT_WIDTH_MM)
        if pyrender:
            info["renderer"] = "pyrenderer"
        t = se3.Tracker(info, mean, std, {"state_dict": sd}, trans_normalizer=tn, rot_normalizer=rn, max_samples=1)
        t.renderer = se3.HipRenderer(t.engine, textured[i % 3], mode="pyrender", frame_size=(480, 640)) if pyrender else se3.HipRenderer(t.engine, mesh)
        trackers.append(t)
    rgb, depth = Fx.structured_frame(401)
    if args.route == "live":
        return live_leg(args, ks, trackers)
    start = [Fx.pose(60 + i, (0.08 * np.cos(1.1 * i), 0.05 * np.sin(1.7 * i), 0.75 + 0.02 * i)) for i in range(max(ks))]
    for K in ks * args.passes:
        trks = trackers[:K]
        mt = se3.MultiTracker(trks)
        P_sep = [p.copy() for p in start[:K]]
        P_mul = np.stack(start[:K])
        sep, mul = [], []
        for f in range(args.warmup + args.frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N_sep = [t.on_track(P, rgb, depth) for t, P in zip(trks, P_sep)]
            t1 = time.perf_counter()
            N_mul = mt.on_track(P_mul, rgb, depth)
            t2 = time.perf_counter()
            if f < 3:
                assert all(np.array_equal(N_mul[i], N_sep[i]) for i in range(K)), "multi-object call differs from the single calls"
                if pyrender:
                    assert all(int((a.cpu().numpy() != 0).sum()) > 300 for a in mt.last_prediction["depthA"]), "an object is not in view"
            if not pyrender:    # (pyrender leg: the poses are held)
                P_sep, P_mul = N_sep, N_mul
            if f >= args.warmup:
                sep.append(t1 - t0)
                mul.append(t2 - t1)
            if f % 50 == 49:    # back to the start poses now and then: the frame does not move, the tracks would drift off it
                P_sep = [p.copy() for p in start[:K]]
                P_mul = np.stack(start[:K])
        mt.close()
        ms_sep, ms_mul = float(np.median(sep)) * 1e3, float(np.median(mul)) * 1e3
        print(json.dumps({"objects": K, "separate_on_track_ms": round(ms_sep, 4), "multi_on_track_ms": round(ms_mul, 4),
                          "speedup": round(ms_sep / ms_mul, 3), "separate_p95_ms": round(float(np.percentile(sep, 95)) * 1e3, 4),
                          "multi_p95_ms": round(float(np.percentile(mul, 95)) * 1e3, 4), "frames": args.frames, "warmup": args.warmup,
                          "route": args.route,
                          "note": "one 480x640 camera frame, K objects alternating the 30- / 5-degree trained stand-ins, %s; "
                                  "K x se3tn_on_track vs one se3tn_on_track_objects; median ms per frame"
                                  % ("textured spheres of %s faces on the full-frame route, poses held" % "/".join(str(len(m["faces"])) for m in textured)
                                     if pyrender else "ellipsoid mesh (%d faces)" % len(mesh["faces"]))}),
              flush=True)


def live_trace(trace_dir):
    import glob
    import shutil
    import subprocess
    prof = shutil.which("rocprofv3")
    if prof is None:
        print(json.dumps({"trace": "rocprofv3 not found: no kernel trace recorded"}))
        return
    for leg in ("composition", "one_call"):
        counts = []
        for frames in (1, 2):
            out = os.path.join(trace_dir, "%s_%d" % (leg, frames))
            subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "live",
                            "--trace-child", "%s:%d" % (leg, frames)], check=True, timeout=300)
            rows = 0
            for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
                with open(f) as fh:
                    rows += max(sum(1 for _ in fh) - 1, 0)
            counts.append(rows)
        print(json.dumps({"leg": leg, "objects": 3, "kernel_launches_per_frame": counts[1] - counts[0],
                          "dispatches_one_frame_run": counts[0], "dispatches_two_frame_run": counts[1], "trace": trace_dir}), flush=True)


def live_leg(args, ks, trackers):
    if args.trace_child:      # the traced child: FRAMES frames of one leg at K = 3
        leg, frames = args.trace_child.split(":")
        bgr, raw = Fx.synthetic_frame(230)
        P0 = np.stack([Fx.pose(60 + i, (0.08 * np.cos(1.1 * i), 0.05 * np.sin(1.7 * i), 0.75 + 0.02 * i)) for i in range(3)])
        lt = se3.LiveMultiTracker(se3.MultiTracker(trackers[:3]), P0, one_call=leg == "one_call")
        for f in range(int(frames)):
            lt.grab_depth(raw)
            lt.grab_color(bgr, stamp=float(f))
            lt.on_track()
            lt.A_in_cam = P0.copy()
        torch.cuda.synchronize()
        return
    bgr, raw = Fx.synthetic_frame(230)          # 480 x 640, 10 % holes / near / far pixels
    start = [Fx.pose(60 + i, (0.08 * np.cos(1.1 * i), 0.05 * np.sin(1.7 * i), 0.75 + 0.02 * i)) for i in range(max(ks))]
    for K in ks * args.passes:
        P0 = np.stack(start[:K])
        legs = [se3.LiveMultiTracker(se3.MultiTracker(trackers[:K]), P0, one_call=oc) for oc in (False, True)]
        times = ([], [])
        for f in range(args.warmup + args.frames):
            outs = []
            for lt, acc in zip(legs, times):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lt.grab_depth(raw)
                lt.grab_color(bgr, stamp=float(f))
                outs.append(lt.on_track())
                t1 = time.perf_counter()
                if f >= args.warmup:
                    acc.append(t1 - t0)
            if f < 3:
                assert np.array_equal(legs[0].A_in_cam, legs[1].A_in_cam), "the one call differs from the composition"
                assert np.array_equal(legs[0].depth, legs[1].depth), "the filled frames differ"
            if f % 50 == 49:    # back to the start poses now and then: the frame does not move, the tracks would drift off it
                for lt in legs:
                    lt.A_in_cam = P0.copy()
        for lt in legs:
            lt.tracker.close()
        ms = [float(np.median(t)) * 1e3 for t in times]
        print(json.dumps({"objects": K, "composition_ms": round(ms[0], 4), "one_call_ms": round(ms[1], 4), "speedup": round(ms[0] / ms[1], 3),
                          "composition_p95_ms": round(float(np.percentile(times[0], 95)) * 1e3, 4),
                          "one_call_p95_ms": round(float(np.percentile(times[1], 95)) * 1e3, 4), "frames": args.frames, "warmup": args.warmup,
                          "route": "live",
                          "note": "LiveMultiTracker grab_depth + grab_color + on_track per frame, one 480x640 frame with holes, K objects "
                                  "alternating the 30- / 5-degree trained stand-ins, bilateral; one_call=False (engine.fill_depth + channel swap + "
                                  "se3tn_on_track_objects) vs one_call=True (se3tn_on_track_objects_live), interleaved; median ms per frame"}),
              flush=True)
    if args.trace:
        live_trace(args.trace)


if __name__ == "__main__":
    main()
