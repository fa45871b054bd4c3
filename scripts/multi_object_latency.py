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
nothing), so every frame renders the rectangles it starts with.  --passes N repeats the whole K list N times (run-to-run spread)."""
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
    ap.add_argument("--ks", default="1,2,3,4,5,8")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("route", nargs="?", default="vispy", choices=("vispy", "pyrender"))
    args = ap.parse_args()
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
    ks = [int(k) for k in args.ks.split(",")]
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


if __name__ == "__main__":
    main()
