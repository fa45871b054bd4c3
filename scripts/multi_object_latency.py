#!/usr/bin/env python3
"""K different objects in one camera frame: K separate Tracker.on_track calls (se3tn_on_track each) against ONE MultiTracker.on_track
(se3tn_on_track_objects), for K = 1..5 and 8.  The objects alternate between the two trained stand-ins (tests/golden/synth_tracker.npz,
30-degree regime; synth_tracker_5deg.npz, 5-degree regime: other weights, mean / std and normalisers) on the synthetic ellipsoid mesh,
each with its own pose near a common anchor.  Pose feedback as in tracking; ms per camera frame, median of `frames` frames after
`warmup`.  Both sides compute the same bits per object (tests/test_gpu_multi_object.py); the loop checks it on the first frames.
Prints one JSON line per K."""
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
    args = ap.parse_args()
    models = []
    for regime in ("ycbineoat_30deg", "ycb_video_5deg"):
        sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights(regime))
        models.append((sd, mean, std) + tuple(CL.REGIMES[regime]))
    mesh = ST.make_object(4)
    ks = [int(k) for k in args.ks.split(",")]
    trackers = []
    for i in range(max(ks)):
        sd, mean, std, tn, rn = models[i % 2]
        t = se3.Tracker(dict(Fx.DATASET_INFO, object_width=ST.OBJECT_WIDTH_MM), mean, std, {"state_dict": sd}, trans_normalizer=tn,
                        rot_normalizer=rn, max_samples=1)
        t.renderer = se3.HipRenderer(t.engine, mesh)
        trackers.append(t)
    rgb, depth = Fx.structured_frame(401)
    start = [Fx.pose(60 + i, (0.08 * np.cos(1.1 * i), 0.05 * np.sin(1.7 * i), 0.75 + 0.02 * i)) for i in range(max(ks))]
    for K in ks:
        trks = trackers[:K]
        mt = se3.MultiTracker(trks)
        P_sep = [p.copy() for p in start[:K]]
        P_mul = np.stack(start[:K])
        sep, mul = [], []
        for f in range(args.warmup + args.frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P_sep = [t.on_track(P, rgb, depth) for t, P in zip(trks, P_sep)]
            t1 = time.perf_counter()
            P_mul = mt.on_track(P_mul, rgb, depth)
            t2 = time.perf_counter()
            if f < 3:
                assert all(np.array_equal(P_mul[i], P_sep[i]) for i in range(K)), "multi-object call differs from the single calls"
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
                          "note": "one 480x640 camera frame, K objects alternating the 30- / 5-degree trained stand-ins, ellipsoid mesh "
                                  "(%d faces); K x se3tn_on_track vs one se3tn_on_track_objects; median ms per frame" % len(mesh["faces"])}),
              flush=True)


if __name__ == "__main__":
    main()
