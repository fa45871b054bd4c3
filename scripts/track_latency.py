#!/usr/bin/env python3
"""Latency of the drop-in Tracker.on_track (batch 1, pose feedback) on one MI355X with a stub
renderer (pre-rendered arrays): what BASELINE config 3 would report as Hz if YCB-Video and a
renderer were available.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import se3tracknet_amd as se3
from oracle import fixtures as Fx
from oracle import se3_oracle as O


class StubRenderer:
    def __init__(self):
        self.rgb, self.depth = Fx.synthetic_render(1, 0.8)

    def render(self, ob2cam, K, window):
        return self.rgb, self.depth


def main(frames=300, faces_subdiv=None, f16x3=False, pyrender=False, one_call=None, fit_check=None, winograd=None):
    mean, std = Fx.mean_std(0)
    sd = {"state_dict": O.make_state_dict(0, head_gain=0.0005)}
    if faces_subdiv is None:
        trk = se3.Tracker(Fx.DATASET_INFO, mean, std, sd, renderer=StubRenderer())
        rdesc = "stub renderer (pre-rendered arrays)"
    elif pyrender:
        # the reference's default configuration (dataset_info.yml `renderer: pyrenderer`): textured model through the full-frame
        # renderer, image A = crop of the render (predict.py:209-213); YCB-size face count, 480 x 640 frame
        ms = Fx.textured_sphere(faces_subdiv, 0.06)
        trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0, renderer="pyrenderer"), mean, std, sd)
        trk.renderer = se3.HipRenderer(trk.engine, dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"], uv=ms["uv"],
                                                        texture=ms["texture"], kd=ms["kd"]), mode="pyrender", frame_size=(480, 640))
        if one_call is not None:
            trk.one_call = bool(one_call)
        rdesc = "pyrender route (full-frame HIP rasteriser, textured), %d faces, one_call=%s" % (len(ms["faces"]), trk.one_call)
    else:  # full pipeline: HIP rasteriser on an icosphere with 20 * 4^subdiv faces (YCB scans: ~1e5 faces)
        from oracle import raster_oracle as R
        mesh = R.icosphere(faces_subdiv, 0.06, 0)
        trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, sd)
        trk.renderer = se3.HipRenderer(trk.engine, mesh)
        rdesc = "HIP rasteriser, %d faces, rendered A stays on the device" % len(mesh["faces"])
    if f16x3:
        trk.engine.set_precision(se3._lib.PREC_F16X3)
        rdesc += ", SE3TN_PREC_F16X3"
    if winograd:    # (min_batch, tile): se3tn_set_winograd -- (1, 4) / (1, 6) run one pair through the fused head block and its own tail
        trk.engine.set_winograd(*winograd)
        rdesc += ", set_winograd%s" % (tuple(winograd),)
    if fit_check:   # every call also renders the estimate and scores it against the observed depth (se3tn_set_fit_check)
        trk.fit_check = int(fit_check)
        rdesc += ", fit_check = %d mm" % trk.fit_check
    rgb, depth = Fx.synthetic_frame(3)
    P = Fx.pose(3)
    for _ in range(20):
        P = trk.on_track(P, rgb, depth)
    P = Fx.pose(3)
    torch.cuda.synchronize()
    lat = []
    for _ in range(frames):
        t0 = time.perf_counter()
        Pn = trk.on_track(P, rgb, depth)
        lat.append(time.perf_counter() - t0)
        if not pyrender:   # (pyrender leg: the pose is held, so the rendered rectangle stays the 200 x 200 pixels it starts with --
            P = Pn         # with these synthetic weights the fed-back pose leaves the frame, and an empty render costs nothing)
    lat = np.array(lat) * 1e3
    # device-only time of one batch-1 infer (HIP events inside the library)
    trk.engine.profile_enable(1)
    trk.on_track(P, rgb, depth)
    conv_ms, _, tot_ms = trk.engine.profile_read(0)
    print(json.dumps({"on_track_ms_median": round(float(np.median(lat)), 4), "on_track_ms_p95": round(float(np.percentile(lat, 95)), 4),
                      "hz_median": round(1000.0 / float(np.median(lat)), 1), "device_infer_ms": round(tot_ms, 4),
                      "device_conv_ms": round(conv_ms, 4), "frames": frames,
                      "note": "batch 1, 480x640 frame uploaded per call (pageable H2D), %s, pose D2H sync per frame" % rdesc}))


def _live_tracker():
    from oracle import raster_oracle as R
    mean, std = Fx.mean_std(0)
    mesh = R.icosphere(6, 0.06, 0)                                   # 81,920 faces
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.0005)})
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    return trk, len(mesh["faces"])


def live(frames=300, passes=2, trace_dir=None):
    """The live-camera front end (predict_ros.TrackerRos) per frame: grab_depth + grab_color + on_track of LiveTracker step by step
    (fill_depth as 10-13 launches, the filled frame to the host and its window back up) against one_call=True (se3tn_on_track_live).
    Built-in rasteriser, 480 x 640 synthetic frames with holes; the legs alternate in one session, one JSON line per leg and pass.
    trace_dir: one frame of each leg in a child process of its own under `rocprofv3 --kernel-trace --stats` (no counters)."""
    trk, faces = _live_tracker()
    seq = [Fx.synthetic_frame(200 + i) for i in range(8)]
    seq = [(np.ascontiguousarray(rgb[:, :, ::-1]), depth) for rgb, depth in seq]      # as CvBridge 'bgr8' delivers them
    P0 = Fx.pose(3)
    legs = [("step_by_step", se3.LiveTracker(trk, P0)), ("one_call", se3.LiveTracker(trk, P0, one_call=True))]
    assert legs[1][1].one_call

    def frame(lt, i):
        bgr, depth = seq[i % len(seq)]
        lt.grab_depth(depth)
        lt.grab_color(bgr, stamp=float(i))
        return lt.on_track()

    for p in range(passes):
        for name, lt in legs:
            lt.reset(P0)
            for i in range(20):
                frame(lt, i)
            lt.reset(P0)
            torch.cuda.synchronize()
            lat = []
            for i in range(frames):
                t0 = time.perf_counter()
                frame(lt, i)
                lat.append(time.perf_counter() - t0)
            lat = np.array(lat) * 1e3
            print(json.dumps({"leg": name, "pass": p, "frame_ms_median": round(float(np.median(lat)), 4),
                              "frame_ms_p95": round(float(np.percentile(lat, 95)), 4), "hz_median": round(1000.0 / float(np.median(lat)), 1),
                              "frames": frames, "note": "LiveTracker grab_depth + grab_color + on_track per frame, 480x640 frames with holes, "
                              "HIP rasteriser, %d faces, pose fed back" % faces}), flush=True)
    if trace_dir:
        import shutil
        import subprocess
        prof = shutil.which("rocprofv3")
        if prof is None:
            print(json.dumps({"trace": "rocprofv3 not found: no kernel trace recorded"}))
            return
        for name, _ in legs:
            out = os.path.join(trace_dir, name)
            subprocess.run([prof, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), "live-frame", name],
                           check=True, timeout=300)
            print(json.dumps({"trace": out, "leg": name}), flush=True)


def live_frame(leg):
    """what the traced child runs: two frames of one leg (the first pays the start-up allocations)"""
    trk, _ = _live_tracker()
    lt = se3.LiveTracker(trk, Fx.pose(3), one_call=leg == "one_call")
    for i in range(2):
        rgb, depth = Fx.synthetic_frame(200 + i)
        lt.grab_depth(depth)
        lt.grab_color(np.ascontiguousarray(rgb[:, :, ::-1]), stamp=float(i))
        lt.on_track()
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:2] == ["live"]:          # `track_latency.py live [--trace DIR]`: the live-camera front end, both legs
        live(trace_dir=sys.argv[3] if sys.argv[2:3] == ["--trace"] and len(sys.argv) > 3 else None)
        sys.exit(0)
    if sys.argv[1:2] == ["live-frame"]:
        live_frame(sys.argv[2])
        sys.exit(0)
    if sys.argv[1:2] == ["fit"]:           # `track_latency.py fit [TOL_MM]`: window route and pyrender route, fit check off, then on
        tol = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        for check in (None, tol):
            main(faces_subdiv=6, fit_check=check)
            main(faces_subdiv=6, pyrender=True, fit_check=check)
        sys.exit(0)
    if sys.argv[1:2] == ["wino"]:          # `track_latency.py wino [TILE]`: window route, 200 frames under se3tn_set_winograd(1, TILE)
        main(frames=200, faces_subdiv=6, winograd=(1, int(sys.argv[2]) if len(sys.argv) > 2 else 4))
        sys.exit(0)
    if "pyrender" not in sys.argv[1:]:     # `track_latency.py pyrender`: the two pyrender legs only
        main()
        main(faces_subdiv=6)
        main(faces_subdiv=6, f16x3=True)
    main(faces_subdiv=6, pyrender=True)                    # one library call per frame
    main(faces_subdiv=6, pyrender=True, one_call=False)    # step by step: full-frame render, two uploads, three calls, a .cpu() copy
