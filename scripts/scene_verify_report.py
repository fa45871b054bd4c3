#!/usr/bin/env python3
"""The colour verification among tracked objects (se3tn_color_stats_scene, se3tn_verify_poses_scene_host) beside the plain one
(se3tn_color_stats, se3tn_verify_poses_host): one JSON line.

  kernel alone   fit_stats_kernel<true, true> beside fit_stats_kernel<true, false> on the SAME pairs in the same process: --pairs
                 (model, observed, scene) triples, the shared cases of tests/scene_verify_scene.py repeated, records into device memory;
                 either call --reps times back to back between two HIP events, alternating which goes first within every window, per
                 call.  The scene call takes its pairs in launches of 16, the plain call in launches of 32; the third gather and the
                 25th sum are in the ratio, and so is the launch count.
  host entry     ONE call for 8 and 24 hypotheses of a sphere on a 480 x 640 frame (a wall at 900 mm with holes, the sphere before
                 it; the scene: a tracked surface 15 mm in front of the right 40 % of the sphere's pixels), the scene call beside
                 se3tn_verify_poses_host, a host clock around each (both are synchronous).

The scene records are held to the loop of tests/scene_verify_oracle.py (kernel part) and, on the frame, to the invariants of the rule
and to the plain call where nothing is hidden.  Each figure: median [min, max] of --windows timings after a warm-up round.  The process
is pinned to at most 16 CPUs before anything is timed; every timed section runs under a watchdog that ends the process if it does not
return.  Without a GPU nothing is measured.

    python scripts/scene_verify_report.py [--pairs 32] [--reps 20] [--windows 31]
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

FH, FW = 480, 640
FK = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]])
WIDTH_MM, FTOL = 170.0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=31)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a timed section may take before the process is ended")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.windows < 30:
        ap.error("--windows must be at least 30")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    os.sched_setaffinity(0, cpus)

    import ctypes as C
    import torch
    import scene_verify_oracle as VO
    import scene_verify_scene as VS
    import se3tracknet_amd as se3
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    L = se3._lib
    cases, want = VS.cases(), VS.expected()
    names = [list(cases)[i % len(cases)] for i in range(a.pairs)]
    want_fit, want_col = VO.as_arrays(se3, [want[k] for k in names])
    if not torch.cuda.is_available():
        sys.exit("scene_verify_report: no GPU -- nothing is measured without one (the loop ran: %d to %d hidden pixels per pair)"
                 % (want_fit["hidden_px"].min(), want_fit["hidden_px"].max()))
    dev = "cuda:%d" % a.device
    n = a.pairs
    eng = se3.Engine(a.device, max(n, 24))
    held = {}

    def on_device(x):
        if id(x) not in held:
            held[id(x)] = (x, torch.from_numpy(np.array(x.view(np.int16) if x.dtype == np.uint16 else x)).to(dev))
        return held[id(x)][1]

    arrs = []
    for side in range(3):
        arr = (L.Crop * n)()
        for i, k in enumerate(names):
            c = cases[k][side]
            arr[i].rgb = on_device(c["rgb"]).data_ptr() if "rgb" in c else None
            arr[i].depth = on_device(c["depth"]).data_ptr()
            arr[i].H, arr[i].W = c["depth"].shape
            arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = c["window"]
        arrs.append(arr)
    out = torch.zeros((n, 112), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp, cp = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 32 * n)
    med = lambda x: float(np.median(x))   # noqa: E731
    stat = lambda name, x, nd: {name: round(med(x), nd), name + "_min": round(min(x), nd), name + "_max": round(max(x), nd)}   # noqa: E731

    def scene_call():
        assert eng.lib.se3tn_color_stats_scene(eng._h, arrs[0], arrs[1], arrs[2], n, VS.TOL, fp, cp, st) == 0

    def plain_call():
        assert eng.lib.se3tn_color_stats(eng._h, arrs[0], arrs[1], n, VS.TOL, fp, cp, st) == 0

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

    def timed(fn):
        faulthandler.dump_traceback_later(a.timeout, exit=True)
        t0 = time.perf_counter()
        res = fn()
        dt = time.perf_counter() - t0
        faulthandler.cancel_dump_traceback_later()
        return dt * 1e3, res

    # ---- the frame of the host entry ----
    info = dict(Fx.DATASET_INFO, object_width=WIDTH_MM, camera=dict(height=FH, width=FW, focalX=FK[0, 0], focalY=FK[1, 1], centerX=FK[0, 2], centerY=FK[1, 2]))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, max_samples=24)
    mesh = Fx.icosphere(2, 0.05, 1)
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    painter = se3.HipRenderer(trk.engine, dict(mesh, kd=(1.0, 1.0, 1.0)), mode="pyrender", frame_size=(FH, FW))
    G = Fx.pose(11, (0.004, -0.003, 0.5))
    orgb, odep = painter.render_frame(G, FK)
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:FH, 0:FW]
    rgb = rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    dep = (900 + 0.2 * (xx - FW / 2) + 0.1 * (yy - FH / 2)).astype(np.uint16)
    dep[rng.random((FH, FW)) < 0.04] = 0
    on = odep > 0
    rgb[on] = np.clip(orgb[on].astype(np.int64) * 3 // 4 + 30, 0, 255).astype(np.uint8)
    dep[on] = odep[on] + rng.integers(-4, 5, int(on.sum())).astype(np.uint16)
    scene = np.zeros((FH, FW), np.uint16)
    right = on & (xx >= np.quantile(xx[on], 0.6))
    scene[right] = odep[right] - 15
    scene_d = torch.from_numpy(scene.view(np.int16)).to(dev)
    empty_d = torch.zeros_like(scene_d)

    def hypotheses(k):
        hyps = np.tile(G, (k, 1, 1))
        r = np.random.default_rng(83 + k)
        hyps[:, :3, 3] += r.uniform(-0.006, 0.006, (k, 3))
        return hyps

    def verify(k, sc):
        return trk.engine.verify_poses(trk.renderer, hypotheses(k), rgb, dep, FK, WIDTH_MM, FTOL, scene=sc)

    k_scene, k_plain = [], []
    host = {(k, which): [] for k in (8, 24) for which in ("scene", "plain")}
    for w in range(a.windows + 1):                          # the first round is the warm-up (the staging grows there)
        order = (scene_call, plain_call) if w % 2 else (plain_call, scene_call)
        ks = {fn: events(fn, a.reps) for fn in order}
        scene_call()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(-1)
        for k in (8, 24):
            dt_s, got_s = timed(lambda: verify(k, scene_d))
            dt_p, got_p = timed(lambda: verify(k, None))
            if w:
                host[(k, "scene")].append(dt_s); host[(k, "plain")].append(dt_p)
        if w:
            k_scene.append(ks[scene_call]); k_plain.append(ks[plain_call])
    equal = bool(got[:32 * n].tobytes() == want_fit.tobytes() and got[32 * n:112 * n].tobytes() == want_col.tobytes())
    fs, cs, _ = got_s
    fz, cz, _ = verify(24, empty_d)
    frame_ok = bool((fs["model_px"] == got_p[0]["model_px"]).all() and (fs["hidden_px"] > 0).all() and (cs["px"] == fs["inlier_px"]).all()
                    and (fs["seen_px"] == fs["inlier_px"] + fs["front_px"] + fs["behind_px"]).all()
                    and fz.tobytes() == got_p[0].tobytes() and cz.tobytes() == got_p[1].tobytes())
    line = {"what": "scene_verify", "lib": os.path.basename(L.LIB_PATH), "cpus": len(cpus), "pairs": n, "windows": a.windows,
            "reps_per_window": a.reps, "scene_pairs_per_launch": L.FIT_SCENE_MAX_PAIRS, "plain_pairs_per_launch": L.FIT_MAX_PAIRS, "frame": [FH, FW]}
    line.update(stat("scene_kernel_us", k_scene, 2)); line.update(stat("plain_kernel_us", k_plain, 2))
    line.update(stat("scene_over_plain", [s / p for s, p in zip(k_scene, k_plain)], 4))
    for k in (8, 24):
        line.update(stat("scene_host_entry_%d_ms" % k, host[(k, "scene")], 4)); line.update(stat("plain_host_entry_%d_ms" % k, host[(k, "plain")], 4))
    line.update(hidden_px=[int(want_fit["hidden_px"].min()), int(want_fit["hidden_px"].max())],
                frame_hidden_px=[int(fs["hidden_px"].min()), int(fs["hidden_px"].max())], frame_px=[int(cs["px"].min()), int(cs["px"].max())],
                equal=equal, frame_ok=frame_ok)
    print(json.dumps(line), flush=True)
    eng.close()
    if not (equal and frame_ok):
        sys.exit("scene_verify_report: a device result differs from its oracle")


if __name__ == "__main__":
    main()
