#!/usr/bin/env python3
"""The pose alignment among tracked objects (se3tn_align_poses_scene) beside the plain one (se3tn_align_poses): one JSON line.

Data (that of scripts/pose_align_report.py): a model of --points points on an ellipsoid with its analytic normals, a 480 x 640 depth
frame holding the model splatted at its true pose before a wall at 900 mm with holes; --poses hypotheses (seeded perturbations of the
true pose of up to 8 degrees and 8 mm per axis), --iters iterations each, stop 0 so that every pose runs them all.  The composed scene:
a tracked surface 15 mm in front of the model's over the right 40 % of the model's pixels (those points are hidden), and a second one
60 mm behind it under the lower quarter (read, but hiding nothing) -- so both outcomes of the verdict are in the walk.

  kernel alone   the scene-aware call and the plain call, --reps times back to back between two HIP events each, alternating within
                 every window, per call;
  device entry   either call on device pointers, a host clock around the call and a stream synchronise;
  host entry     se3tn_align_poses_scene_host from host arrays (one upload, one launch, one read-back, synchronous), and the same
                 work step by step: upload of poses, frame and scene, the device entry, read-back of poses, records and sums.

Both device results are held to their oracles, bytes.  Each figure: median [min, max] of --windows timings after a warm-up round.  The
process is pinned to at most 16 CPUs before anything is timed.  Every timed section runs under a watchdog that ends the process if it
does not return.  Without a GPU nothing is measured.

    python scripts/scene_align_report.py [--points 2620] [--poses 8] [--iters 20] [--reps 20] [--windows 31]
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
SCENE_TOL = 10


def composed_scene(depth, wall_from=880):
    """the scene frame: over the model's pixels (everything nearer than the wall), 15 mm in front of the observed surface on the
    right 40 % of their columns, 60 mm behind it on the lowest quarter of their rows elsewhere, 0 everywhere else"""
    on = (depth > 100) & (depth < wall_from)
    rows, cols = np.nonzero(on)
    scene = np.zeros_like(depth)
    right = on & (np.arange(depth.shape[1])[None, :] >= np.quantile(cols, 0.6))
    low = on & ~right & (np.arange(depth.shape[0])[:, None] >= np.quantile(rows, 0.75))
    scene[right] = depth[right] - 15
    scene[low] = depth[low] + 60
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2620)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
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
    from scipy.spatial.transform import Rotation
    import pose_align_oracle as PAO
    import scene_align_oracle as SAO
    import se3tracknet_amd as se3
    from pose_search_report import H, W, K, scene as make_scene
    L = se3._lib
    pts, depth, true, _ = make_scene(a.points, 7 + a.points)
    nrm = pts / RADII ** 2
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]             # unit normals (see scripts/pose_align_report.py)
    scene = composed_scene(depth)
    rng = np.random.default_rng(83)
    hyps = np.tile(true, (a.poses, 1, 1))
    for T in hyps:
        T[:3, :3] = Rotation.from_rotvec(np.deg2rad(rng.uniform(-8, 8, 3))).as_matrix() @ T[:3, :3]
        T[:3, 3] += rng.uniform(-0.008, 0.008, 3)
    n = a.poses
    prm = dict(gate_mm=20, iters=a.iters, min_pairs=12, damping=1e-6, stop=0.0)
    want_scene = SAO.align(pts, nrm, hyps, depth, scene, K, SCENE_TOL, **prm)
    want_plain = PAO.align(pts, nrm, hyps, depth, K, **prm)
    if not torch.cuda.is_available():
        sys.exit("scene_align_report: no GPU -- nothing is measured without one (the oracles ran: %d to %d hidden points per pose)"
                 % (want_scene[1]["hidden_pts"].min(), want_scene[1]["hidden_pts"].max()))
    eng = se3.Engine(a.device, 1)
    mp = eng.model_points(pts, nrm)
    dev = "cuda:%d" % a.device
    depth_d = torch.from_numpy(depth.view(np.int16)).to(dev)
    scene_d = torch.from_numpy(scene.view(np.int16)).to(dev)
    hyps16 = np.ascontiguousarray(hyps.reshape(n, 16))
    poses_d = torch.from_numpy(hyps16).to(dev)
    out_d = torch.zeros((n, 16), dtype=torch.float64, device=dev)
    rec_d = torch.zeros((n, 40), dtype=torch.uint8, device=dev)
    sums_d = torch.zeros((n, 28), dtype=torch.int64, device=dev)
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    cp = L.AlignParams(prm["gate_mm"], prm["iters"], prm["min_pairs"], 0, prm["damping"], prm["stop"])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
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

    def scene_call():
        assert eng.lib.se3tn_align_poses_scene(eng._h, mp._h, n, vp(poses_d), vp(depth_d), vp(scene_d), H, W, Kp, C.byref(cp), SCENE_TOL,
                                               vp(out_d), vp(rec_d), vp(sums_d), st) == 0

    def plain_call():
        assert eng.lib.se3tn_align_poses(eng._h, mp._h, n, vp(poses_d), vp(depth_d), H, W, Kp, C.byref(cp), vp(out_d), vp(rec_d), vp(sums_d), st) == 0

    def synced(fn):
        fn()
        torch.cuda.synchronize()

    def stepwise():
        """what the host entry does in one call, step by step through torch: three uploads, the device entry, three read-backs"""
        p, d, s = torch.from_numpy(hyps16).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(scene.view(np.int16)).to(dev)
        out, rec, sums = eng.align_poses(mp, p, d, K, sums=True, scene=s, scene_tol_mm=SCENE_TOL, **prm)
        return out.cpu().numpy(), rec.cpu().numpy().view(L.SCENE_ALIGN_REC_DTYPE).reshape(n), sums.cpu().numpy()

    def result():
        torch.cuda.synchronize()
        return out_d.cpu().numpy().reshape(n, 4, 4).copy(), rec_d.cpu().numpy().copy(), sums_d.cpu().numpy().copy()

    k_scene, k_plain, d_scene, d_plain, h_one, h_steps = [], [], [], [], [], []
    for w in range(a.windows + 1):                          # the first round is the warm-up (the staging grows there)
        order = (scene_call, plain_call) if w % 2 else (plain_call, scene_call)      # alternating which one goes first
        ks = {fn: events(fn, a.reps) for fn in order}
        dt_s, _ = timed(lambda: synced(scene_call))
        got_scene = result()
        dt_p, _ = timed(lambda: synced(plain_call))
        got_plain = result()
        dt_h, got_host = timed(lambda: eng.align_poses(mp, hyps, depth, K, sums=True, scene=scene, scene_tol_mm=SCENE_TOL, **prm))
        dt_w, got_steps = timed(stepwise)
        if w:
            k_scene.append(ks[scene_call]); k_plain.append(ks[plain_call]); d_scene.append(dt_s); d_plain.append(dt_p)
            h_one.append(dt_h); h_steps.append(dt_w)
    same = lambda got, want: all(np.asarray(g).tobytes() == w_.tobytes() for g, w_ in zip(got, want))   # noqa: E731
    equal = bool(same(got_scene, want_scene) and same(got_plain, want_plain) and same(got_host, want_scene) and same(got_steps, want_scene))
    rec = want_scene[1]
    errs = np.array([PAO.pose_error(o, true) for o in want_scene[0]])
    line = {"what": "scene_align", "lib": os.path.basename(L.LIB_PATH), "cpus": len(cpus), "n": n, "P": a.points, "frame": [H, W],
            "iters": a.iters, "stop": 0.0, "gate_mm": 20, "scene_tol_mm": SCENE_TOL, "windows": a.windows, "reps_per_window": a.reps}
    line.update(stat("scene_kernel_us", k_scene, 2)); line.update(stat("plain_kernel_us", k_plain, 2))
    line.update(stat("scene_over_plain", [s / p for s, p in zip(k_scene, k_plain)], 4))
    line.update(stat("scene_device_entry_ms", d_scene, 4)); line.update(stat("plain_device_entry_ms", d_plain, 4))
    line.update(stat("host_entry_ms", h_one, 4)); line.update(stat("stepwise_ms", h_steps, 4))
    line.update(hidden_pts=[int(rec["hidden_pts"].min()), int(rec["hidden_pts"].max())],
                pairs_last=[int(rec["pairs"].min()), int(rec["pairs"].max())], facing=[int(rec["facing_pts"].min()), int(rec["facing_pts"].max())],
                scene_pixels=int((scene > 0).sum()), worst_mm_from_truth=round(float(1000 * errs[:, 0].max()), 3), equal=equal)
    print(json.dumps(line), flush=True)
    mp.close()
    eng.close()
    if not equal:
        sys.exit("scene_align_report: a device result differs from its oracle")


if __name__ == "__main__":
    main()
