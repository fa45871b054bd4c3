"""GPU: ADD / ADD-S of n pose pairs in one device call (se3tn_pose_errors, Engine.pose_errors, metrics.pose_errors(engine=...),
Tracker.pose_errors, the device_metrics / engine switches of the sequence evaluators).

The yardstick is the CPU `metrics.add` / `metrics.adi` (KD-tree, pinned to the reference by tests/golden/eval_reference.npz), never
the code under test.  Tolerance 1e-12 m absolute on both values, derived: the tests keep coordinates <= 4 m, errors <= 1 m and
P <= 4,096; under those bounds the worst case of a sequential float64 sum of P terms <= 1 is 4096 * 2^-53 * 1 = 4.5e-13, and the
transform and distance roundings add about 1.3e-14 (a float64 brute force in another operation order lies within 1.1e-14 of the
KD-tree evaluators over these shapes).

Point counts sit where the tiling can go wrong.  The kernel's query tile is 1,024 points per workgroup (256 threads x 4 points in
registers: thread t holds points t, t + 256, t + 512, t + 768 of the tile), not 256, and its LDS reference tile is 1,024 points, so
the edges are: one wave (63, 64, 65), the first to the second register slot of a thread (255, 256, 257), one query tile = one
reference tile (1,023, 1,024, 1,025), several tiles with a ragged last one (2,620: a YCB model), and 4,096, the upper bound of the
tolerance argument."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from oracle import eval_fixtures as EF
from oracle import fixtures as Fx
from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
TOL = 1e-12
P_CASES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2620, 4096]
DISPLACEMENTS = [1e-6, 5e-3, 0.3, 1.0]
RADIUS = 0.1          # the model clouds lie inside a ball of this radius (metres)
H, W = Fx.SOUP_FRAME_HW
K = Fx.SOUP_FRAME_K
INFO = dict(Fx.DATASET_INFO, object_width=150.0,
            camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, 1)
    yield e
    e.close()


def cloud(P):
    """P points inside the ball of radius RADIUS; from 4 points on the last quarter repeats the first (ties in the minimum)."""
    rng = np.random.default_rng(1000 + P)
    v = rng.normal(size=(P, 3))
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * RADIUS * rng.uniform(0.2, 1.0, (P, 1))
    if P >= 4:
        pts[-(P // 4):] = pts[:P // 4]
    return pts


def rigid(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix()
    T[:3, 3] = t
    return T


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def pair(rng, d):
    """gt: any orientation (rotation angle up to 3 rad), 0.5 - 2.5 m in front of the camera.  pred = gt o delta with delta in the
    object frame: a translation of 0.7 d and a rotation of min(3, 0.25 d / RADIUS) rad, so no model point moves by more than
    0.95 d (<= 0.9 m at d = 1)."""
    gt = rigid(unit(rng) * rng.uniform(0.5, 3.0), [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.5, 2.5)])
    delta = rigid(unit(rng) * min(3.0, 0.25 * d / RADIUS), unit(rng) * 0.7 * d)
    return gt @ delta, gt


def cpu(metrics, preds, gts, pts):
    """the loop over metrics.add / metrics.adi; one query thread (the values do not depend on it, the many-core start-up cost does)"""
    return metrics.pose_errors(preds, gts, pts, workers=1)


# ---- against the CPU evaluators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_CASES)
def test_every_tiling_edge_against_the_cpu_evaluators(se3, eng, P):
    pts = cloud(P)
    rng = np.random.default_rng(P)
    pairs = [pair(rng, d) for d in DISPLACEMENTS]
    preds, gts = np.array([p for p, _ in pairs]), np.array([g for _, g in pairs])
    want_add, want_adds = cpu(se3.metrics, preds, gts, pts)
    # the bounds the tolerance was derived under
    assert max(np.abs(pts @ T[:3, :3].T + T[:3, 3]).max() for T in list(preds) + list(gts)) <= 4.0
    assert want_add.max() <= 1.0 and want_adds.max() <= 1.0
    mp = eng.model_points(pts)
    assert len(mp) == P and eng.lib.se3tn_points_count(mp._h) == P
    add, adds = eng.pose_errors(mp, preds, gts)
    print("P = %d: max |d add| = %.3e, max |d adds| = %.3e" % (P, np.abs(add - want_add).max(), np.abs(adds - want_adds).max()))
    assert add.dtype == adds.dtype == np.float64 and add.shape == adds.shape == (4,)
    assert np.abs(add - want_add).max() <= TOL and np.abs(adds - want_adds).max() <= TOL
    # adds = False: the all-pairs loop is skipped, add has the same bits
    add_only, none = eng.pose_errors(mp, preds, gts, adds=False)
    assert none is None and np.array_equal(add_only, add)
    # metrics.pose_errors with an engine: from a point array, a PointCloud and the handle -- one device call, the same bits
    for model in (pts, se3.utils.PointCloud(pts), mp):
        a2, s2 = se3.metrics.pose_errors(preds, gts, model, engine=eng)
        assert np.array_equal(a2, add) and np.array_equal(s2, adds)
    # guarantee (a): equal poses give exactly 0.0 twice, also far from the origin
    same = np.array([gts[0], rigid(unit(rng) * 2.9, [31.7, -18.3, 57.1]), rigid([0, 0, 0], [0, 0, 0])])
    z_add, z_adds = eng.pose_errors(mp, same, same.copy())
    assert np.array_equal(z_add, np.zeros(3)) and np.array_equal(z_adds, np.zeros(3))
    assert not np.signbit(z_add).any() and not np.signbit(z_adds).any()
    mp.close()


# ---- guarantee (b): a pair's bits do not depend on the call ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(se3):
    """chunk + 1 pairs on a model of two query tiles and two reference tiles with ragged ends, and their CPU values"""
    chunk = se3._lib.POSE_ERRORS_CHUNK
    pts = cloud(1300)
    rng = np.random.default_rng(99)
    pairs = [pair(rng, DISPLACEMENTS[i % 4]) for i in range(chunk + 1)]
    preds, gts = np.array([p for p, _ in pairs]), np.array([g for _, g in pairs])
    return dict(chunk=chunk, pts=pts, preds=preds, gts=gts, want=cpu(se3.metrics, preds, gts, pts))


def test_a_pair_has_the_same_bits_alone_in_any_call_at_any_position_and_on_every_run(se3, eng, many):
    chunk, preds, gts = many["chunk"], many["preds"], many["gts"]
    mp = eng.model_points(many["pts"])
    full = eng.pose_errors(mp, preds, gts)                       # chunk + 1 pairs: two launches, the last pair alone in the second
    print("n = %d: max |d add| = %.3e, max |d adds| = %.3e" % (chunk + 1, np.abs(full[0] - many["want"][0]).max(),
                                                               np.abs(full[1] - many["want"][1]).max()))
    assert np.abs(full[0] - many["want"][0]).max() <= TOL and np.abs(full[1] - many["want"][1]).max() <= TOL
    k = 3
    alone = eng.pose_errors(mp, preds[k:k + 1], gts[k:k + 1])
    assert alone[0][0] == full[0][k] and alone[1][0] == full[1][k]
    for n in (1, 2, 7, chunk, chunk + 1):
        others = [i for i in range(chunk + 1) if i != k][:n - 1]
        for pos in sorted({0, n // 2, n - 1}):                   # first, middle, last (the last of chunk + 1 is the second launch)
            order = others[:pos] + [k] + others[pos:]
            got = eng.pose_errors(mp, preds[order], gts[order])
            again = eng.pose_errors(mp, preds[order], gts[order])
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), (n, pos)      # run twice
            assert got[0][pos] == alone[0][0] and got[1][pos] == alone[1][0], (n, pos)                  # the pair alone
            assert np.array_equal(got[0], full[0][order]) and np.array_equal(got[1], full[1][order]), (n, pos)   # every pair of the call
    mp.close()


# ---- the device-pointer entry point ------------------------------------------------------------------------------------------------------
def enqueue(eng, mp, n, pred_d, gt_d, add_d, adds_d):
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
    return eng.lib.se3tn_pose_errors(eng._h, mp._h, n, p(pred_d), p(gt_d), p(add_d), p(adds_d),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_device_pointers_give_the_host_variants_bits_also_from_a_replayed_graph(se3, eng, many):
    chunk = many["chunk"]
    n = chunk + 1
    mp = eng.model_points(many["pts"])
    want = eng.pose_errors(mp, many["preds"], many["gts"])
    pred_d = torch.from_numpy(many["preds"].reshape(n, 16)).cuda()
    gt_d = torch.from_numpy(many["gts"].reshape(n, 16)).cuda()
    add_t, adds_t = eng.pose_errors(mp, pred_d, gt_d)                                     # tensors in, tensors out
    assert add_t.is_cuda and add_t.dtype == torch.float64 and tuple(add_t.shape) == (n,)
    assert np.array_equal(add_t.cpu().numpy(), want[0]) and np.array_equal(adds_t.cpu().numpy(), want[1])
    add_only, none = eng.pose_errors(mp, pred_d, gt_d, adds=False)
    assert none is None and np.array_equal(add_only.cpu().numpy(), want[0])
    # capture on a side stream, replay, change the CONTENTS of the pose buffers, replay
    add_d = torch.zeros(n, dtype=torch.float64, device="cuda")
    adds_d = torch.zeros(n, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert enqueue(eng, mp, n, pred_d, gt_d, add_d, adds_d) == 0                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert enqueue(eng, mp, n, pred_d, gt_d, add_d, adds_d) == 0
    for turn in range(3):
        order = np.roll(np.arange(n), 5 * turn)                                           # other poses in the same buffers
        pred_d.copy_(torch.from_numpy(many["preds"][order].reshape(n, 16)))
        gt_d.copy_(torch.from_numpy(many["gts"][order].reshape(n, 16)))
        add_d.zero_(); adds_d.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(add_d.cpu().numpy(), want[0][order]) and np.array_equal(adds_d.cpu().numpy(), want[1][order]), turn
    # an eager host call after the replays
    again = eng.pose_errors(mp, many["preds"], many["gts"])
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    mp.close()


# ---- Tracker.pose_errors and the refusals ----------------------------------------------------------------------------------------------
def write_ply(path, verts):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\nend_header\n" % len(verts))
        for v in verts:
            f.write("%.17g %.17g %.17g\n" % tuple(v))


@pytest.fixture(scope="module")
def tracker(se3, tmp_path_factory):
    """A Tracker whose model file is a small .ply (its object_cloud) and whose renderer is the built-in rasteriser on the same mesh"""
    mesh = Fx.icosphere(2, 0.05, 1)
    ply = str(tmp_path_factory.mktemp("pose_errors") / "sphere.ply")
    write_ply(ply, np.asarray(mesh["vertices"], np.float64))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(INFO, mean, std, {"state_dict": O.make_state_dict(0)}, model_path=ply, max_samples=1)
    assert trk.renderer is None and trk.object_cloud is not None and len(trk.object_cloud.points) > 20
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    return trk


def test_tracker_scores_against_its_object_cloud(se3, tracker):
    rng = np.random.default_rng(5)
    pairs = [pair(rng, d) for d in DISPLACEMENTS + [0.02, 0.05, 0.1]]
    preds, gts = np.array([p for p, _ in pairs]), np.array([g for _, g in pairs])
    add, adds = tracker.pose_errors(preds, gts)
    want = cpu(se3.metrics, preds, gts, tracker.object_cloud)
    assert np.abs(add - want[0]).max() <= TOL and np.abs(adds - want[1]).max() <= TOL
    handle = tracker._model_points
    assert handle is not None and len(handle) == len(tracker.object_cloud.points)
    again = tracker.pose_errors(preds, gts)
    assert tracker._model_points is handle                                                # uploaded once
    assert np.array_equal(again[0], add) and np.array_equal(again[1], adds)


def test_refusals_leave_the_engine_tracking_and_scoring(se3, tracker):
    eng, lib, L = tracker.engine, tracker.engine.lib, se3._lib
    rgb, depth = Fx.synthetic_frame(3, H, W)
    prev = Fx.pose(11, (0.004, -0.003, 0.5))
    rng = np.random.default_rng(6)
    pairs = [pair(rng, d) for d in DISPLACEMENTS]
    preds, gts = np.array([p for p, _ in pairs]), np.array([g for _, g in pairs])
    pose0 = tracker.on_track(prev, rgb, depth)
    score0 = tracker.pose_errors(preds, gts)
    mp = tracker._model_points

    def still_right(what):
        assert np.array_equal(tracker.on_track(prev, rgb, depth), pose0), what
        got = tracker.pose_errors(preds, gts)
        assert np.array_equal(got[0], score0[0]) and np.array_equal(got[1], score0[1]), what

    p16, g16 = np.ascontiguousarray(preds.reshape(-1, 16)), np.ascontiguousarray(gts.reshape(-1, 16))
    out = np.zeros(8)
    hp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    pred_d, gt_d = torch.from_numpy(p16).cuda(), torch.from_numpy(g16).cuda()
    out_d = torch.zeros(8, dtype=torch.float64, device="cuda")
    dp = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
    for n in (0, -3):
        assert lib.se3tn_pose_errors_host(eng._h, mp._h, n, hp(p16), hp(g16), hp(out), hp(out[4:]), None) == E_ARG
        assert lib.se3tn_pose_errors(eng._h, mp._h, n, dp(pred_d), dp(gt_d), dp(out_d), dp(out_d[4:]), None) == E_ARG
    still_right("after n < 1")
    assert lib.se3tn_pose_errors_host(eng._h, mp._h, 4, None, hp(g16), hp(out), hp(out[4:]), None) == E_ARG
    assert lib.se3tn_pose_errors_host(eng._h, mp._h, 4, hp(p16), None, hp(out), hp(out[4:]), None) == E_ARG
    assert lib.se3tn_pose_errors(eng._h, mp._h, 4, None, dp(gt_d), dp(out_d), dp(out_d[4:]), None) == E_ARG
    assert lib.se3tn_pose_errors(eng._h, mp._h, 4, dp(pred_d), dp(gt_d), None, None, None) == E_ARG      # nothing asked for
    assert lib.se3tn_pose_errors(eng._h, None, 4, dp(pred_d), dp(gt_d), dp(out_d), dp(out_d[4:]), None) == E_ARG
    still_right("after NULL pointers")
    for bad in (np.nan, np.inf):
        broken = preds.copy()
        broken[2, 1, 3] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*pose 2" % E_ARG):
            eng.pose_errors(mp, broken, gts)
        with pytest.raises(L.Se3tnError, match="rc=%d" % E_ARG):
            eng.pose_errors(mp, preds, broken)
    still_right("after a pose that is not finite")
    # row 3 of a pose is not read
    odd = preds.copy()
    odd[:, 3, :] = [7.0, -2.0, 0.5, 3.0]
    got = eng.pose_errors(mp, odd, gts)
    assert np.array_equal(got[0], score0[0]) and np.array_equal(got[1], score0[1])
    # model sizes: P = 0, a coordinate that is not finite, and P > 2^20 by argument only (three doubles stand behind the pointer)
    h = C.c_void_p()
    few = np.zeros(3)
    assert lib.se3tn_points_create(eng._h, hp(few), 0, C.byref(h)) == E_ARG and not h.value
    assert lib.se3tn_points_create(eng._h, hp(few), L.POSE_ERRORS_MAX_POINTS + 1, C.byref(h)) == E_ARG and not h.value
    assert b"SE3TN_POSE_ERRORS_MAX_POINTS" in lib.se3tn_last_error()
    with pytest.raises(L.Se3tnError, match="not finite"):
        eng.model_points(np.array([[0.0, 1.0, np.nan]]))
    still_right("after the refused models")
    # the host variant waits for its stream: inside a capture it says so and leaves the capture whole
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(L.Se3tnError, match="rc=%d" % E_STATE):
            eng.pose_errors(mp, preds, gts)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    still_right("after the refused capture")


# ---- the evaluators ---------------------------------------------------------------------------------------------------------------------
CLASS_ID = 2


def clear_of_the_cap(*errs):
    """VOCap x 100 moves by at most 100 d / 0.1 for an error shift d -- while no error crosses the 0.1 m cap"""
    e = np.concatenate([np.asarray(x, np.float64).ravel() for x in errs])
    return np.abs(e - 0.1).min() > 1e-9


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) > 0
    for name in names:
        with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
            assert fa.read() == fb.read(), name


def test_predict_sequence_ycb_scores_on_the_device(se3, tracker, tmp_path):
    ycb = EF.make_ycb_tree(str(tmp_path), CLASS_ID)
    seq_dir = os.path.join(ycb, "data_organized", "0048")
    runs = {}
    for name, dm in (("cpu", False), ("dev", True)):
        tracker.on_track = EF.StubTracker(5).on_track     # the fixture's seeded motion on the fixture's 12 x 16 frames
        try:
            runs[name] = se3.sequence.predict_sequence_ycb(tracker, seq_dir, CLASS_ID, str(tmp_path / name), device_metrics=dm)
        finally:
            del tracker.on_track
    c, d = runs["cpu"], runs["dev"]
    assert clear_of_the_cap(c["add_errs"], c["adi_errs"])
    assert np.array_equal(c["poses"], d["poses"]) and len(c["add_errs"]) == 40
    assert np.abs(c["add_errs"] - d["add_errs"]).max() <= TOL and np.abs(c["adi_errs"] - d["adi_errs"]).max() <= TOL
    assert abs(c["add_auc"] - d["add_auc"]) <= 1e-9 and abs(c["adi_auc"] - d["adi_auc"]) <= 1e-9
    assert 0.0 < c["adi_auc"] < 100.0
    same_files(str(tmp_path / "cpu"), str(tmp_path / "dev"))


def test_eval_one_class_and_eval_ycbineoat_score_on_the_device(se3, eng, tmp_path):
    seq = se3.sequence
    ycb = EF.make_ycb_tree(str(tmp_path), CLASS_ID)
    res = str(tmp_path / "res_ycb")
    EF.make_ycb_results(seq, ycb, res, CLASS_ID)
    c = seq.eval_one_class(res, ycb, CLASS_ID)
    d = seq.eval_one_class(res, ycb, CLASS_ID, engine=eng)
    assert clear_of_the_cap(c["add_errs"], c["adi_errs"]) and c["n"] == d["n"] > 10
    assert np.abs(c["add_errs"] - d["add_errs"]).max() <= TOL and np.abs(c["adi_errs"] - d["adi_errs"]).max() <= TOL
    assert abs(c["add_auc"] - d["add_auc"]) <= 1e-9 and abs(c["adi_auc"] - d["adi_auc"]) <= 1e-9
    # YCBInEOAT: one call per model, the same per-object and overall numbers
    data = EF.make_eoat_tree(str(tmp_path))
    res_e = str(tmp_path / "res_eoat")
    EF.make_eoat_results(seq, data, res_e)
    # the cap condition on the CPU errors of every frame of every video
    models = {}
    for name in EF.YCB_CLASSES:
        for obj in seq.YCBINEOAT_OBJECTS:
            if obj in name:
                models[obj] = np.loadtxt(os.path.join(ycb, "CADmodels", name, "points.xyz")).reshape(-1, 3)
    for video, _ in EF.EOAT_VIDEOS:
        obj = next(o for o in seq.YCBINEOAT_OBJECTS if o in video)
        preds = [np.loadtxt(os.path.join(res_e, video, f)) for f in sorted(os.listdir(os.path.join(res_e, video)))]
        gts = [np.loadtxt(os.path.join(data, video, "annotated_poses", f))
               for f in sorted(os.listdir(os.path.join(data, video, "annotated_poses")))]
        assert clear_of_the_cap(*cpu(se3.metrics, preds, gts, models[obj]))
    ce = seq.eval_ycbineoat(res_e, data, ycb)
    de = seq.eval_ycbineoat(res_e, data, ycb, engine=eng)
    assert ce["n"] == de["n"] == sum(n for _, n in EF.EOAT_VIDEOS) and sorted(ce["per_object"]) == sorted(de["per_object"])
    assert abs(ce["add_auc"] - de["add_auc"]) <= 1e-9 and abs(ce["adi_auc"] - de["adi_auc"]) <= 1e-9
    for obj in ce["per_object"]:
        for key in ("add_auc", "adi_auc"):
            assert abs(ce["per_object"][obj][key] - de["per_object"][obj][key]) <= 1e-9, (obj, key)
        assert ce["per_object"][obj]["n"] == de["per_object"][obj]["n"]
