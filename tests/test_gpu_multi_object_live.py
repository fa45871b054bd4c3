"""GPU: se3tn_on_track_objects_live / MultiTracker.on_track_live / LiveMultiTracker -- predict_ros.py:38-60 for several objects of one
live camera frame in ONE library call -- against the two compositions the library already had: MultiTracker.on_track on
engine.fill_depth's output with the colours already swapped, and every object's own Tracker.on_track_live.  The same kernels see the
same bytes, so pose, (trans, rot), bbox and image A (rgb and depth) are compared BIT FOR BIT.

Trackers as in tests/test_gpu_multi_object.py: the two trained stand-ins plus a random-init model, ellipsoid / icosphere meshes.
Frames: 480 x 640 i.i.d. frames with holes (Fx.synthetic_frame).  Without the feature every case fails: the methods are missing."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import closed_loop as CL
from oracle import fixtures as Fx
from oracle import free_run as FR
from oracle import se3_oracle as O
from oracle import synth_track as ST

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
H, W = 480, 640
KEYS = ("pose", "trans", "rot", "bbox", "rgbA", "depthA")


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def models():
    """name -> (state_dict, mean, std, trans_normalizer, rot_normalizer)"""
    out = {}
    for name, regime in (("30deg", "ycbineoat_30deg"), ("5deg", "ycb_video_5deg")):
        sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights(regime))
        out[name] = (sd, mean, std) + tuple(CL.REGIMES[regime])
    mean, std = Fx.mean_std(3)
    out["random"] = (O.make_state_dict(5, head_gain=CL.HEAD_GAIN), mean, std, 0.05, 12 * np.pi / 180)
    return out


MESHES = {"ellipsoid": ST.make_object(4), "sphere": Fx.icosphere(3, 0.05, 1)}


def make_tracker(se3, models, model, mesh, width):
    sd, mean, std, tn, rn = models[model]
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=width), mean, std, {"state_dict": sd}, trans_normalizer=tn,
                      rot_normalizer=rn, max_samples=1)
    trk.renderer = se3.HipRenderer(trk.engine, MESHES[mesh])
    assert trk.one_call and not trk.renderer.full_frame
    trk.spec = (model, mesh, width)          # (test bookkeeping)
    return trk


@pytest.fixture(scope="module")
def trackers(se3, models):
    specs = [("30deg", "ellipsoid", 150.0), ("5deg", "sphere", 120.0), ("random", "ellipsoid", 140.0), ("5deg", "ellipsoid", 150.0),
             ("30deg", "sphere", 110.0), ("random", "sphere", 130.0)]
    return [make_tracker(se3, models, *s) for s in specs]


@pytest.fixture(scope="module")
def trackers150(se3, models):
    """150 mm wide (the width the window cases of tests/test_gpu_live_one_call.py were made for), one model each + one repeated"""
    return [make_tracker(se3, models, m, mesh, 150.0) for m, mesh in (("30deg", "ellipsoid"), ("5deg", "sphere"), ("random", "ellipsoid"),
                                                                       ("5deg", "ellipsoid"))]


@pytest.fixture(scope="module")
def frames():
    out = [Fx.synthetic_frame(220 + i) for i in range(3)]
    for rgb, depth in out:
        assert rgb.shape == (H, W, 3) and (depth == 0).mean() > 0.03      # 480 x 640 with holes
    return out


def poses_inside(n, seed=0):
    return [Fx.pose(50 + 7 * seed + i, (0.09 * np.cos(1.3 * i + seed), 0.06 * np.sin(0.9 * i + seed), 0.7 + 0.04 * (i % 7))) for i in range(n)]


def window_kind(se3, P, width=150.0):
    l, t, r, b = se3.crop_window(se3.compute_bbox(P, Fx.K_YCB, width))
    if r <= 0 or b <= 0 or l >= W or t >= H:
        return "miss"
    return ("L" if l < 0 else "") + ("T" if t < 0 else "") + ("R" if r > W else "") + ("B" if b > H else "") or "inside"


def bgr_of(rgb):
    return np.ascontiguousarray(rgb[:, :, ::-1])


def records(mt, out):
    lp = mt.last_prediction
    return [dict(pose=out[i].copy(), trans=lp["trans"][i].copy(), rot=lp["rot"][i].copy(), bbox=np.asarray(lp["bbox"][i]).copy(),
                 rgbA=lp["rgbA"][i].cpu().numpy().copy(), depthA=lp["depthA"][i].cpu().numpy().view(np.uint16).copy()) for i in range(mt.n)]


def multi_live(mt, poses, color, raw, bgr, blur, **kw):
    return records(mt, mt.on_track_live(np.stack(poses), color, raw, bgr=bgr, max_depth=2.0, extrapolate=False, blur_type=blur, **kw))


def multi_composed(mt, poses, rgb, raw, blur):
    """what the library offered before: the filled frame through the host, the colours swapped there, MultiTracker.on_track"""
    return records(mt, mt.on_track(np.stack(poses), rgb, mt.engine.fill_depth(raw, 2.0, False, blur)))


def single_live(t, P, color, raw, bgr, blur):
    pose = t.on_track_live(P, color, raw, bgr=bgr, max_depth=2.0, extrapolate=False, blur_type=blur)
    lp = t.last_prediction
    return dict(pose=pose.copy(), trans=lp["trans"].reshape(3).copy(), rot=lp["rot"].reshape(3).copy(), bbox=np.asarray(lp["bbox"]).reshape(4, 2).copy(),
                rgbA=t.renderer.rgb.cpu().numpy().copy(), depthA=t.renderer.depth.cpu().numpy().view(np.uint16).copy())


def assert_same(got, want, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def assert_all_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, (what, i))


@pytest.mark.parametrize("blur", ["bilateral", None], ids=["bilateral", "None"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])
def test_object_counts(se3, trackers, frames, n, blur):
    """n = 6 makes two network chunks (5 + 1)"""
    rgb, raw = frames[n % 3]
    poses = poses_inside(n, seed=n)
    trks = trackers[:n]
    for P, t in zip(poses, trks):
        assert window_kind(se3, P, t.object_width) == "inside"
    mt = se3.MultiTracker(trks)
    got = multi_live(mt, poses, bgr_of(rgb), raw, True, blur)
    assert_all_same(got, multi_composed(mt, poses, rgb, raw, blur), ("composition", n, blur))
    for i, t in enumerate(trks):
        assert_same(got[i], single_live(t, poses[i], bgr_of(rgb), raw, True, blur), ("single", n, blur, i, t.spec))
        assert (got[i]["depthA"] > 0).sum() > 300                # an empty render cannot pass
    mt.close()


def test_equal_models_differ_in_outputs_and_both_channel_orders(se3, trackers, frames):
    rgb, raw = frames[0]
    trks = [trackers[0], trackers[1], trackers[0]]                # objects 0 and 2 share model, mesh and width
    poses = poses_inside(3, seed=9)
    mt = se3.MultiTracker(trks)
    want = multi_composed(mt, poses, rgb, raw, "bilateral")
    assert not np.array_equal(want[0]["trans"], want[2]["trans"])   # ... and still come out differently: the comparison is not vacuous
    assert_all_same(multi_live(mt, poses, rgb, raw, False, "bilateral"), want, "rgb")
    assert_all_same(multi_live(mt, poses, bgr_of(rgb), raw, True, "bilateral"), want, "bgr")
    # the channel order matters: the BGR frame taken for RGB gives other bits
    wrong = multi_live(mt, poses, bgr_of(rgb), raw, False, "bilateral")
    assert not np.array_equal(wrong[0]["trans"], want[0]["trans"])
    mt.close()


LEAVING = [("inside", 3, (0.02, -0.01, 0.8)), ("LT", 5, (-0.2, -0.17, 0.75)), ("RB", 5, (0.2, 0.14, 0.7)), ("miss", 5, (0.6, 0.5, 0.9))]


def test_windows_leaving_the_frame(se3, trackers150, frames):
    """the poses of tests/test_gpu_live_one_call.py::test_windows_leaving_the_frame (and its inside pose) in ONE call"""
    poses = [Fx.pose(seed, t) for _, seed, t in LEAVING]
    for (kind, _, _), P in zip(LEAVING, poses):
        assert window_kind(se3, P) == kind
    mt = se3.MultiTracker(trackers150)
    filled_dev = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    rgb, raw = frames[1]
    for blur in ("bilateral", "gaussian", None):
        want = multi_composed(mt, poses, rgb, raw, blur)
        assert_all_same(multi_live(mt, poses, bgr_of(rgb), raw, True, blur), want, (blur, "no depth_filled"))
        filled_dev.zero_()
        assert_all_same(multi_live(mt, poses, bgr_of(rgb), raw, True, blur, depth_filled=filled_dev), want, (blur, "depth_filled"))
        assert np.array_equal(filled_dev.cpu().numpy().view(np.uint16), mt.engine.fill_depth(raw, 2.0, False, blur)), blur
    got = multi_live(mt, poses, bgr_of(rgb), raw, True, "bilateral")
    for i, t in enumerate(trackers150):                           # ... and every object as alone
        assert_same(got[i], single_live(t, poses[i], bgr_of(rgb), raw, True, "bilateral"), ("single", LEAVING[i][0]))
    # every window off the frame: no rectangle, no fill -- the call returns and equals the composition
    miss = [Fx.pose(5 + i, (0.6 + 0.02 * i, 0.5, 0.9)) for i in range(4)]
    for P in miss:
        assert window_kind(se3, P) == "miss"
    want = multi_composed(mt, miss, rgb, raw, "bilateral")
    assert_all_same(multi_live(mt, miss, bgr_of(rgb), raw, True, "bilateral"), want, "all miss")
    filled_dev.zero_()
    assert_all_same(multi_live(mt, miss, bgr_of(rgb), raw, True, "bilateral", depth_filled=filled_dev), want, "all miss, depth_filled")
    assert np.array_equal(filled_dev.cpu().numpy().view(np.uint16), mt.engine.fill_depth(raw, 2.0, False, "bilateral"))
    mt.close()


def test_two_heavily_overlapping_windows(se3, models, frames):
    rgb, raw = frames[2]
    P = Fx.pose(3, (0.02, -0.01, 0.8))
    trks = [make_tracker(se3, models, "30deg", "ellipsoid", 150.0), make_tracker(se3, models, "5deg", "sphere", 120.0)]
    mt = se3.MultiTracker(trks)
    got = multi_live(mt, [P, P], bgr_of(rgb), raw, True, "bilateral")
    for i, t in enumerate(trks):
        assert_same(got[i], single_live(t, P, bgr_of(rgb), raw, True, "bilateral"), ("overlap", i))
    assert not np.array_equal(got[0]["bbox"], got[1]["bbox"])
    mt.close()


def test_thirty_three_objects(se3, trackers, frames):
    """two crop launches (32 objects each at most) and seven network chunks"""
    rgb, raw = frames[0]
    trks = list(trackers[:3]) * 11
    poses = poses_inside(33, seed=4)
    mt = se3.MultiTracker(trks)
    got = multi_live(mt, poses, bgr_of(rgb), raw, True, "bilateral")
    assert_all_same(got, multi_composed(mt, poses, rgb, raw, "bilateral"), "n = 33")
    for i in (0, 16, 32):
        assert_same(got[i], single_live(trks[i], poses[i], bgr_of(rgb), raw, True, "bilateral"), ("single", i))
    mt.close()


def _frame_route_trackers(se3, models):
    big, mid = Fx.textured_sphere(3, 0.06), Fx.textured_sphere(2, 0.045)
    t = big["texture"]
    tex2 = np.ascontiguousarray(t[(np.arange(40) * t.shape[0]) // 40][:, (np.arange(24) * t.shape[1]) // 24][::-1, :, ::-1][..., [1, 2, 0]])
    meshes = [dict(vertices=big["vertices"], faces=big["faces"], colors=big["colors"], uv=big["uv"], texture=big["texture"], kd=big["kd"]),
              dict(vertices=mid["vertices"], faces=mid["faces"], colors=mid["colors"], uv=mid["uv"], texture=tex2, kd=np.array([1.0, 0.85, 0.95]))]
    out = []
    for (model, mesh) in (("30deg", meshes[0]), ("random", meshes[1])):
        sd, mean, std, tn, rn = models[model]
        trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0, renderer="pyrenderer"), mean, std, {"state_dict": sd},
                          trans_normalizer=tn, rot_normalizer=rn, max_samples=1)
        trk.renderer = se3.HipRenderer(trk.engine, mesh, mode="pyrender", frame_size=(H, W))
        assert trk.renderer.full_frame and trk.one_call
        out.append(trk)
    return out


def test_frame_route(se3, models, frames):
    """SE3TN_ROUTE_FRAME: two textured objects, one with its window partly outside the frame"""
    rgb, raw = frames[1]
    trks = _frame_route_trackers(se3, models)
    poses = [Fx.pose(4, (0.0, 0.0, 0.7)), Fx.pose(4, (-0.18, 0.0, 0.7))]
    assert [window_kind(se3, P) for P in poses] == ["inside", "L"]
    mt = se3.MultiTracker(trks)
    want = multi_composed(mt, poses, rgb, raw, "bilateral")
    assert all((w["depthA"] > 0).any() for w in want)
    assert_all_same(multi_live(mt, poses, bgr_of(rgb), raw, True, "bilateral"), want, "frame route")
    mt.close()


def test_live_multi_tracker_one_call_equals_the_composition(se3, trackers, frames):
    trks = trackers[:3]
    P0 = np.stack(poses_inside(3, seed=2))
    step = se3.LiveMultiTracker(se3.MultiTracker(trks), P0)
    one = se3.LiveMultiTracker(se3.MultiTracker(trks), P0, one_call=True)
    assert not step.one_call and one.one_call
    assert step.on_track() is None and one.on_track() is None            # nothing grabbed yet
    one.grab_depth(frames[0][1])
    assert one.on_track() is None                                        # no colour frame yet
    one.reset(P0)
    for i, (bgr, raw) in enumerate(frames):                              # (the fixture's channels taken as B, G, R)
        outs = []
        for lt in (step, one):
            lt.grab_depth(raw)
            lt.grab_color(bgr, stamp=10.0 + i)
            res = lt.on_track()
            assert len(res) == 3
            outs.append(([np.asarray(r[0]).copy() for r in res], [np.asarray(r[1], np.float64) for r in res], [r[2] for r in res],
                         lt.A_in_cam.copy(), lt.depth.copy()))
        for a, b in zip(*outs):
            assert np.array_equal(np.asarray(a), np.asarray(b)), i
        assert outs[1][2] == [10.0 + i] * 3 and outs[1][4].dtype == np.uint16 and outs[1][4].shape == (H, W)
        assert np.array_equal(outs[1][4], one.tracker.engine.fill_depth(raw, 2.0, False, "bilateral"))
        assert np.array_equal(np.stack(outs[1][0]), one.A_in_cam[:, :3, 3])
    assert all(not np.array_equal(one.A_in_cam[k], P0[k]) for k in range(3))   # the poses move
    one.reset(P0)
    assert one.on_track() is None and one.depth is None and np.array_equal(one.A_in_cam, P0)
    with pytest.raises(ValueError):
        se3.LiveMultiTracker(one.tracker, P0[:2])
    step.tracker.close()
    one.tracker.close()


def _raw_call(se3, ctx, objs, poses, color, raw, K, order=1, blur=1):
    lib = se3._lib.load()
    n = len(objs)
    arr = (se3._lib.Object * max(n, 1))(*objs)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    out = np.zeros((max(n, 1), 16))
    Kc = np.ascontiguousarray(K, np.float64)
    return lib.se3tn_on_track_objects_live(ctx._h, n, arr, C.c_void_p(P.ctypes.data), Kc.ctypes.data_as(C.POINTER(C.c_double)),
                                           C.c_void_p(color.ctypes.data), order, C.c_void_p(raw.ctypes.data), H, W, 2.0, 0, blur, None, None,
                                           None, C.c_void_p(out.ctypes.data), None, None, None, None), out


def test_refusals_leave_the_context_usable(se3, trackers, models, frames):
    rgb, raw = frames[2]
    trks = trackers[:3]
    good = poses_inside(3, seed=6)
    mt = se3.MultiTracker(trks)
    want = multi_live(mt, good, rgb, raw, False, "bilateral")

    def good_call_is_right(what):
        assert_all_same(multi_live(mt, good, rgb, raw, False, "bilateral"), want, what)

    for z in (0.0, -0.5):                                                 # a pose at / behind the camera plane in the MIDDLE of the list
        bad = [p.copy() for p in good]
        bad[1][2, 3] = z
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
            mt.on_track_live(np.stack(bad), rgb, raw)
        good_call_is_right(("z", z))
    with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
        mt.on_track_live(np.stack(good), rgb, raw, bgr=2)                 # colour order 2
    good_call_is_right("colour order")
    with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
        mt.on_track_live(np.stack(good), rgb, raw, blur_type=7)
    good_call_is_right("blur")
    # a call that mixes the routes (MultiTracker refuses to be built that way: through the C ABI)
    fr = _frame_route_trackers(se3, models)[0]
    obj = lambda t: se3._lib.Object(t.engine._h.value, t.renderer._m.value, float(t.object_width))   # noqa: E731
    rc, _ = _raw_call(se3, mt.engine, [obj(trks[0]), obj(fr), obj(trks[2])], good, rgb, raw, mt.K, order=0)
    assert rc == E_ARG and b"mixes" in se3._lib.load().se3tn_last_error()
    rc, out = _raw_call(se3, mt.engine, [obj(t) for t in trks], good, rgb, raw, mt.K, order=0)
    assert rc == 0 and np.array_equal(out.reshape(3, 4, 4), np.stack([w["pose"] for w in want]))
    good_call_is_right("mixed routes")
    # inside a stream capture: the call is synchronous and says so instead of breaking the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_STATE):
            mt.on_track_live(np.stack(good), rgb, raw)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    good_call_is_right("after the refused capture")
    mt.close()
