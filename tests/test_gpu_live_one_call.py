"""GPU: se3tn_on_track_live (predict_ros.py:38-60 in one library call) against the composition the library already had --
engine.fill_depth of the raw frame on the host round trip, then Tracker.on_track on the filled frame.  The same kernels see the same
bytes, so pose, (trans, rot), bbox and image A are compared BIT FOR BIT."""
import numpy as np
import pytest
import torch

from oracle import fixtures as Fx
from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
H, W = 480, 640


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def trk(se3):
    """window route: the built-in rasteriser on a vertex-colour mesh"""
    mean, std = Fx.mean_std(0)
    t = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, max_samples=1)
    t.renderer = se3.HipRenderer(t.engine, Fx.icosphere(2, 0.05, 1))
    assert t.one_call and not t.renderer.full_frame
    return t


@pytest.fixture(scope="module")
def trk_frame(se3):
    """SE3TN_ROUTE_FRAME: the textured fixture through the full-frame renderer"""
    mean, std = Fx.mean_std(3)
    t = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0, renderer="pyrenderer"), mean, std,
                    {"state_dict": O.make_state_dict(5, head_gain=0.01)}, max_samples=1)
    m = Fx.textured_sphere(3, 0.06)
    t.renderer = se3.HipRenderer(t.engine, dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], uv=m["uv"],
                                                texture=m["texture"], kd=m["kd"]), mode="pyrender", frame_size=(H, W))
    assert t.one_call and t.renderer.full_frame
    return t


@pytest.fixture(scope="module")
def frames():
    out = [Fx.synthetic_frame(120 + i) for i in range(3)]
    for rgb, depth in out:
        assert rgb.shape == (H, W, 3) and (depth == 0).mean() > 0.03      # 480 x 640 with holes
    return out


def record(t, pose):
    lp = t.last_prediction
    if "rgbA" in lp:
        rgbA, depthA = lp["rgbA"], lp["depthA"]
    else:
        rgbA, depthA = t.renderer.rgb, t.renderer.depth
    return dict(pose=pose.copy(), trans=lp["trans"].reshape(3).copy(), rot=lp["rot"].reshape(3).copy(),
                bbox=np.asarray(lp["bbox"]).reshape(4, 2).copy(), rgbA=rgbA.cpu().numpy().copy(), depthA=depthA.cpu().numpy().view(np.uint16).copy())


def composed(t, P, rgb, raw, blur):
    filled = t.engine.fill_depth(raw, 2.0, False, blur)
    return record(t, t.on_track(P, rgb, filled))


def live(t, P, color, raw, bgr, blur, **kw):
    return record(t, t.on_track_live(P, color, raw, bgr=bgr, max_depth=2.0, extrapolate=False, blur_type=blur, **kw))


def assert_same(got, want, what):
    for k in ("pose", "trans", "rot", "bbox", "rgbA", "depthA"):
        assert np.array_equal(got[k], want[k]), (what, k)


def window_kind(se3, P, width=150.0):
    l, t, r, b = se3.crop_window(se3.compute_bbox(P, Fx.K_YCB, width))
    if r <= 0 or b <= 0 or l >= W or t >= H:
        return "miss"
    return ("L" if l < 0 else "") + ("T" if t < 0 else "") + ("R" if r > W else "") + ("B" if b > H else "") or "inside"


@pytest.mark.parametrize("blur", ["bilateral", None], ids=["bilateral", "None"])
@pytest.mark.parametrize("bgr", [True, False], ids=["bgr", "rgb"])
def test_closed_loop_equals_fill_depth_then_on_track(se3, trk, frames, bgr, blur):
    P0 = Fx.pose(3, (0.02, -0.01, 0.8))
    assert window_kind(se3, P0) == "inside"
    want, P = [], P0
    for rgb, raw in frames:
        want.append(composed(trk, P, rgb, raw, blur))
        P = want[-1]["pose"]
    assert not np.array_equal(want[0]["pose"], P0) and not np.array_equal(want[1]["trans"], want[0]["trans"])   # the loop moves
    P = P0
    for i, (rgb, raw) in enumerate(frames):
        color = np.ascontiguousarray(rgb[:, :, ::-1]) if bgr else rgb
        got = live(trk, P, color, raw, bgr, blur)
        assert_same(got, want[i], (bgr, blur, i))
        P = got["pose"]


def test_frame_route_equals_fill_depth_then_on_track(se3, trk_frame, frames):
    rgb, raw = frames[0]
    for t in ((0.0, 0.0, 0.7), (-0.18, 0.0, 0.7)):
        P = Fx.pose(4, t)
        want = composed(trk_frame, P, rgb, raw, "bilateral")
        assert (want["depthA"] > 0).any()
        assert_same(live(trk_frame, P, np.ascontiguousarray(rgb[:, :, ::-1]), raw, True, "bilateral"), want, t)


@pytest.mark.parametrize("kind,t", [("LT", (-0.2, -0.17, 0.75)), ("RB", (0.2, 0.14, 0.7)), ("miss", (0.6, 0.5, 0.9))], ids=["left_top", "right_bottom", "miss"])
def test_windows_leaving_the_frame(se3, trk, frames, kind, t):
    P = Fx.pose(5, t)
    assert window_kind(se3, P) == kind
    filled_dev = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    for i, (rgb, raw) in enumerate(frames):        # the pose is held: the window stays where it is
        want = composed(trk, P, rgb, raw, "bilateral")
        assert_same(live(trk, P, np.ascontiguousarray(rgb[:, :, ::-1]), raw, True, "bilateral"), want, (kind, i))
        assert_same(live(trk, P, rgb, raw, False, "bilateral", depth_filled=filled_dev), want, (kind, i, "depth_filled"))
        assert np.array_equal(filled_dev.cpu().numpy().view(np.uint16), trk.engine.fill_depth(raw, 2.0, False, "bilateral"))


@pytest.mark.parametrize("blur", ["bilateral", "gaussian", None], ids=["bilateral", "gaussian", "None"])
def test_depth_filled_is_the_whole_filled_frame(trk, frames, blur):
    rgb, raw = frames[1]
    P = Fx.pose(3, (0.02, -0.01, 0.8))
    filled_dev = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    got = live(trk, P, rgb, raw, False, blur, depth_filled=filled_dev)
    assert np.array_equal(filled_dev.cpu().numpy().view(np.uint16), trk.engine.fill_depth(raw, 2.0, False, blur))
    assert_same(got, composed(trk, P, rgb, raw, blur), blur)


def test_live_tracker_one_call_equals_step_by_step(se3, trk, frames):
    P0 = Fx.pose(3, (0.02, -0.01, 0.8))
    step, one = se3.LiveTracker(trk, P0), se3.LiveTracker(trk, P0, one_call=True)
    assert not step.one_call and one.one_call
    assert step.on_track() is None and one.on_track() is None            # nothing grabbed yet
    for i, (bgr, raw) in enumerate(frames):                              # (the fixture's channels taken as B, G, R)
        outs = []
        for lt in (step, one):
            lt.grab_depth(raw)
            lt.grab_color(bgr, stamp=10.0 + i)
            trans, q, stamp = lt.on_track()
            outs.append((np.asarray(trans).copy(), np.asarray(q, np.float64), stamp, lt.A_in_cam.copy(), lt.depth.copy()))
        for a, b in zip(*outs):
            assert np.array_equal(a, b), i
        assert outs[1][2] == 10.0 + i and outs[1][4].dtype == np.uint16 and outs[1][4].shape == (H, W)
    assert not np.array_equal(one.A_in_cam, P0)
    one.reset(P0)
    assert one.on_track() is None and one.depth is None


def test_refusals_leave_the_context_usable(se3, trk, frames):
    rgb, raw = frames[2]
    good = Fx.pose(3, (0.0, 0.0, 0.8))
    want = live(trk, good, rgb, raw, False, "bilateral")
    for z in (0.0, -0.5):
        P = good.copy(); P[2, 3] = z
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
            trk.on_track_live(P, rgb, raw)
    with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
        trk.on_track_live(good, rgb, raw, bgr=2)                          # color_order 2
    with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_ARG):
        trk.on_track_live(good, rgb, raw, blur_type=7)
    assert_same(live(trk, good, rgb, raw, False, "bilateral"), want, "after the argument refusals")
    # inside a stream capture: the call is synchronous and says so instead of breaking the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d" % E_STATE):
            trk.on_track_live(good, rgb, raw)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert_same(live(trk, good, rgb, raw, False, "bilateral"), want, "after the refused capture")
