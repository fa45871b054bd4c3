"""GPU: the fit check inside the one-call tracking bodies (se3tn_set_fit_check) -- se3tn_on_track, _live, _batch, _objects and
_objects_live, on the window route and on the full-frame route.

Expected record of a pair, from calls the library already had:
  model image     window route: renderer.render_device(estimate, K, gl_window(previous pose));
                  frame route:  O.crop_bbox of renderer.render_frame(estimate) at the previous pose's bbox
  observed image  O.crop_bbox of the camera frame at that bbox (live routes: of engine.fill_depth(raw))
  record          utils.fit_stats(model depth, observed depth, tol)
Records, pred_rgb and pred_depth must equal them bit for bit; with the check on, pose / trans / rot / bbox / image A must equal the same
call with the check off on a context that never had it on.

Scene: the 120 x 160 camera of Fx.SOUP_FRAME_K, the ellipsoid of ST.make_object(4) composed into the frame at its true pose
(ST.object_patch / ST.compose_frame) before a wall at 900 mm; the same frame with a 300 mm occluder over the left half of the window;
the wall alone (object removed).  Without the feature every case fails: the attributes and symbols do not exist."""
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
TOL = 25
H, W = Fx.SOUP_FRAME_HW
K = Fx.SOUP_FRAME_K
WIDTH = ST.OBJECT_WIDTH_MM
INFO = dict(Fx.DATASET_INFO, object_width=WIDTH,
            camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
MESHES = {"ellipsoid": ST.make_object(4), "sphere": Fx.icosphere(2, 0.05, 1)}
G_TRUE = Fx.pose(11, (0.004, -0.003, 0.5))                 # where the ellipsoid really is
G_SPHERE = Fx.pose(12, (-0.05, 0.02, 0.62))                # where the sphere really is
P_MISS = Fx.pose(5, (0.6, 0.5, 0.9))                       # a window off the frame
OUT_KEYS = ("pose", "trans", "rot", "bbox", "rgbA", "depthA")
ROUTES = ["window", "frame"]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def near(P, k):
    """a previous pose a tracking step away from P"""
    Q = P.copy()
    Q[:3, 3] += np.array([0.004, -0.003, 0.006]) * (1 + 0.3 * k)
    return Q


def window_of(P):
    bb = O.compute_bbox(P, K, WIDTH, (1000, 1000, 1000))
    return int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())


def misses(P):
    l, t, r, b = window_of(P)
    return r <= 0 or b <= 0 or l >= W or t >= H


@pytest.fixture(scope="module")
def frames():
    """name -> (rgb, depth): `object` (both objects before the wall), `occluded` (a 300 mm occluder over the left half of the
    ellipsoid's window), `removed` (the wall alone).  The wall has holes, so the live routes have something to fill."""
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = Fx.structured_frame(401, H, W)[0]
    wall = (900 + 0.5 * (xx - W / 2) + 0.3 * (yy - H / 2)).astype(np.uint16)
    wall[rng.random((H, W)) < 0.04] = 0
    removed = (rgb, wall)
    obj = removed
    for mesh, G in (("sphere", G_SPHERE), ("ellipsoid", G_TRUE)):
        obj = ST.compose_frame(obj, ST.object_patch(CL.oracle_mesh(MESHES[mesh]), G, K))
    l, t, r, b = window_of(G_TRUE)
    occ_rgb, occ_d = obj[0].copy(), obj[1].copy()
    occ_rgb[t:b, l:(l + r) // 2] = 90
    occ_d[t:b, l:(l + r) // 2] = 300
    assert (obj[1] != wall).sum() > 1500 and not misses(G_TRUE) and not misses(G_SPHERE) and misses(P_MISS)
    return dict(object=obj, occluded=(occ_rgb, occ_d), removed=removed)


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, regime in (("30deg", "ycbineoat_30deg"), ("5deg", "ycb_video_5deg")):
        sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights(regime))
        out[name] = (sd, mean, std) + tuple(CL.REGIMES[regime])
    return out


def make_tracker(se3, models, model, mesh, route):
    sd, mean, std, tn, rn = models[model]
    info = dict(INFO, renderer="pyrenderer") if route == "frame" else INFO
    trk = se3.Tracker(info, mean, std, {"state_dict": sd}, trans_normalizer=tn, rot_normalizer=rn, max_samples=3)
    trk.renderer = se3.HipRenderer(trk.engine, MESHES[mesh], mode="pyrender", frame_size=(H, W)) if route == "frame" \
        else se3.HipRenderer(trk.engine, MESHES[mesh])
    assert trk.one_call and trk.renderer.full_frame == (route == "frame") and trk.fit_check is None
    return trk


@pytest.fixture(scope="module")
def trackers(se3, models):
    """route -> dict(a = ellipsoid, b = sphere: the check gets switched on; off = a's twin that never has it on)"""
    return {r: dict(a=make_tracker(se3, models, "30deg", "ellipsoid", r), b=make_tracker(se3, models, "5deg", "sphere", r),
                    off=make_tracker(se3, models, "30deg", "ellipsoid", r)) for r in ROUTES}


# ---- expected values -----------------------------------------------------------------------------------------------------------------
def crop(rgb, depth, P):
    """O.crop_bbox at P's bbox; a window that misses the frame is all zeros (crop_bbox itself raises there)"""
    if misses(P):
        return np.zeros((176, 176, 3), np.uint8), np.zeros((176, 176), np.uint16)
    return O.crop_bbox(rgb, depth, O.compute_bbox(P, K, WIDTH, (1000, 1000, 1000)))


def model_image(se3, trk, prev, est):
    r = trk.renderer
    if r.full_frame:
        rgb, dep = r.render_frame(est, trk.K)
        return crop(rgb, dep, prev)
    rgb_t = torch.empty((176, 176, 3), dtype=torch.uint8, device="cuda")
    dep_t = torch.empty((176, 176), dtype=torch.int16, device="cuda")
    r.render_device(est, trk.K, se3.HipRenderer.gl_window(prev, trk.K, trk.object_width), rgb_t, dep_t)
    return rgb_t.cpu().numpy(), dep_t.cpu().numpy().view(np.uint16)


def expected(se3, trk, prev, est, frame):
    rgbP, depP = model_image(se3, trk, prev, est)
    obs = crop(frame[0], frame[1], prev)[1]
    return dict(fit=se3.utils.fit_stats(depP, obs, TOL), pred_rgb=rgbP, pred_depth=depP)


def check_fit(se3, lp, i, want, what):
    """record i of last_prediction against the expected one, bit for bit"""
    assert np.array_equal(lp["fit"][i], want["fit"]), (what, lp["fit"][i], want["fit"])
    assert np.array_equal(lp["pred_depth"][i].cpu().numpy().view(np.uint16), want["pred_depth"]), (what, "pred_depth")
    assert np.array_equal(lp["pred_rgb"][i].cpu().numpy(), want["pred_rgb"]), (what, "pred_rgb")
    f = lp["fit"][i]
    assert int(f["seen_px"]) == int(f["inlier_px"]) + int(f["front_px"]) + int(f["behind_px"]) and int(f["tol_mm"]) == TOL


def outputs_single(trk, pose):
    lp = trk.last_prediction
    rA, dA = (lp["rgbA"], lp["depthA"]) if trk.renderer.full_frame else (trk.renderer.rgb, trk.renderer.depth)
    return dict(pose=pose.copy(), trans=lp["trans"].copy(), rot=lp["rot"].copy(), bbox=np.asarray(lp["bbox"]).copy(),
                rgbA=rA.cpu().numpy().copy(), depthA=dA.cpu().numpy().copy())


def outputs_multi(lp, poses):
    return dict(pose=poses.copy(), trans=lp["trans"].copy(), rot=lp["rot"].copy(), bbox=np.asarray(lp["bbox"]).copy(),
                rgbA=torch.stack(list(lp["rgbA"])).cpu().numpy(), depthA=torch.stack(list(lp["depthA"])).cpu().numpy())


def assert_same_outputs(got, want, what):
    for k in OUT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def num(rec, key):
    return int(rec[key])


# ---- se3tn_on_track ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_on_track(se3, trackers, frames, route):
    a, off = trackers[route]["a"], trackers[route]["off"]
    a.fit_check = TOL
    assert a.fit_check == TOL and off.fit_check is None
    prev = near(G_TRUE, 0)
    ratios = {}
    for name, P in (("object", prev), ("occluded", prev), ("removed", prev), ("miss", P_MISS)):
        rgb, depth = frames["object" if name == "miss" else name]
        est = a.on_track(P, rgb, depth)
        got = outputs_single(a, est)
        lp = a.last_prediction
        want = expected(se3, a, P, est, (rgb, depth))
        check_fit(se3, lp, 0, want, (route, name))
        f = want["fit"]
        # preconditions on the expected values: the cases show what they are meant to show
        if name == "object":
            assert num(f, "inlier_px") > 300 and num(f, "model_px") > 2000
        if name == "occluded":
            assert num(f, "inlier_px") > 0 and num(f, "front_px") > 0
        if name == "removed":
            assert num(f, "behind_px") > 0
        if name == "miss":
            assert num(f, "seen_px") == 0 and (num(f, "model_px") > 0 or route == "frame")   # (frame route: the rectangle is empty too)
        ratios[name] = a.last_fit_ratio
        assert a.last_fit_ratio == (num(f, "inlier_px") / num(f, "model_px") if num(f, "model_px") else 0.0)
        # the check changes nothing else: the same call with the check off, on a context that never had it on
        est_off = off.on_track(P, rgb, depth)
        assert_same_outputs(got, outputs_single(off, est_off), (route, name))
        assert "fit" not in off.last_prediction and off.last_fit_ratio is None
    assert ratios["object"] > ratios["removed"]                  # the one ordering: the object being there fits better than its absence
    a.fit_check = None


# ---- se3tn_on_track_live -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_on_track_live(se3, trackers, frames, route):
    a, off = trackers[route]["a"], trackers[route]["off"]
    a.fit_check = TOL
    rgb, raw = frames["object"]
    assert (raw == 0).mean() > 0.02
    filled = a.engine.fill_depth(raw, 2.0, False, "bilateral")
    assert not np.array_equal(filled, raw)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    for name, P in (("object", near(G_TRUE, 1)), ("miss", P_MISS)):
        est = a.on_track_live(P, bgr, raw, bgr=True)
        got = outputs_single(a, est)
        want = expected(se3, a, P, est, (rgb, filled))           # the observed depth is the FILLED window the rectangle pass wrote
        check_fit(se3, a.last_prediction, 0, want, (route, name))
        if name == "object":
            assert num(want["fit"], "inlier_px") > 300
            assert not np.array_equal(want["fit"], expected(se3, a, P, est, (rgb, raw))["fit"])   # ... not the raw one
        est_off = off.on_track_live(P, bgr, raw, bgr=True)
        assert_same_outputs(got, outputs_single(off, est_off), (route, name))
    # the live front end passes the switch and the ratio through
    lt = se3.LiveTracker(a, near(G_TRUE, 1), one_call=True)
    assert lt.fit_check == TOL
    lt.grab_depth(raw); lt.grab_color(bgr, 1.0)
    lt.on_track()
    assert lt.last_fit_ratio == a.last_fit_ratio and lt.last_fit_ratio > 0
    a.fit_check = None


# ---- se3tn_on_track_batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_on_track_batch(se3, trackers, frames, route):
    a, off = trackers[route]["a"], trackers[route]["off"]
    a.fit_check = TOL
    poses = [near(G_TRUE, 0), near(G_TRUE, 2), P_MISS]
    names = ["object", "occluded", "removed"]
    rgbs, depths = [frames[k][0] for k in names], [frames[k][1] for k in names]
    est = a.on_track_batch(poses, rgbs, depths)
    got = outputs_multi(a.last_prediction, est)
    lp = a.last_prediction
    assert lp["fit"].shape == (3,) and tuple(lp["pred_rgb"].shape) == (3, 176, 176, 3) and a.last_fit_ratio.shape == (3,)
    for i in range(3):
        want = expected(se3, a, poses[i], est[i], (rgbs[i], depths[i]))
        check_fit(se3, lp, i, want, (route, i))
    assert a.last_fit_ratio[0] > 0 and num(lp["fit"][2], "seen_px") == 0
    assert np.array_equal(a.last_fit_ratio, se3.utils.fit_ratio(lp["fit"]))
    est_off = off.on_track_batch(poses, rgbs, depths)
    assert_same_outputs(got, outputs_multi(off.last_prediction, est_off), route)
    assert "fit" not in off.last_prediction
    a.fit_check = None


# ---- se3tn_on_track_objects / _objects_live ------------------------------------------------------------------------------------------------
def object_poses(n):
    base = [near(G_TRUE, 0), near(G_SPHERE, 0), near(G_TRUE, 3), near(G_SPHERE, 2), P_MISS, near(G_SPHERE, 4)]
    return base[:n]


@pytest.mark.parametrize("n", [1, 5, 6])
@pytest.mark.parametrize("route", ROUTES)
def test_on_track_objects(se3, trackers, frames, route, n):
    """n = 6 makes two network chunks (5 + 1); objects alternate between the two trackers (model, mesh), object 4 misses the frame"""
    trks = [trackers[route]["a" if i % 2 == 0 else "b"] for i in range(n)]
    poses = object_poses(n)
    rgb, depth = frames["occluded"]
    mt = se3.MultiTracker(trks)
    mt.fit_check = TOL
    est = mt.on_track(np.stack(poses), rgb, depth)
    got = outputs_multi(mt.last_prediction, est)
    lp = mt.last_prediction
    assert lp["fit"].shape == (n,) and mt.last_fit_ratio.shape == (n,)
    for i in range(n):
        check_fit(se3, lp, i, expected(se3, trks[i], poses[i], est[i], (rgb, depth)), (route, n, i))
    assert num(lp["fit"][0], "front_px") > 0 and num(lp["fit"][0], "model_px") > 2000
    if n > 4:
        assert num(lp["fit"][4], "seen_px") == 0
    mt.close()
    plain = se3.MultiTracker(trks)                                  # a fresh executing context, check off
    assert plain.fit_check is None
    est_off = plain.on_track(np.stack(poses), rgb, depth)
    assert_same_outputs(got, outputs_multi(plain.last_prediction, est_off), (route, n))
    assert "fit" not in plain.last_prediction and plain.last_fit_ratio is None
    plain.close()


@pytest.mark.parametrize("route", ROUTES)
def test_on_track_objects_live(se3, trackers, frames, route):
    trks = [trackers[route][k] for k in ("a", "b", "a")]
    poses = [near(G_TRUE, 1), near(G_SPHERE, 1), P_MISS]
    rgb, raw = frames["object"]
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    mt = se3.MultiTracker(trks)
    mt.fit_check = TOL
    filled = mt.engine.fill_depth(raw, 2.0, False, "bilateral")
    est = mt.on_track_live(np.stack(poses), bgr, raw, bgr=True)
    got = outputs_multi(mt.last_prediction, est)
    for i in range(3):
        check_fit(se3, mt.last_prediction, i, expected(se3, trks[i], poses[i], est[i], (rgb, filled)), (route, i))
    assert num(mt.last_prediction["fit"][0], "inlier_px") > 300 and num(mt.last_prediction["fit"][2], "seen_px") == 0
    lm = se3.LiveMultiTracker(mt, np.stack(poses), one_call=True)
    lm.grab_depth(raw); lm.grab_color(bgr, 2.0)
    lm.on_track()
    assert lm.fit_check == TOL and np.array_equal(lm.last_fit_ratio, mt.last_fit_ratio) and lm.last_fit_ratio[0] > 0
    mt.close()
    plain = se3.MultiTracker(trks)
    est_off = plain.on_track_live(np.stack(poses), bgr, raw, bgr=True)
    assert_same_outputs(got, outputs_multi(plain.last_prediction, est_off), route)
    plain.close()


# ---- the step-by-step path gives the same records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_one_call_and_step_by_step_give_equal_records(se3, trackers, frames, route):
    a = trackers[route]["a"]
    a.fit_check = TOL
    rgb, depth = frames["occluded"]
    runs = {}
    for one_call in (True, False):
        a.one_call = one_call
        single = []
        for P in (near(G_TRUE, 0), P_MISS):
            a.on_track(P, rgb, depth)
            lp = a.last_prediction
            single.append((lp["fit"].copy(), lp["pred_rgb"].cpu().numpy().copy(), lp["pred_depth"].cpu().numpy().copy(), a.last_fit_ratio))
        a.on_track_batch([near(G_TRUE, 0), near(G_TRUE, 2)], [rgb, frames["removed"][0]], [depth, frames["removed"][1]])
        lp = a.last_prediction
        runs[one_call] = (single, (lp["fit"].copy(), lp["pred_rgb"].cpu().numpy().copy(), lp["pred_depth"].cpu().numpy().copy(),
                                   np.asarray(a.last_fit_ratio)))
    a.one_call = True
    a.fit_check = None
    for x, y in zip(runs[True][0] + [runs[True][1]], runs[False][0] + [runs[False][1]]):
        for u, v in zip(x, y):
            assert np.array_equal(np.asarray(u), np.asarray(v)), route
    assert int(runs[True][0][0][0]["inlier_px"][0]) > 0 and int(runs[True][0][0][0]["front_px"][0]) > 0


# ---- state ---------------------------------------------------------------------------------------------------------------------------------
def test_state_toggling_and_refusals(se3, trackers, frames):
    a = trackers["window"]["a"]
    lib, h = a.engine.lib, a.engine._h
    rgb, depth = frames["object"]
    P = near(G_TRUE, 0)
    rec = (se3._lib.Fit * 3)()
    img = C.c_void_p()

    def right(what):
        est = a.on_track(P, rgb, depth)
        check_fit(se3, a.last_prediction, 0, expected(se3, a, P, est, (rgb, depth)), what)
        assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == 0 and rec[0].tol_mm == TOL and rec[0].model_px > 2000
        assert lib.se3tn_last_fit_images(h, C.byref(img), None) == 0 and img.value

    def off(what):
        a.on_track(P, rgb, depth)
        assert "fit" not in a.last_prediction and a.last_fit_ratio is None, what
        assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == E_STATE and b"se3tn_last_fit" in lib.se3tn_last_error()
        assert lib.se3tn_last_fit_images(h, C.byref(img), None) == E_STATE

    a.fit_check = None
    off("never on")                                    # a check-off call leaves no records
    a.fit_check = TOL
    right("on")
    assert lib.se3tn_last_fit(h, 2, C.byref(rec)) == E_STATE          # the last call held one pair, not two
    assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == 0                # ... and the refusal took nothing away
    a.fit_check = None
    off("off again")                                   # ... and not the records of the call before it
    a.fit_check = TOL
    right("on again")
    # a batch of another size on the same context, then back
    a.on_track_batch([P, near(G_TRUE, 2)], [rgb, rgb], [depth, depth])
    assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == E_STATE and lib.se3tn_last_fit(h, 2, C.byref(rec)) == 0
    right("after the batch")
    # bad tolerances are refused and leave the setting alone
    for bad in (-1, 65536):
        assert lib.se3tn_set_fit_check(h, bad) == E_ARG
    assert a.fit_check == TOL
    # with the check on a call inside a stream capture is refused; the context stays usable
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(se3._lib.Se3tnError, match="captured"):
            a.on_track(P, rgb, depth)
    assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == E_STATE          # the refused call left no records
    right("after the refused capture")
    # a refused tracking call (a pose behind the camera) leaves no records either
    behind = P.copy(); behind[2, 3] = -0.5
    with pytest.raises(se3._lib.Se3tnError):
        a.on_track(behind, rgb, depth)
    assert lib.se3tn_last_fit(h, 1, C.byref(rec)) == E_STATE
    right("after the refused pose")
    a.fit_check = None
