"""se3tn_on_track_objects / MultiTracker on the full-frame (pyrender) route: several DIFFERENT textured objects in one camera frame per
call -- the configuration the reference ships (dataset_info `renderer: pyrenderer`, one textured .obj and one set of weights per YCB
class).  The contract is the one of the window route (tests/test_gpu_multi_object.py): every object gets exactly the bits
se3tn_on_track on its own model context gives it, whatever n, the chunking, the order or the company -- now with each instance of
the FOUR rasteriser launches bringing its own mesh, its own material (texture pyramid of its own size, or vertex colours under its
own Kd) and its own rectangle of the frame.

Objects: three meshes that differ in face count and radius (Fx.textured_sphere subdivisions 2 / 3 / 4), in material (the fixture's
64 x 128 texture; a 40 x 24 resampled, channel-permuted copy under another Kd; none at all, vertex colours under a non-unit Kd) and
in model (the two trained stand-ins and a random-init one: other weights, mean / std, normalisers).  Image A is pinned to
se3tn_render_frame (what tests/test_renderer.py and tests/test_gl_swiftshader.py pin to the oracles), not to a second copy of the
batched launch.  Every case fails before the feature with SE3TN_E_ARG / ValueError."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import closed_loop as CL
from oracle import fixtures as Fx
from oracle import free_run as FR
from oracle import se3_oracle as O
from oracle import synth_track as ST
from oracle import ycbv_fixtures as YF

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
H, W = 480, 640
# tests/test_gpu_frame_route.py: translations (YCB camera, 150 mm object width) and where their crop window lies
WINDOWS = [
    ("inside", (0.0, 0.0, 0.7)),
    ("left", (-0.18, 0.0, 0.7)),
    ("right", (0.2, 0.0, 0.7)),
    ("top", (0.0, -0.13, 0.7)),
    ("bottom", (0.0, 0.14, 0.7)),
    ("miss", (0.6, 0.5, 0.9)),
    ("larger", (0.0, 0.0, 0.3)),
]


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


def _meshes():
    big, mid, small = Fx.textured_sphere(3, 0.06), Fx.textured_sphere(2, 0.045), Fx.textured_sphere(4, 0.05)
    # another texture: resampled to 40 x 24 (other size, other number of mip levels), channels permuted, rows reversed
    t = big["texture"]
    yy = (np.arange(40) * t.shape[0]) // 40
    xx = (np.arange(24) * t.shape[1]) // 24
    tex2 = np.ascontiguousarray(t[yy][:, xx][::-1, :, ::-1][..., [1, 2, 0]])
    pick = lambda m, **kw: dict(dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"]), **kw)
    return {
        "textured": pick(big, uv=big["uv"], texture=big["texture"], kd=big["kd"]),                    # 1280 faces, 64 x 128 texture
        "retextured": pick(mid, uv=mid["uv"], texture=tex2, kd=np.array([1.0, 0.85, 0.95])),          # 320 faces, 40 x 24 texture
        "plain": pick(small, kd=np.array([0.7, 0.9, 0.6])),                                          # 5120 faces, vertex colours x Kd
    }


MESHES = _meshes()
assert len({len(m["faces"]) for m in MESHES.values()}) == 3


def make_tracker(se3, models, model, mesh, width, frame_hw=(H, W)):
    sd, mean, std, tn, rn = models[model]
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=width, renderer="pyrenderer"), mean, std, {"state_dict": sd},
                      trans_normalizer=tn, rot_normalizer=rn, max_samples=1)
    trk.renderer = se3.HipRenderer(trk.engine, MESHES[mesh], mode="pyrender", frame_size=frame_hw)
    assert trk.renderer.full_frame and trk.one_call
    trk.spec = (model, mesh, width)          # (test bookkeeping)
    return trk


SPECS = [("30deg", "textured", 150.0), ("5deg", "retextured", 120.0), ("random", "plain", 140.0), ("5deg", "textured", 150.0),
         ("30deg", "plain", 110.0), ("random", "retextured", 130.0), ("30deg", "textured", 160.0)]


@pytest.fixture(scope="module")
def trackers(se3, models):
    return [make_tracker(se3, models, *s) for s in SPECS]


@pytest.fixture(scope="module")
def trackers150(se3, models):
    """one tracker per WINDOWS case, all 150 mm wide (the width the cases were made for), cycling the three objects"""
    return [make_tracker(se3, models, SPECS[i % 3][0], SPECS[i % 3][1], 150.0) for i in range(len(WINDOWS))]


def frame_and_poses(n, seed=0):
    rgb, depth = Fx.structured_frame(400 + seed)
    poses = [Fx.pose(50 + 7 * seed + i, (0.09 * np.cos(1.3 * i + seed), 0.06 * np.sin(0.9 * i + seed), 0.7 + 0.04 * i)) for i in range(n)]
    return rgb, depth, poses


def single(trk, P, rgb, depth):
    """what se3tn_on_track on the object's own context gives on this route: pose, trans, rot, bbox, the raw crop of the render"""
    assert trk.one_call
    pose = trk.on_track(P, rgb, depth)
    lp = trk.last_prediction
    return dict(pose=pose, trans=lp["trans"].reshape(3).copy(), rot=lp["rot"].reshape(3).copy(), bbox=np.asarray(lp["bbox"]).reshape(4, 2).copy(),
                rgbA=lp["rgbA"].cpu().numpy().copy(), depthA=lp["depthA"].cpu().numpy().view(np.uint16).copy())


def multi(se3, trks, poses, rgb, depth):
    mt = se3.MultiTracker(trks)
    n = len(trks)
    bb = np.empty((n, 4, 2), np.int32)
    out = mt.on_track(np.stack(poses), rgb, depth, bbox_out=bb)
    lp = mt.last_prediction
    res = [dict(pose=out[i].copy(), trans=lp["trans"][i].copy(), rot=lp["rot"][i].copy(), bbox=bb[i].copy(), rgbA=lp["rgbA"][i].cpu().numpy(),
                depthA=lp["depthA"][i].cpu().numpy().view(np.uint16)) for i in range(n)]
    mt.close()
    return res


def assert_same(got, want, what):
    for k in ("pose", "trans", "rot", "bbox", "rgbA", "depthA"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def covered(rec):
    return int((rec["depthA"] > 0).sum())


def render_window(trk, P):
    """Tracker.render_window: se3tn_render_frame of the whole frame, then crop_bbox on the device"""
    rgbA, depthA = trk.render_window(P)
    to_np = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return to_np(rgbA), to_np(depthA).view(np.uint16)


def kind(P, width=150.0):
    bb = O.compute_bbox(P, Fx.K_YCB, width, (1000, 1000, 1000))
    left, top, right, bottom = bb[:, 1].min(), bb[:, 0].min(), bb[:, 1].max(), bb[:, 0].max()
    if right <= 0 or bottom <= 0 or left >= W or top >= H:
        return "miss"
    if top < 0 and bottom > H:
        return "larger"
    return "left" if left < 0 else "right" if right > W else "top" if top < 0 else "bottom" if bottom > H else "inside"


# ---- bit equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_each_object_gets_the_bits_of_its_own_single_object_call(se3, trackers, n):
    """n = 7 crosses the chunk boundary of the network (5 + 2) and repeats every model"""
    rgb, depth, poses = frame_and_poses(n, seed=n)
    trks = trackers[:n]
    got = multi(se3, trks, poses, rgb, depth)
    for i, t in enumerate(trks):
        want = single(t, poses[i], rgb, depth)
        print("n %d object %d %s: image A covers %d pixels" % (n, i, t.spec, covered(want)))
        assert covered(want) > 300, (n, i)                       # an empty render cannot pass
        assert_same(got[i], want, (n, i, t.spec))
        rgbA, depthA = render_window(t, poses[i])                # ... and that is the crop of se3tn_render_frame
        assert np.array_equal(got[i]["rgbA"], rgbA) and np.array_equal(got[i]["depthA"], depthA), (n, i)
    if n > 1:   # mixed models and objects really differ: the same pose through another tracker gives another image A and output
        other = single(trks[1], poses[0], rgb, depth)
        assert not np.array_equal(got[0]["trans"], other["trans"])
        assert not np.array_equal(got[0]["rgbA"], other["rgbA"])


def test_different_objects_at_one_pose_and_order_and_company(se3, trackers):
    rgb, depth, poses = frame_and_poses(5, seed=11)
    trks = trackers[:5]
    # the three objects (textured, re-textured, vertex colours) at ONE pose and one width-independent place: three different images A
    same = multi(se3, trks[:3], [poses[0]] * 3, rgb, depth)
    for i in range(3):
        assert covered(same[i]) > 300
        assert_same(same[i], single(trks[i], poses[0], rgb, depth), ("one pose", i))
        for j in range(i):
            assert not np.array_equal(same[i]["rgbA"], same[j]["rgbA"]), (i, j)
    base = multi(se3, trks, poses, rgb, depth)
    perm = [3, 0, 4, 2, 1]
    got = multi(se3, [trks[p] for p in perm], [poses[p] for p in perm], rgb, depth)
    for j, p in enumerate(perm):
        assert covered(got[j]) > 300
        assert_same(got[j], base[p], ("permuted", j))
    # the same object (tracker = model + mesh + material) listed twice, with the same pose and with another one, in another company
    got = multi(se3, [trks[1], trks[2], trks[1], trks[1]], [poses[1], poses[2], poses[1], poses[4]], rgb, depth)
    assert_same(got[0], base[1], "twice a")
    assert_same(got[2], base[1], "twice b")
    assert_same(got[1], base[2], "company")
    assert_same(got[3], single(trks[1], poses[4], rgb, depth), "other pose")


# ---- window geometry -------------------------------------------------------------------------------------------------------------
def test_windows_inside_cut_larger_and_off_the_frame_in_one_call(se3, trackers150):
    rgb, depth = Fx.structured_frame(431)
    poses = [Fx.pose(3 + i, t) for i, (_, t) in enumerate(WINDOWS)]
    for (name, _), P in zip(WINDOWS, poses):
        assert kind(P) == name                                   # the window lies where the case says
    got = multi(se3, trackers150, poses, rgb, depth)
    sizes = set()
    for i, (name, _) in enumerate(WINDOWS):
        t = trackers150[i]
        want = single(t, poses[i], rgb, depth)
        assert_same(got[i], want, name)
        rgbA, depthA = render_window(t, poses[i])
        assert np.array_equal(got[i]["rgbA"], rgbA) and np.array_equal(got[i]["depthA"], depthA), name
        print("window %-7s %s: image A covers %d pixels" % (name, t.spec, covered(got[i])))
        if name == "miss":
            assert covered(got[i]) == 0 and not got[i]["rgbA"].any()
            assert np.isfinite(got[i]["pose"]).all()
        else:
            assert covered(got[i]) > 300, name
        bb = got[i]["bbox"]
        x0, x1 = max(int(bb[:, 1].min()), 0), min(int(bb[:, 1].max()), W)
        y0, y1 = max(int(bb[:, 0].min()), 0), min(int(bb[:, 0].max()), H)
        sizes.add((max(x1 - x0, 0), max(y1 - y0, 0)))
    assert len(sizes) >= 5                                       # rectangles of different sizes shared the launch
    # every window off the frame: nothing is rendered, the poses still come out as the single calls give them
    off = [Fx.pose(1, (0.6, 0.5, 0.9)), Fx.pose(2, (-0.7, 0.5, 0.9))]
    got = multi(se3, trackers150[:2], off, rgb, depth)
    for i in range(2):
        assert not got[i]["rgbA"].any() and not got[i]["depthA"].any()
        assert_same(got[i], single(trackers150[i], off[i], rgb, depth), ("all off", i))


# ---- the rendered rectangles ------------------------------------------------------------------------------------------------------
def _unscaled_pose(seed, width, xy):
    """a pose whose crop window is exactly 176 x 176 pixels inside the frame: crop_bbox then copies the rectangle pixel for pixel"""
    for z in np.arange(0.55, 1.2, 0.0005):
        P = Fx.pose(seed, (xy[0], xy[1], float(z)))
        bb = O.compute_bbox(P, Fx.K_YCB, width, (1000, 1000, 1000))
        left, top, right, bottom = int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())
        if right - left == 176 and bottom - top == 176 and left >= 0 and top >= 0 and right <= W and bottom <= H:
            return P, (left, top, right, bottom)
    raise AssertionError("no 176 x 176 window for width %g" % width)


def test_rendered_rectangles_equal_the_slices_of_render_frame(se3, trackers):
    """Where the window is 176 x 176 and inside the frame the raw crop IS the rendered rectangle: every byte of it equals the slice of
    se3tn_render_frame for that object and pose -- three materials, three face counts and three rectangles in one launch."""
    rgb, depth = Fx.structured_frame(440)
    trks = trackers[:3]
    found = [_unscaled_pose(20 + i, t.object_width, xy) for i, (t, xy) in enumerate(zip(trks, ((-0.1, 0.02), (0.08, -0.05), (0.0, 0.06))))]
    poses = [f[0] for f in found]
    got = multi(se3, trks, poses, rgb, depth)
    for i, t in enumerate(trks):
        left, top, right, bottom = found[i][1]
        full_rgb, full_depth = t.renderer.render_frame(poses[i], t.K)
        n_cov = int((full_depth[top:bottom, left:right] > 0).sum())
        print("object %d %s: rectangle %s covers %d pixels" % (i, t.spec, found[i][1], n_cov))
        assert n_cov > 300 and n_cov == int((full_depth > 0).sum())            # the whole object lies in the rectangle
        assert np.array_equal(got[i]["depthA"], full_depth[top:bottom, left:right]), i
        assert np.array_equal(got[i]["rgbA"], full_rgb[top:bottom, left:right]), i
    assert len(np.unique(got[0]["rgbA"].reshape(-1, 3), axis=0)) > 300         # (a texture, not a flat colour)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_against_the_oracle_per_object(se3, trackers, models):
    rgb, depth, poses = frame_and_poses(5, seed=3)
    trks = trackers[:5]
    got = multi(se3, trks, poses, rgb, depth)
    for i, t in enumerate(trks):
        sd, mean, std, tn, rn = models[t.spec[0]]
        assert covered(got[i]) > 300
        want, aux = O.on_track(sd, poses[i], rgb, depth, got[i]["rgbA"], got[i]["depthA"], t.K, t.object_width, mean, std, tn, rn)
        err_t, err_r = np.abs(got[i]["trans"] - aux["trans"]).max(), np.abs(got[i]["rot"] - aux["rot"]).max()
        err_p = np.abs(got[i]["pose"] - want).max()
        print("object %d %s: |d trans| %.3g |d rot| %.3g |d pose| %.3g" % (i, t.spec, err_t, err_r, err_p))
        assert err_t < 1e-4 and err_r < 1e-4, (i, t.spec)
        assert err_p < 1e-5, (i, t.spec)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _call(se3, ctx, objs, poses, rgb, depth, K, hw=None):
    lib = se3._lib.load()
    n = len(objs)
    arr = (se3._lib.Object * max(n, 1))(*objs)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    out = np.zeros((max(n, 1), 16))
    Kc = np.ascontiguousarray(K, np.float64)
    h, w = hw if hw is not None else rgb.shape[:2]
    rc = lib.se3tn_on_track_objects(ctx._h, n, arr, C.c_void_p(P.ctypes.data), Kc.ctypes.data_as(C.POINTER(C.c_double)),
                                    C.c_void_p(rgb.ctypes.data), C.c_void_p(depth.ctypes.data), h, w, None, None,
                                    C.c_void_p(out.ctypes.data), None, None, None, None)
    return rc, out, lib.se3tn_last_error()


def test_refusals_leave_the_context_usable(se3, trackers, models):
    rgb, depth, poses = frame_and_poses(2, seed=21)
    t0, t1 = trackers[0], trackers[2]                            # a textured object and the vertex-colour one
    K = t0.K
    ctx = se3.Engine(0, 2)
    obj = lambda t, mesh=None: se3._lib.Object(t.engine._h.value, mesh if mesh is not None else t.renderer._m.value, float(t.object_width))
    ok = [obj(t0), obj(t1)]
    want = [single(t, poses[i], rgb, depth)["pose"] for i, t in enumerate((t0, t1))]

    def valid():
        rc, out, _ = _call(se3, ctx, ok, poses, rgb, depth, K)
        assert rc == 0
        for i in range(2):
            assert np.array_equal(out[i].reshape(4, 4), want[i]), i
    valid()
    # mixed routes: a vertex-colour mesh on the window route beside a frame-route object
    window_mesh = se3.HipRenderer(t1.engine, Fx.icosphere(3, 0.05, 1))
    rc, _, err = _call(se3, ctx, [ok[0], obj(t1, window_mesh._m.value)], poses, rgb, depth, K)
    assert rc == E_ARG and b"mixes" in err and b"ROUTE_WINDOW" in err and b"ROUTE_FRAME" in err
    valid()
    rc, _, err = _call(se3, ctx, [obj(t1, window_mesh._m.value), ok[0]], poses, rgb, depth, K)
    assert rc == E_ARG and b"mixes" in err
    valid()
    # a textured mesh left on (put back on) the window route
    lib = t0.engine.lib
    tex_window = se3.HipRenderer(t0.engine, MESHES["textured"], mode="pyrender", frame_size=(H, W))
    assert lib.se3tn_mesh_set_route(tex_window._m, se3._lib.ROUTE_WINDOW) == 0
    rc, _, err = _call(se3, ctx, [obj(t0, tex_window._m.value), obj(t0, tex_window._m.value)], poses, rgb, depth, K)
    assert rc == E_ARG and b"textured mesh" in err
    valid()
    # H > 2048
    tall_rgb, tall_depth = np.zeros((2049, 8, 3), np.uint8), np.zeros((2049, 8), np.uint16)
    rc, _, err = _call(se3, ctx, ok, poses, tall_rgb, tall_depth, K)
    assert rc == E_ARG and b"2048" in err
    valid()
    # a pose with z <= 0 / not finite
    for bad in (0.0, -0.5, np.nan, np.inf):
        P = [poses[0], poses[1].copy()]
        P[1][2, 3] = bad
        assert _call(se3, ctx, ok, P, rgb, depth, K)[0] == E_ARG, bad
    valid()
    # a model without weights
    bare = se3.Engine(0, 1)
    rc, _, err = _call(se3, ctx, [ok[0], se3._lib.Object(bare._h.value, t1.renderer._m.value, 120.0)], poses, rgb, depth, K)
    assert rc == E_STATE and b"no weights" in err
    valid()
    # MultiTracker: a mix of routes and an injected renderer name the first offender
    sd, mean, std, tn, rn = models["5deg"]
    win_trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, {"state_dict": sd}, trans_normalizer=tn, rot_normalizer=rn,
                          max_samples=1)
    win_trk.renderer = se3.HipRenderer(win_trk.engine, Fx.icosphere(3, 0.05, 1))
    with pytest.raises(ValueError, match="tracker 2"):
        se3.MultiTracker([t0, t1, win_trk])
    with pytest.raises(ValueError, match="tracker 1"):
        se3.MultiTracker([win_trk, t0, t1])

    class Injected:
        def render(self, ob2cam, K, window):
            return np.zeros((176, 176, 3), np.uint8), np.zeros((176, 176), np.uint16)
    keep = win_trk.renderer
    win_trk.renderer = Injected()
    with pytest.raises(ValueError, match="tracker 1"):
        se3.MultiTracker([t0, win_trk])
    win_trk.renderer = keep
    valid()
    for e in (ctx, bare):
        e.close()


# ---- closed loop -----------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_two_composited_sequences_equals_two_separate_loops(se3, models):
    frames = 30
    K = np.array([[Fx.DATASET_INFO["camera"]["focalX"], 0, Fx.DATASET_INFO["camera"]["centerX"]],
                  [0, Fx.DATASET_INFO["camera"]["focalY"], Fx.DATASET_INFO["camera"]["centerY"]], [0, 0, 1.0]])
    regimes = (("30deg", "ycbineoat_30deg", 2, "textured"), ("5deg", "ycb_video_5deg", 5, "retextured"))
    seqs = [ST.make_sequence(seed, frames + 1, K, regime=reg) for _, reg, seed, _ in regimes]
    bg = ST.backgrounds()

    def frame(f):   # the second object pasted over a frame that shows the first
        rgb, depth = ST.compose_frame(bg[f % len(bg)], seqs[0].patches[f])
        return ST.compose_frame((rgb, depth), seqs[1].patches[f])

    solo = [make_tracker(se3, models, name, mesh, ST.OBJECT_WIDTH_MM) for name, _, _, mesh in regimes]
    together = [make_tracker(se3, models, name, mesh, ST.OBJECT_WIDTH_MM) for name, _, _, mesh in regimes]
    mt = se3.MultiTracker(together)
    P0 = [ST.gt_pose(seed, 0, reg) for _, reg, seed, _ in regimes]
    P_solo = [p.copy() for p in P0]
    P_multi = [p.copy() for p in P0]
    moved = [0.0, 0.0]
    for f in range(1, frames + 1):
        rgb, depth = frame(f)
        P_solo = [t.on_track(P, rgb, depth) for t, P in zip(solo, P_solo)]
        P_multi = list(mt.on_track(np.stack(P_multi), rgb, depth))
        for k in range(2):
            assert np.array_equal(P_multi[k], P_solo[k]), (f, k)
            if f == 1:     # the loop starts with both objects in view
                assert int((mt.last_prediction["depthA"][k].cpu().numpy() != 0).sum()) > 300, k
            moved[k] = max(moved[k], float(np.abs(P_multi[k] - P0[k]).max()))
    print("closed loop: largest pose change over %d frames %s" % (frames, moved))
    assert min(moved) > 1e-3      # (the loop does move)
    mt.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_ycbv_objects_driver_writes_the_files_of_the_per_class_driver(se3, models, tmp_path):
    """get_results_ycb_objects with two frame-route trackers on a tree where sequence 0048 shows a second class: byte-identical files
    to two get_results_ycb runs"""
    import shutil
    tree = YF.make_tree(str(tmp_path / "ycbv"))
    c1, c2 = YF.CLASS_ID, YF.CLASS_ID + 1
    src = os.path.join(tree, "data_organized", "0048", "pose_gt", str(c1))
    dst = os.path.join(tree, "data_organized", "0048", "pose_gt", str(c2))
    shutil.copytree(src, dst)
    for f in sorted(os.listdir(dst)):                         # the second object sits 2 cm to the side and 3 cm further away
        P = np.loadtxt(os.path.join(dst, f))
        P[:3, 3] += (0.02, -0.01, 0.03)
        np.savetxt(os.path.join(dst, f), P)
    t1 = make_tracker(se3, models, "30deg", "retextured", 120.0, frame_hw=YF.FRAME_HW)
    t2 = make_tracker(se3, models, "5deg", "textured", 120.0, frame_hw=YF.FRAME_HW)
    rgbA, depthA = render_window(t1, YF.gt_pose(48, 0))
    assert (depthA > 0).sum() > 300                           # the tree's poses show the object
    d = {c: str(tmp_path / ("multi%d" % c)) for c in (c1, c2)}
    done = se3.sequence.get_results_ycb_objects({c1: t1, c2: t2}, tree, d)
    e1, e2 = str(tmp_path / "one1"), str(tmp_path / "one2")
    assert done[c1] == se3.sequence.get_results_ycb(t1, tree, c1, e1)
    assert done[c2] == se3.sequence.get_results_ycb(t2, tree, c2, e2) == {48: 9}
    for c, e in ((c1, e1), (c2, e2)):
        for sdir in sorted(os.listdir(e)):
            names = sorted(os.listdir(os.path.join(e, sdir)))
            assert names == sorted(os.listdir(os.path.join(d[c], sdir)))
            for f in names:
                with open(os.path.join(e, sdir, f), "rb") as a, open(os.path.join(d[c], sdir, f), "rb") as b:
                    assert a.read() == b.read(), (c, sdir, f)
