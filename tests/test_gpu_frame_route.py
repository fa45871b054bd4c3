"""GPU: the full-frame (pyrender) renderer route in ONE library call per frame.

se3tn_render_frame_rect renders only a rectangle of the camera frame; se3tn_on_track / se3tn_on_track_batch with a mesh on
SE3TN_ROUTE_FRAME render the rectangle the crop window covers and crop it in the launch that crops the camera frame.  Every
comparison here is BITWISE against what the repository already pins to the pyrender oracle and the SwiftShader goldens
(tests/test_renderer.py, tests/test_gl_swiftshader.py): se3tn_render_frame and the step-by-step path of the same Tracker."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as Fx
from oracle import se3_oracle as O

E_ARG, E_STATE = -1, -2
H, W = 480, 640
INFO = dict(Fx.DATASET_INFO, object_width=150.0, renderer="pyrenderer")
# translations (YCB camera, 150 mm object width: a 229-pixel window at 0.7 m) and where their crop window lies
WINDOWS = [
    ("inside", (0.0, 0.0, 0.7)),
    ("left", (-0.18, 0.0, 0.7)),
    ("right", (0.2, 0.0, 0.7)),
    ("top", (0.0, -0.13, 0.7)),
    ("bottom", (0.0, 0.14, 0.7)),
    ("miss", (0.6, 0.5, 0.9)),
    ("larger", (0.0, 0.0, 0.3)),      # a 533-pixel window on 480 rows
]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def _model(textured, subdiv=3, radius=0.06):
    ms = Fx.textured_sphere(subdiv, radius)
    if textured:
        return dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"], uv=ms["uv"], texture=ms["texture"], kd=ms["kd"])
    return dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"], kd=(1.0, 0.9, 0.8))


def _tracker(se3, max_samples=1, textured=True, head_gain=0.01):
    sd = O.make_state_dict(0, head_gain=head_gain)
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(INFO, mean, std, {"state_dict": sd}, max_samples=max_samples)
    trk.renderer = se3.HipRenderer(trk.engine, _model(textured), mode="pyrender", frame_size=(H, W))
    assert trk.renderer.full_frame and trk.engine.lib.se3tn_mesh_get_route(trk.renderer._m) == se3._lib.ROUTE_FRAME
    return trk


def _kind(P, width=150.0):
    bb = O.compute_bbox(P, Fx.K_YCB, width, (1000, 1000, 1000))
    left, top, right, bottom = bb[:, 1].min(), bb[:, 0].min(), bb[:, 1].max(), bb[:, 0].max()
    if right <= 0 or bottom <= 0 or left >= W or top >= H:
        return "miss"
    if top < 0 and bottom > H:
        return "larger"
    return "left" if left < 0 else "right" if right > W else "top" if top < 0 else "bottom" if bottom > H else "inside"


# ---- 1. the primitive ----------------------------------------------------------------------------------------------------------
RECTS = [
    ("whole_frame", (0, 0, W, H), False),
    ("odd_origin", (201, 53, 480, 340), False),
    ("even_origin", (200, 52, 480, 340), False),
    ("odd_x_even_y", (203, 60, 411, 301), False),
    ("half_object", (337, 0, W, H), False),          # the sphere's centre projects to column 337: cut in half
    ("no_geometry", (0, 400, 100, 480), True),
]


@pytest.mark.parametrize("sub_bits", [4, 8])
@pytest.mark.parametrize("textured", [True, False], ids=["textured", "vertex_colour"])
def test_render_frame_rect_equals_the_slice_of_render_frame(se3, textured, sub_bits):
    eng = se3.Engine(0, 1)
    eng.set_raster_rule(sub_bits)
    ren = se3.HipRenderer(eng, _model(textured), mode="pyrender", frame_size=(H, W))
    P = Fx.pose(4, (0.01, -0.02, 0.45))
    full_rgb, full_depth = ren.render_frame(P, Fx.K_YCB)
    assert (full_depth > 0).sum() > 30000
    for name, (x0, y0, x1, y1), empty in RECTS:
        rgb, depth = ren.render_frame_rect(P, Fx.K_YCB, (x0, y0, x1, y1))
        assert rgb.shape == (y1 - y0, x1 - x0, 3) and depth.shape == (y1 - y0, x1 - x0) and depth.dtype == np.uint16
        covered = int((full_depth[y0:y1, x0:x1] > 0).sum())
        print("rect %-13s rule %d textured %d: covered pixels %d" % (name, sub_bits, textured, covered))
        if empty:
            assert covered == 0 and not rgb.any() and not depth.any(), name
        else:
            assert covered > 300, (name, covered)          # an empty render cannot pass
        assert np.array_equal(depth, full_depth[y0:y1, x0:x1]), name
        assert np.array_equal(rgb, full_rgb[y0:y1, x0:x1]), name
    if textured:   # the level of detail varies over the object (several mip levels in play), so a rebased quad would show
        assert len(np.unique(full_rgb[full_depth > 0].reshape(-1, 3), axis=0)) > 500
    # the clip queue: a pose whose triangles cross the near plane (z - r = 0.08 m < 0.1 m) and every border of the frame
    Pc = Fx.pose(6, (0.03, 0.02, 0.14))
    full_rgb, full_depth = ren.render_frame(Pc, Fx.K_YCB)
    assert (full_depth > 0).sum() > 100000 and (full_depth == 0).sum() > 1000     # covered up to the borders, with the near-plane hole
    for (x0, y0, x1, y1) in ((0, 0, W, H), (101, 33, 500, 400), (0, 0, 321, 77), (320, 240, W, H)):
        rgb, depth = ren.render_frame_rect(Pc, Fx.K_YCB, (x0, y0, x1, y1))
        covered = int((full_depth[y0:y1, x0:x1] > 0).sum())
        print("clip-queue pose rect %s: covered pixels %d" % ((x0, y0, x1, y1), covered))
        assert covered > 300
        assert np.array_equal(depth, full_depth[y0:y1, x0:x1]) and np.array_equal(rgb, full_rgb[y0:y1, x0:x1]), (x0, y0, x1, y1)
    eng.close()


# ---- 2. one call against step by step ------------------------------------------------------------------------------------------
def _both_paths(trk, P, rgb, depth):
    out = []
    for one_call in (True, False):
        trk.one_call = one_call
        pose = trk.on_track(P, rgb, depth)
        lp = trk.last_prediction
        rec = dict(pose=pose, trans=np.array(lp["trans"]), rot=np.array(lp["rot"]), bbox=np.array(lp["bbox"]),
                   logits=trk.engine.logits(1).cpu().numpy().copy())
        if one_call:
            rec["rgbA"] = lp["rgbA"].cpu().numpy(); rec["depthA"] = lp["depthA"].cpu().numpy().view(np.uint16)
        out.append(rec)
    trk.one_call = True
    return out


@pytest.mark.parametrize("rule", ["numpy1", "numpy2"])
@pytest.mark.parametrize("name,t", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_on_track_one_call_equals_step_by_step(se3, name, t, rule):
    trk = _tracker(se3)
    trk.engine.set_offset_rule(rule)
    rgb, depth = Fx.synthetic_frame(12)
    P = Fx.pose(3, t)
    assert _kind(P) == name            # the window lies where the case says
    got, want = _both_paths(trk, P, rgb, depth)
    for k in ("pose", "trans", "rot", "logits"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got["bbox"].reshape(4, 2), np.asarray(want["bbox"]).reshape(4, 2))
    assert np.isfinite(got["pose"]).all() and np.abs(got["logits"]).max() > 0
    rgbA, depthA = trk.render_window(P)
    rgbA = rgbA.cpu().numpy() if torch.is_tensor(rgbA) else np.asarray(rgbA)
    depthA = (depthA.cpu().numpy() if torch.is_tensor(depthA) else np.asarray(depthA)).view(np.uint16)
    assert np.array_equal(got["rgbA"], rgbA) and np.array_equal(got["depthA"], depthA), name
    covered = int((depthA > 0).sum())
    print("window %-7s rule %s: image A covers %d pixels" % (name, rule, covered))
    if name == "miss":
        assert covered == 0 and not rgbA.any()
    else:
        assert covered > 300


# ---- 3. n pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 8, 21])
def test_on_track_batch_one_call_equals_step_by_step(se3, n):
    trk = _tracker(se3, max_samples=n)
    frames = [Fx.synthetic_frame(70 + i) for i in range(4)]
    poses = [Fx.pose(3 + i, WINDOWS[i % len(WINDOWS)][1]) for i in range(n)]
    rgbs, deps = [frames[i % 4][0] for i in range(n)], [frames[i % 4][1] for i in range(n)]     # frames repeated
    assert trk.one_call
    got = trk.on_track_batch(poses, rgbs, deps)
    lp = trk.last_prediction
    g = dict(trans=lp["trans"].copy(), rot=lp["rot"].copy(), bbox=lp["bbox"].copy(), logits=trk.engine.logits(n).cpu().numpy().copy(),
             rgbA=[x.cpu().numpy() for x in lp["rgbA"]], depthA=[x.cpu().numpy() for x in lp["depthA"]])
    trk.one_call = False
    want = trk.on_track_batch(poses, rgbs, deps)
    lw = trk.last_prediction
    assert got.shape == (n, 4, 4) and np.array_equal(got, want)
    assert np.array_equal(g["trans"], lw["trans"]) and np.array_equal(g["rot"], lw["rot"]) and np.array_equal(g["bbox"], lw["bbox"])
    assert np.array_equal(g["logits"], trk.engine.logits(n).cpu().numpy())
    for i in range(n):
        assert len(g["rgbA"]) == n
        assert np.array_equal(g["rgbA"][i], lw["rgbA"][i].cpu().numpy()) and np.array_equal(g["depthA"][i], lw["depthA"][i].cpu().numpy()), i
        covered = int((g["depthA"][i] != 0).sum())
        assert (covered == 0) if _kind(poses[i]) == "miss" else (covered > 300), (i, covered)
    # per pair the single-frame call: at 1-5 pairs one kernel family that works image by image (the same bits)
    trk.one_call = True
    if n <= 5:
        for i in range(n):
            one = trk.on_track(poses[i], rgbs[i], deps[i])
            lo = trk.last_prediction
            assert np.array_equal(one, got[i]), i
            assert np.array_equal(lo["trans"][0], g["trans"][i]) and np.array_equal(lo["rot"][0], g["rot"][i]), i
            assert np.array_equal(np.asarray(lo["bbox"]).reshape(4, 2), g["bbox"][i].reshape(4, 2)), i
            assert np.array_equal(trk.engine.logits(1).cpu().numpy()[0], g["logits"][i]), i
            assert np.array_equal(lo["rgbA"].cpu().numpy(), g["rgbA"][i]) and np.array_equal(lo["depthA"].cpu().numpy(), g["depthA"][i]), i


def test_on_track_batch_when_every_window_misses_the_frame(se3):
    trk = _tracker(se3, max_samples=2)
    rgb, depth = Fx.synthetic_frame(5)
    poses = [Fx.pose(1, (0.6, 0.5, 0.9)), Fx.pose(2, (-0.7, 0.5, 0.9))]
    got = trk.on_track_batch(poses, [rgb] * 2, [depth] * 2)
    assert not any(x.cpu().numpy().any() for x in trk.last_prediction["rgbA"])
    trk.one_call = False
    assert np.array_equal(got, trk.on_track_batch(poses, [rgb] * 2, [depth] * 2))


# ---- 4. closed loop ------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_30_frames_equals_step_by_step(se3):
    trk = _tracker(se3)
    P0 = Fx.pose(3, (0.02, -0.01, 0.7))
    tracks = []
    for one_call in (True, False):
        trk.one_call = one_call
        P, seq = P0, []
        for f in range(30):
            P = trk.on_track(P, *Fx.synthetic_frame(100 + f))
            seq.append(P)
        tracks.append(np.stack(seq))
    moved = float(np.abs(tracks[0][-1] - P0).max())
    print("closed loop: pose change over 30 frames %.4g" % moved)
    for f in range(30):
        assert np.array_equal(tracks[0][f], tracks[1][f]), f
    assert moved > 1e-3


# ---- 5. capture and refusals ---------------------------------------------------------------------------------------------------
def _rect_rc(eng, ren, P, rect, rgb_t, dep_t, frame=(W, H)):
    import se3tracknet_amd as se3
    _stream_ptr = se3.engine._stream_ptr
    p = (C.c_double * 16)(*np.asarray(P, np.float64).reshape(16))
    k = (C.c_double * 9)(*Fx.K_YCB.reshape(9))
    r = (C.c_int32 * 4)(*rect)
    return eng.lib.se3tn_render_frame_rect(eng._h, ren._m, p, k, frame[0], frame[1], r, C.c_void_p(rgb_t.data_ptr()),
                                           C.c_void_p(dep_t.data_ptr()), _stream_ptr())


def test_render_frame_rect_capture_and_refusals(se3):
    P = Fx.pose(4, (0.01, -0.02, 0.45))
    rect = (150, 40, 520, 360)                                   # 370 x 320 pixels: more than the 176 x 176 keys a context starts with
    reserved, bare = se3.Engine(0, 1), se3.Engine(0, 1)
    reserved.reserve(H, W)
    ren = se3.HipRenderer(reserved, _model(True), mode="pyrender", frame_size=(H, W))
    ren_bare = se3.HipRenderer(bare, _model(True), mode="pyrender", frame_size=(H, W))
    want_rgb, want_depth = ren.render_frame_rect(P, Fx.K_YCB, rect)
    assert (want_depth > 0).sum() > 300
    rgb_t = torch.zeros((rect[3] - rect[1], rect[2] - rect[0], 3), dtype=torch.uint8, device="cuda")
    dep_t = torch.zeros((rect[3] - rect[1], rect[2] - rect[0]), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert _rect_rc(reserved, ren, P, rect, rgb_t, dep_t) == 0          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc_bare = _rect_rc(bare, ren_bare, P, rect, rgb_t, dep_t)           # un-reserved: would have to allocate
        err = bare.lib.se3tn_last_error()
        rc_res = _rect_rc(reserved, ren, P, rect, rgb_t, dep_t)
    assert rc_bare == E_STATE and b"se3tn_reserve" in err
    assert rc_res == 0
    rgb_t.zero_(); dep_t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rgb_t.cpu().numpy(), want_rgb) and np.array_equal(dep_t.cpu().numpy().view(np.uint16), want_depth)
    # empty / out-of-frame rectangles, frames of more than 2048 rows
    for bad in ((100, 100, 100, 200), (100, 100, 200, 100), (200, 100, 100, 200), (-1, 0, 100, 100), (0, -1, 100, 100),
                (0, 0, W + 1, 100), (0, 0, 100, H + 1), (W, 0, W + 10, 10), (0, 0, 0, 0)):
        assert _rect_rc(reserved, ren, P, bad, rgb_t, dep_t) == E_ARG, bad
    assert _rect_rc(reserved, ren, P, (0, 0, 10, 10), rgb_t, dep_t, frame=(W, 2049)) == E_ARG
    with pytest.raises(se3._lib.Se3tnError):
        ren.render_frame_rect(P, Fx.K_YCB, (10, 10, 10, 50))
    # both contexts serve a valid call afterwards (the bare one grows its z-buffer outside a capture)
    for r in (ren, ren_bare):
        rgb, depth = r.render_frame_rect(P, Fx.K_YCB, rect)
        assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth)
    reserved.close(); bare.close()


def test_on_track_objects_refuses_a_frame_route_mesh_without_a_texture(se3):
    sd = O.make_state_dict(0, head_gain=0.01)
    mean, std = Fx.mean_std(0)
    mesh = Fx.icosphere(3, 0.05, 2)
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, {"state_dict": sd}, max_samples=1)
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    lib = trk.engine.lib
    plain = se3.HipRenderer(trk.engine, mesh)                     # vertex colours, no texture ...
    assert lib.se3tn_mesh_get_route(plain._m) == se3._lib.ROUTE_WINDOW
    assert lib.se3tn_mesh_set_route(plain._m, 7) == E_ARG and lib.se3tn_mesh_get_route(plain._m) == se3._lib.ROUTE_WINDOW
    assert lib.se3tn_mesh_set_route(plain._m, se3._lib.ROUTE_FRAME) == 0      # ... but on the full-frame route
    ctx = se3.Engine(0, 1)
    rgb, depth = Fx.synthetic_frame(12)
    P = np.ascontiguousarray(Fx.pose(3, (0.0, 0.0, 0.7)).reshape(1, 16))
    K = np.ascontiguousarray(Fx.K_YCB)
    out = np.zeros((1, 16))

    def call(mesh_handle):
        objs = (se3._lib.Object * 1)(se3._lib.Object(trk.engine._h.value, mesh_handle.value, 150.0))
        return lib.se3tn_on_track_objects(ctx._h, 1, objs, C.c_void_p(P.ctypes.data), K.ctypes.data_as(C.POINTER(C.c_double)),
                                          C.c_void_p(rgb.ctypes.data), C.c_void_p(depth.ctypes.data), H, W, None, None,
                                          C.c_void_p(out.ctypes.data), None, None, None, None)
    assert call(plain._m) == E_ARG and b"ROUTE_FRAME" in lib.se3tn_last_error()
    assert call(trk.renderer._m) == 0                             # the context serves a valid call afterwards
    assert np.array_equal(out.reshape(4, 4), trk.on_track(P.reshape(4, 4), rgb, depth))
    assert lib.se3tn_mesh_set_route(plain._m, se3._lib.ROUTE_WINDOW) == 0 and call(plain._m) == 0
    ctx.close()


# ---- 6. the default route is untouched -----------------------------------------------------------------------------------------
def test_a_textured_mesh_on_the_default_route_keeps_the_window_renderer(se3):
    sd = O.make_state_dict(0, head_gain=0.01)
    mean, std = Fx.mean_std(0)
    ms = Fx.textured_sphere(3, 0.05)
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=150.0), mean, std, {"state_dict": sd}, max_samples=3)
    trk.renderer = se3.HipRenderer(trk.engine, dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"]))
    lib, m = trk.engine.lib, trk.renderer._m
    rgb, depth = Fx.synthetic_frame(12)
    poses = [Fx.pose(3 + i, t) for i, t in enumerate([(0.0, 0.0, 0.7), (0.2, 0.0, 0.7), (0.0, 0.14, 0.6)])]
    before = [trk.on_track(P, rgb, depth) for P in poses]
    uv = np.ascontiguousarray(ms["uv"], np.float32)
    tex = np.ascontiguousarray(ms["texture"], np.uint8)
    assert lib.se3tn_mesh_set_texture(m, uv.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], None) == 0
    assert lib.se3tn_mesh_get_route(m) == se3._lib.ROUTE_WINDOW
    for i, P in enumerate(poses):
        got = trk.on_track(P, rgb, depth)                          # se3tn_on_track
        rgbA, depthA = trk.renderer.rgb.cpu().numpy(), trk.renderer.depth.cpu().numpy()
        lg = trk.engine.logits(1).cpu().numpy().copy()
        assert np.array_equal(got, before[i]), i                   # the texture changes nothing on this route
        win = se3.HipRenderer.gl_window(P, trk.K, trk.object_width)
        r2, d2 = trk.renderer.render(P, trk.K, win)                # se3tn_render
        assert np.array_equal(rgbA, r2) and np.array_equal(depthA.view(np.uint16), d2) and (d2 > 0).sum() > 300
        trk.one_call = False
        want = trk.on_track(P, rgb, depth)                         # se3tn_render + se3tn_preprocess x 2 + se3tn_infer
        trk.one_call = True
        assert np.array_equal(got, want) and np.array_equal(lg, trk.engine.logits(1).cpu().numpy()), i
    got = trk.on_track_batch(poses, [rgb] * 3, [depth] * 3)
    assert np.array_equal(got, np.stack(before))
