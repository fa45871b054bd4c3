"""GPU: the full-frame rasteriser (csrc/raster.hip, mode 1, with its scissored and per-instance forms) against the statement of the GL
rules (oracle/ss_rules.py) at LARGE frames -- byte equality.  The other frame tests stop at 480 rows, where every float32 product of a
triangle's set-up is still (all but) exact, no row of the clip path's span tables beyond 479 is touched and no rectangle lies farther than
640 columns from the origin.  Here: 1080 x 1920 (the size include/se3tracknet.h names), 2048 x 1024 (the row limit and the 2^21-pixel
limit at once) and 2048 x 96, on the frame soup (triangles across every frame edge and the near plane: the clip path over all 2048 rows)
and the sliver soup (long thin triangles inside the frustum, whose float area, D, depth planes and varying matrix are inexact on most of
them).  tests/test_raster_large_frames_oracle.py proves on the CPU that the soups reach all that and holds the rules to the live GL
library on them, colours included.  The oracle renders are computed once per module; each case is one or two launches and a read-back."""
import numpy as np
import pytest

import scene_fit_scene as SS
from oracle import fixtures as Fx
from oracle import ss_rules as S
from test_gpu_raster_soups import assert_equal_images, vertex_colour_model

pytestmark = pytest.mark.gpu
f32 = np.float32
SOUPS = ("frame", "slivers")
BIG_TWO = Fx.LARGE_FRAMES[:2]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, max_batch=4)
    yield e
    e.close()


def soup_of(soup, hw):
    return Fx.soup_frame() if soup == "frame" else Fx.soup_slivers(hw)


_oracle = {}


def oracle_frame(soup, hw):
    """the rules' render of the soup at hw, vertex colours: (mesh, rgb uint8 [H,W,3], depth uint16 [H,W]); computed once, read-only"""
    if (soup, hw) not in _oracle:
        m = soup_of(soup, hw)
        rgb, depth = S.render_frame(m["vertices"], (m["colors"] / 255.0).astype(f32), m["faces"], Fx.soup_frame_pose(), Fx.large_frame_K(hw),
                                    hw[1], hw[0], kd=m["kd"])
        rgb.setflags(write=False); depth.setflags(write=False)
        _oracle[(soup, hw)] = (m, rgb, depth)
    return _oracle[(soup, hw)]


_renderers = {}


def renderer_of(se3, eng, soup, hw):
    if (soup, hw) not in _renderers:
        _renderers[(soup, hw)] = se3.HipRenderer(eng, vertex_colour_model(soup_of(soup, hw)), mode="pyrender", frame_size=hw)
    return _renderers[(soup, hw)]


# ---- a. whole frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soup", SOUPS)
@pytest.mark.parametrize("hw", Fx.LARGE_FRAMES)
def test_whole_large_frame_equals_the_rules(se3, eng, soup, hw):
    H, W = hw
    m, want_rgb, want_d = oracle_frame(soup, hw)
    ren = renderer_of(se3, eng, soup, hw)
    P, K = Fx.soup_frame_pose(), Fx.large_frame_K(hw)
    rgb, depth = ren.render_frame(P, K)
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W) and depth.dtype == np.uint16
    print("%s %d x %d: %d pixels covered in the rules' render" % (soup, H, W, (want_d > 0).sum()))
    assert (want_d > 0).sum() > 100000
    assert_equal_images(rgb, depth, want_rgb, want_d, "%s, whole frame %d x %d" % (soup, H, W))
    assert (rgb[want_d == 0] == 0).all() and (depth[want_d == 0] == 0).all()              # the background is exactly 0
    rgb2, depth2 = ren.render_frame(P, K)                                                   # the order of the atomics does not matter
    assert np.array_equal(rgb2, rgb) and np.array_equal(depth2, depth)


# ---- b. rectangles far from the origin ------------------------------------------------------------------------------------------------
def rectangles(hw):
    H, W = hw
    r = [("top left corner", (0, 0, 97, 61)), ("top right corner", (W - 97, 0, W, 61)), ("bottom left corner", (0, H - 61, 97, H)),
         ("bottom right corner", (W - 97, H - 61, W, H)), ("the last column", (W - 1, 0, W, H)), ("the last row", (0, H - 1, W, H)),
         ("whole frame", (0, 0, W, H))]
    if H == 2048:        # the image's rows 2040 .. 2047, and the span tables' (GL rows count bottom-up: the image's first eight)
        r += [("rows 2040 to 2048", (0, 2040, W, 2048)), ("GL rows 2040 to 2048", (0, 0, W, 8))]
    return r


@pytest.mark.parametrize("soup", SOUPS)
@pytest.mark.parametrize("hw", BIG_TWO)
def test_large_frame_rectangles_equal_the_slices_of_the_rules_render(se3, eng, soup, hw):
    """The frame soup reaches every border; the sliver soup keeps 2 pixels from it (it stays inside the frustum), so its last column and
    last row hold nothing: there the rectangle must come back as zeros, and the 30-pixel condition applies to the others."""
    m, want_rgb, want_d = oracle_frame(soup, hw)
    ren = renderer_of(se3, eng, soup, hw)
    P, K = Fx.soup_frame_pose(), Fx.large_frame_K(hw)
    for name, (x0, y0, x1, y1) in rectangles(hw):
        rgb, depth = ren.render_frame_rect(P, K, (x0, y0, x1, y1))
        covered = int((want_d[y0:y1, x0:x1] > 0).sum())
        print("%s %s, rect %s %s: %d covered pixels" % (soup, hw, name, (x0, y0, x1, y1), covered))
        assert rgb.shape == (y1 - y0, x1 - x0, 3), name
        if soup == "frame" or name not in ("the last column", "the last row"):
            assert covered > 30, name
        assert np.array_equal(depth, want_d[y0:y1, x0:x1]) and np.array_equal(rgb, want_rgb[y0:y1, x0:x1]), (soup, hw, name)


# ---- c. the per-instance scissor path of the scene stage ------------------------------------------------------------------------------
SCENE_HW = (1080, 1920)
SCENE_TOL = 10
SCENE_WIDTHS = [200.0, 120.0, 150.0]           # the frame soup's window leaves the frame on every side, the slivers' at the top


def scene_world(se3):
    """three objects at 1080 x 1920: the frame soup and the sliver soup under soup_frame_pose(), an icosphere whose window the right and
    the bottom edge cut.  The observed frame is synthetic: the composed scene +- 14 mm of uniform integer noise (more than the
    tolerance: inliers, front and behind all occur) over a wall at 1700 mm, with 5 % holes."""
    H, W = SCENE_HW
    K = Fx.large_frame_K(SCENE_HW)
    ball = Fx.icosphere(2, 0.05, 7)
    meshes = [vertex_colour_model(soup_of("frame", SCENE_HW)), vertex_colour_model(soup_of("slivers", SCENE_HW)),
              dict(ball, colors=ball["colors"].astype(np.uint8), vertices=ball["vertices"].astype(np.float32))]
    poses = np.stack([Fx.soup_frame_pose(), Fx.soup_frame_pose(), Fx.pose(11, (0.10, 0.09, 0.45))])
    layers, rects = SS.oracle_layers(se3, meshes, poses, SCENE_WIDTHS, hw=SCENE_HW, k=K)
    scene = se3.utils.scene_stats(layers, rects, np.zeros(SCENE_HW, np.uint16), SCENE_TOL)[2]
    rng = np.random.default_rng(21)
    s = scene.astype(np.int64)
    obs = np.where(s > 0, s + rng.integers(-14, 15, s.shape), 1700)
    obs[rng.random(obs.shape) < 0.05] = 0
    return dict(K=K, meshes=meshes, poses=poses, layers=layers, rects=rects, observed=obs.astype(np.uint16))


def test_scene_fit_at_1080_x_1920_equals_the_oracle_renders_through_the_numpy_rule(se3, eng):
    H, W = SCENE_HW
    w = scene_world(se3)
    want, ids_w, scene_w = se3.utils.scene_stats(w["layers"], w["rects"], w["observed"], SCENE_TOL)
    print("rectangles %s\nrecords %s" % (w["rects"], want))
    # on the oracle alone: one window cut by the right edge, one by the bottom edge, and every count of every object is alive
    assert any(r[2] == W and r[0] > 0 for r in w["rects"]) and any(r[3] == H and r[1] > 0 for r in w["rects"])
    for k in ("visible_px", "hidden_px", "inlier_px", "front_px", "behind_px"):
        assert (want[k] > 100).all(), (k, want[k])
    # layers of the whole frame agree with the whole-frame oracle of the other tests (one oracle, two ways to it)
    x0, y0, x1, y1 = w["rects"][1]
    assert np.array_equal(w["layers"][1], oracle_frame("slivers", SCENE_HW)[2][y0:y1, x0:x1])
    rens = [se3.HipRenderer(eng, m, mode="pyrender", frame_size=SCENE_HW) for m in w["meshes"]]
    objs = [(r, wd) for r, wd in zip(rens, SCENE_WIDTHS)]
    rec, ids, scene = eng.scene_fit(objs, w["poses"], w["observed"], w["K"], tol_mm=SCENE_TOL, ids=True, scene=True)       # the host entry
    assert np.array_equal(scene, scene_w), "scene: %d pixels differ" % (scene != scene_w).sum()
    assert ids.dtype == np.uint8 and np.array_equal(ids, ids_w)
    assert np.array_equal(rec, want), (rec, want)
