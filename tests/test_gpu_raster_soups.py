"""GPU: the HIP rasteriser (csrc/raster.hip) against the statement of the GL rules (oracle/ss_rules.py) on the triangle soups of
oracle/fixtures.py -- byte equality.  Every other comparison of the rasteriser renders a sphere: closed, convex, consistently wound,
well conditioned.  The soups bring what a sphere never does: two triangles with the same depth at a pixel (the (z | triangle id) key
decides), pixel centres exactly on edges and vertices (edges_inside / tie[], the ceiling of the clip path's span walk), w <= 0 (the
sign-xor of tri_load, clip_edge / plane_exact), the far plane, polygons cut by up to six planes, both windings, zero-area / collinear /
sub-pixel triangles and slivers, equal w (rotate_max_w).  tests/test_raster_soups_oracle.py proves on the CPU that each family reaches
the path it names and holds the rules to the live GL library on these very soups.

Three routes: the 176 x 176 window (both depth-offset rules, both sub-pixel rules), the full frame (clip path with a non-square frame
and flipped rows; vertex colours exact, texture by the bound tests/test_renderer.py holds the pair to; scissor rectangles), and the
batched launches (blockIdx.y = instance: poses of one mesh, and meshes of different sizes)."""
import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import se3_oracle as O
from oracle import ss_rules as S

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [(fam, i) for fam in Fx.SOUP_FAMILIES for i in range(len(Fx.soup_poses(fam)))]
RULE_CASES = [(fam, i) for fam, i in CASES if fam in ("lattice", "ties", "near")]
H, W = Fx.SOUP_FRAME_HW


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    return se3.Engine(0, 1)


@pytest.fixture(scope="module")
def eng2(se3):
    """a second engine for the tests that select another rule (and put the default back)"""
    return se3.Engine(0, 1)


def soup_args(m):
    """what HipRenderer makes of the mesh dict: float32 normals normalised in float32, colours / 255"""
    nrm = m["normals"] / np.linalg.norm(m["normals"], axis=1).reshape(-1, 1)
    return m["vertices"], nrm.astype(f32), (m["colors"].astype(np.float64) / 255.0).astype(f32), m["faces"]


_oracle = {}


def oracle_window(key, m, P, sub_bits=4):
    """the rules' render of mesh m under P (computed once per module): rgb, depth under both offset rules, owner map"""
    key = (key, sub_bits)
    if key not in _oracle:
        win = Fx.gl_window(P, Fx.K_YCB, Fx.SOUP_WIDTH)
        rgb, d1, _, zbuf, owner = S.render_vispy(*soup_args(m), P, Fx.K_YCB, win, return_float=True, numpy_rule="numpy1", sub_bits=sub_bits)
        _, _, _, (pA, pB) = S.vispy_uniforms(P, Fx.K_YCB, win)
        _oracle[key] = dict(win=win, rgb=rgb, numpy1=d1, numpy2=S.depth_mm(zbuf, pA, pB, "numpy2"), owner=owner)
        for v in _oracle[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _oracle[key]


def family_case(fam, i, sub_bits=4):
    m, P = Fx.soup(fam), Fx.soup_poses(fam)[i]
    return m, P, oracle_window((fam, i), m, P, sub_bits)


_renderers = {}


def renderer_of(se3, engine, fam):
    if (id(engine), fam) not in _renderers:
        _renderers[(id(engine), fam)] = se3.HipRenderer(engine, Fx.soup(fam))
    return _renderers[(id(engine), fam)]


def assert_equal_images(rgb, depth, want_rgb, want_depth, what):
    nd = int((depth != want_depth).sum())
    nc = int((rgb != want_rgb).any(2).sum())
    print("%s: depth differs on %d pixels (max %d mm), rgb on %d" % (what, nd, np.abs(depth.astype(int) - want_depth.astype(int)).max(), nc))
    assert nd == 0 and nc == 0, (what, nd, nc)


# ---- window route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,i", CASES)
def test_window_route_equals_the_rules(se3, eng, fam, i):
    """Background = the pixels no triangle owns in the rules' render (a pixel drawn at or beyond 2 m reads depth 0 with a colour, as in
    the reference: depth > 0 is not the coverage there)."""
    m, P, want = family_case(fam, i)
    ren = renderer_of(se3, eng, fam)
    win = se3.HipRenderer.gl_window(P, Fx.K_YCB, Fx.SOUP_WIDTH)
    assert tuple(win) == tuple(want["win"])
    rgb, depth = ren.render(P, Fx.K_YCB, win)
    assert rgb.shape == (176, 176, 3) and depth.dtype == np.uint16 and (want["owner"] >= 0).sum() > 3000
    assert_equal_images(rgb, depth, want["rgb"], want["numpy1"], "%s pose %d" % (fam, i))
    bg = want["owner"] < 0
    assert (rgb[bg] == 0).all() and (depth[bg] == 0).all()                                # the background is exactly 0
    rgb2, depth2 = ren.render(P, Fx.K_YCB, win)                                             # the order of the atomics does not matter
    assert np.array_equal(rgb2, rgb) and np.array_equal(depth2, depth)


@pytest.mark.parametrize("fam,i", RULE_CASES)
def test_window_route_under_the_numpy2_offset_rule(se3, eng2, fam, i):
    m, P, want = family_case(fam, i)
    try:
        eng2.set_offset_rule("numpy2")
        rgb, depth = renderer_of(se3, eng2, fam).render(P, Fx.K_YCB, want["win"])
        assert_equal_images(rgb, depth, want["rgb"], want["numpy2"], "%s pose %d numpy2" % (fam, i))
    finally:
        eng2.set_offset_rule("numpy1")


@pytest.mark.parametrize("fam,i", CASES)
def test_window_route_under_the_8_bit_subpixel_rule(se3, eng2, fam, i):
    """every family: under the finer snap the float area of most triangles of `small`, `big` and `far` is inexact
    (tests/test_raster_large_frames_oracle.py counts them)"""
    m, P, want = family_case(fam, i, sub_bits=8)
    try:
        eng2.set_raster_rule(8)
        rgb, depth = renderer_of(se3, eng2, fam).render(P, Fx.K_YCB, want["win"])
        assert (want["owner"] >= 0).sum() > 3000
        assert_equal_images(rgb, depth, want["rgb"], want["numpy1"], "%s pose %d 1/256 pixel" % (fam, i))
    finally:
        eng2.set_raster_rule(4)


# ---- full-frame route ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_oracle():
    m = Fx.soup_frame()
    rgb, depth = S.render_frame(m["vertices"], (m["colors"] / 255.0).astype(f32), m["faces"], Fx.soup_frame_pose(), Fx.SOUP_FRAME_K, W, H, kd=m["kd"])
    rgb.setflags(write=False); depth.setflags(write=False)
    return m, rgb, depth


def vertex_colour_model(m):
    return dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], normals=m["normals"], kd=m["kd"])


def test_full_frame_route_vertex_colours_equal_the_rules(se3, eng, frame_oracle):
    """The clip path with a non-square frame, flipped rows and span tables indexed by frame rows, against the rules themselves."""
    m, want_rgb, want_d = frame_oracle
    border = int((want_d[0] > 0).sum() + (want_d[-1] > 0).sum() + (want_d[:, 0] > 0).sum() + (want_d[:, -1] > 0).sum())
    print("frame soup: %d pixels covered, %d on the border, nearest %d mm" % ((want_d > 0).sum(), border, want_d[want_d > 0].min()))
    assert (want_d > 0).sum() > 10000 and border > 200 and want_d[want_d > 0].min() <= 102
    ren = se3.HipRenderer(eng, vertex_colour_model(m), mode="pyrender", frame_size=(H, W))
    rgb, depth = ren.render_frame(Fx.soup_frame_pose(), Fx.SOUP_FRAME_K)
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W) and depth.dtype == np.uint16
    assert_equal_images(rgb, depth, want_rgb, want_d, "full frame, vertex colours")
    assert (rgb[want_d == 0] == 0).all()


def test_full_frame_route_textured(se3, eng, frame_oracle):
    """The same soup with a planar texture map that leaves [0, 1] (REPEAT wraps): coverage and depth exact; colour by the bound
    tests/test_renderer.py holds this pair to (the texture FILTER is float32 arithmetic on both sides, 16-bit fixed point in the GL
    library): median <= 1, and more than 6 off on under 2 % of the covered pixels."""
    m, _, want_d = frame_oracle
    P, K = Fx.soup_frame_pose(), Fx.SOUP_FRAME_K
    assert (m["uv"] < 0).any() and (m["uv"] > 1).any()
    want_rgb, want_d2 = S.render_frame(m["vertices"], None, m["faces"], P, K, W, H, uv=m["uv"], texture=m["texture"], kd=m["kd"])
    assert np.array_equal(want_d2, want_d)
    ren = se3.HipRenderer(eng, dict(vertex_colour_model(m), uv=m["uv"], texture=m["texture"]), mode="pyrender", frame_size=(H, W))
    rgb, depth = ren.render_frame(P, K)
    assert np.array_equal(depth, want_d)                                                   # coverage and depth: every pixel
    assert (rgb[want_d == 0] == 0).all()
    d = np.abs(rgb.astype(int) - want_rgb.astype(int)).max(2)[want_d > 0]
    print("full frame, textured: colour off by max %d, median %d, share of covered pixels off by more than 6: %.4f"
          % (d.max(), np.median(d), (d > 6).mean()))
    assert np.median(d) <= 1 and (d > 6).mean() < 0.02
    assert len(np.unique(rgb[want_d > 0].reshape(-1, 3), axis=0)) > 500                   # (a texture is really sampled)
    # ... and per pixel: every byte inside the range the float64 statement of the filter admits (oracle/texture_oracle.py)
    from oracle import texture_oracle as T
    T.check(rgb, T.Expect(m["vertices"], m["faces"], m["uv"], m["texture"], m["kd"], P, K, W, H), "full frame, textured")


RECTS = [("inside", (40, 30, 121, 95)), ("across the right and bottom edges' triangles", (97, 61, 160, 120)),
         ("one pixel wide", (83, 0, 84, 120)), ("one pixel high", (0, 59, 160, 60)), ("whole frame", (0, 0, 160, 120))]


def test_full_frame_rectangles_equal_the_slices_of_the_rules_render(se3, eng, frame_oracle):
    m, want_rgb, want_d = frame_oracle
    ren = se3.HipRenderer(eng, vertex_colour_model(m), mode="pyrender", frame_size=(H, W))
    for name, (x0, y0, x1, y1) in RECTS:
        rgb, depth = ren.render_frame_rect(Fx.soup_frame_pose(), Fx.SOUP_FRAME_K, (x0, y0, x1, y1))
        covered = int((want_d[y0:y1, x0:x1] > 0).sum())
        print("rect %s %s: %d covered pixels" % (name, (x0, y0, x1, y1), covered))
        assert rgb.shape == (y1 - y0, x1 - x0, 3) and covered > 30, name
        assert np.array_equal(depth, want_d[y0:y1, x0:x1]) and np.array_equal(rgb, want_rgb[y0:y1, x0:x1]), name


# ---- batched launches: blockIdx.y is the instance -----------------------------------------------------------------------------------
def make_tracker(se3, mesh, max_samples):
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=Fx.SOUP_WIDTH), mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.002)},
                      max_samples=max_samples)
    trk.renderer = se3.HipRenderer(trk.engine, mesh)
    return trk


def test_batched_poses_of_one_soup(se3):
    """Tracker.on_track_batch (se3tn_on_track_batch: image A of all poses in four launches) with the small + big + near composite as the
    model, one of the three poses a close-up with triangles before the near plane and behind the camera: every image A equals the
    render of that pose alone and the rules' render.  (The network's output is not the subject.)"""
    m, poses = Fx.soup_composite(), Fx.soup_composite_poses()
    trk = make_tracker(se3, m, 3)
    rgb, depth = Fx.synthetic_frame(12)
    trk.on_track_batch(poses, [rgb] * 3, [depth] * 3)
    lp = trk.last_prediction
    got = [(lp["rgbA"][i].cpu().numpy().copy(), lp["depthA"][i].cpu().numpy().view(np.uint16).copy()) for i in range(3)]
    for i, P in enumerate(poses):
        want = oracle_window(("composite", i), m, P)
        assert (want["owner"] >= 0).sum() > 3000
        if i == 2:
            assert want["numpy1"][want["numpy1"] > 0].min() <= 102                         # the close-up reaches the near plane
        one_rgb, one_depth = trk.renderer.render(P, trk.K, se3.HipRenderer.gl_window(P, trk.K, Fx.SOUP_WIDTH))
        assert_equal_images(got[i][0], got[i][1], one_rgb, one_depth, "batched pose %d against the single render" % i)
        assert_equal_images(got[i][0], got[i][1], want["rgb"], want["numpy1"], "batched pose %d against the rules" % i)


def test_batched_soups_of_different_sizes(se3):
    """MultiTracker (se3tn_on_track_objects) over three trackers whose meshes are three families with different vertex and face counts
    (the launch takes the strides of the largest; the smallest comes first): the same two comparisons."""
    fams = ["big", "small", "ties"]
    trks = [make_tracker(se3, Fx.soup(f), 1) for f in fams]
    assert len({len(t.renderer.mesh["faces"]) for t in trks}) == 3
    poses = [Fx.soup_poses(f)[1] for f in fams]
    rgb, depth = Fx.synthetic_frame(12)
    mt = se3.MultiTracker(trks)
    mt.on_track(np.stack(poses), rgb, depth)
    lp = mt.last_prediction
    for i, f in enumerate(fams):
        got_rgb, got_depth = lp["rgbA"][i].cpu().numpy(), lp["depthA"][i].cpu().numpy().view(np.uint16)
        _, P, want = family_case(f, 1)
        one_rgb, one_depth = trks[i].renderer.render(P, trks[i].K, want["win"])
        assert_equal_images(got_rgb, got_depth, one_rgb, one_depth, "object %d (%s) against the single render" % (i, f))
        assert_equal_images(got_rgb, got_depth, want["rgb"], want["numpy1"], "object %d (%s) against the rules" % (i, f))
    mt.close()
