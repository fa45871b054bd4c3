"""GPU: se3tn_scene_stats, se3tn_scene_fit / _host and MultiTracker.scene_check.  The kernel is held to utils.scene_stats (which
tests/test_scene_fit_host.py holds to a per-pixel loop) on the synthetic layer sets of tests/scene_fit_scene.py; the rendering entries
to the oracle's renders cut to se3tn_frame_rect's rectangles; the tracker's property to a tracker that never had it.  Everything is
integers or bits: every comparison is an equality.  Small frames (40 x 56 and 120 x 160) except the one case that can only show at
2^21 pixels.  Without the feature every test fails: the names do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_fit_scene as SS
from mapped_memory import Mapped   # noqa: F401  (tests/test_gpu_scene_search.py imports it from here)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, max_batch=32)
    yield e
    e.close()


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def run_stats(se3, eng, c, **kw):
    layers = [None if l is None else dev16(l) for l in c["layers"]]
    return eng.scene_stats(layers, c["rects"], dev16(c["observed"]), c["tol"], **kw)


@pytest.mark.parametrize("name", sorted(SS.cases()))
def test_scene_stats_equals_the_numpy_rule(se3, eng, name):
    c = SS.cases()[name]
    want, ids_w, scene_w = se3.utils.scene_stats(c["layers"], c["rects"], c["observed"], c["tol"])
    n = len(want)
    # records in device memory, ids and scene asked for: the tiles cover the whole frame
    rec, ids, scene = run_stats(se3, eng, c)
    assert np.array_equal(rec, want), (name, rec, want)
    assert np.array_equal(ids, ids_w) and np.array_equal(scene, scene_w), name
    # again on the same context (the counters were re-armed), records in mapped pinned memory, ids and scene NULL: the tiles cover
    # the bounding box of the rectangles only
    m = Mapped(48 * n)
    try:
        none, i2, s2 = run_stats(se3, eng, c, ids=False, scene=False, out=m.d.value)
        torch.cuda.synchronize()
        assert none is None and i2 is None and s2 is None
        assert np.array_equal(m.read().view(se3._lib.SCENE_FIT_DTYPE), want), (name, "mapped")
    finally:
        m.close()
    # and a third time, ids alone
    rec3, ids3, s3 = run_stats(se3, eng, c, scene=False)
    assert np.array_equal(rec3, want) and np.array_equal(ids3, ids_w) and s3 is None


def test_scene_stats_fills_a_word_to_the_brim_at_2_21_pixels(se3, eng):
    """2048 x 1024 = 2^21 pixels, one full-frame layer at 101 mm, the observed frame at 1999 mm, tol 1898: every pixel is an inlier
    1898 mm off, sum_abs_mm = 2^21 x 1898 = 3,980,394,496 -- no wrap.  One more row is refused."""
    H, W = 2048, 1024
    layer = torch.full((H, W), 101, dtype=torch.int16, device="cuda")
    obs = torch.full((H, W), 1999, dtype=torch.int16, device="cuda")
    rec, ids, scene = eng.scene_stats([layer], [(0, 0, W, H)], obs, 1898)
    px = H * W
    want = np.zeros(1, se3._lib.SCENE_FIT_DTYPE)
    for k, v in dict(model_px=px, visible_px=px, seen_px=px, inlier_px=px, sum_abs_mm=px * 1898, tol_mm=1898, n_objects=1).items():
        want[k] = v
    assert px * 1898 == 3980394496 and np.array_equal(rec, want), rec
    assert (ids == 1).all() and (scene == 101).all()
    big = torch.zeros((H + 1, W), dtype=torch.int16, device="cuda")
    with pytest.raises(se3._lib.Se3tnError, match="2\\^21"):
        eng.scene_stats([layer], [(0, 0, W, H)], big, 10)
    rec2 = eng.scene_stats([layer], [(0, 0, W, H)], obs, 1898, ids=False, scene=False)[0]       # the context is usable after a refusal
    assert np.array_equal(rec2, want)


# ---- render + kernel ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(se3):
    """three objects on two meshes in the occlusion scene: the slab at A, the block at B, the slab at C"""
    meshes = [SS.slab_mesh(), SS.block_mesh(), SS.slab_mesh()]
    poses = SS.scene_poses()
    widths = [SS.OBJECT_WIDTH_MM] * 3
    layers, rects = SS.oracle_layers(se3, meshes, poses, widths)
    scene = se3.utils.scene_stats(layers, rects, np.zeros(SS.HW, np.uint16), SS.TOL)[2]
    return dict(meshes=meshes, poses=poses, widths=widths, layers=layers, rects=rects, observed=SS.observe(scene))


@pytest.fixture(scope="module")
def renderers(se3):
    """an engine of its own with the two meshes on BOTH routes: window route without a material, frame route with a texture"""
    e = se3.Engine(0, max_batch=8)
    rng = np.random.default_rng(5)
    out = {}
    for name, mesh in (("slab", SS.slab_mesh()), ("block", SS.block_mesh())):
        textured = dict(mesh, uv=rng.random((len(mesh["vertices"]), 2)), texture=rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))
        out[name] = (se3.HipRenderer(e, mesh), se3.HipRenderer(e, textured, mode="pyrender", frame_size=SS.HW))
    assert out["slab"][0].full_frame is False and out["slab"][1].full_frame is True
    yield e, out
    e.close()


def test_scene_fit_equals_the_oracle_renders_through_the_numpy_rule(se3, world, renderers):
    e, r = renderers
    U = se3.utils
    want, ids_w, scene_w = U.scene_stats(world["layers"], world["rects"], world["observed"], SS.TOL)
    assert int(want["hidden_px"][1]) > 200 and int(want["hidden_by"][1]) == 1 and int(want["visible_px"][1]) > 200      # B stands behind A
    # window-route meshes without a material and frame-route meshes with a texture in ONE call, through the host entry
    objs = [(r["slab"][0], 150.0), (r["block"][1], 150.0), (r["slab"][1], 150.0)]
    rec, ids, scene = e.scene_fit(objs, world["poses"], world["observed"], SS.K, tol_mm=SS.TOL, ids=True, scene=True)
    assert np.array_equal(rec, want), (rec, want)
    assert ids.dtype == np.uint8 and np.array_equal(ids, ids_w) and np.array_equal(scene, scene_w)
    # the device entry: the same, and no image asked for
    rec_d, ids_d, scene_d = e.scene_fit(objs, world["poses"], dev16(world["observed"]), SS.K, tol_mm=SS.TOL, ids=True, scene=True)
    assert np.array_equal(rec_d, want) and np.array_equal(ids_d.cpu().numpy(), ids_w)
    assert np.array_equal(scene_d.cpu().numpy().view(np.uint16), scene_w)
    rec_n, i_n, s_n = e.scene_fit(objs, world["poses"], dev16(world["observed"]), SS.K, tol_mm=SS.TOL)
    assert np.array_equal(rec_n, want) and i_n is None and s_n is None
    # the other route of every mesh: the same depth layers
    other = [(r["slab"][1], 150.0), (r["block"][0], 150.0), (r["slab"][0], 150.0)]
    assert np.array_equal(e.scene_fit(other, world["poses"], world["observed"], SS.K, tol_mm=SS.TOL)[0], want)
    # the order of the objects permuted
    perm = [2, 0, 1]
    want_p, ids_p, _ = U.scene_stats([world["layers"][j] for j in perm], [world["rects"][j] for j in perm], world["observed"], SS.TOL)
    rec_p, ids_got, _ = e.scene_fit([objs[j] for j in perm], world["poses"][perm], world["observed"], SS.K, tol_mm=SS.TOL, ids=True)
    assert np.array_equal(rec_p, want_p) and np.array_equal(ids_got, ids_p)
    # an object_width_mm too small for B: its rectangle cuts its render, and the model is rendered inside the rectangle only
    widths = [150.0, 60.0, 150.0]
    layers_c, rects_c = SS.oracle_layers(se3, world["meshes"], world["poses"], widths)
    want_c, ids_c, _ = U.scene_stats(layers_c, rects_c, world["observed"], SS.TOL)
    assert 0 < int(want_c["model_px"][1]) < int(want["model_px"][1])
    rec_c, ids_got, _ = e.scene_fit([(o[0], w) for o, w in zip(objs, widths)], world["poses"], world["observed"], SS.K, tol_mm=SS.TOL, ids=True)
    assert np.array_equal(rec_c, want_c) and np.array_equal(ids_got, ids_c)
    # every window off the frame: zero records, zero ids, zero scene
    away = np.stack([SS.pose((-0.6, 0.0, 0.5), 140, 0), SS.pose((0.0, 0.7, 0.5), 140, 0), SS.pose((0.9, -0.7, 0.6), 150, 10)])
    for depth in (world["observed"], dev16(world["observed"])):
        rec_a, ids_a, scene_a = e.scene_fit(objs, away, depth, SS.K, tol_mm=SS.TOL, ids=True, scene=True)
        zero = np.zeros(3, se3._lib.SCENE_FIT_DTYPE)
        zero["tol_mm"], zero["n_objects"] = SS.TOL, 3
        assert np.array_equal(rec_a, zero)
        assert not np.asarray(ids_a.cpu() if torch.is_tensor(ids_a) else ids_a).any()
        assert not np.asarray(scene_a.cpu() if torch.is_tensor(scene_a) else scene_a).any()
    # refusals leave the context usable: a pose behind the camera, a pose that is not finite, too many rows
    bad = world["poses"].copy(); bad[1, 2, 3] = -0.5
    nan = world["poses"].copy(); nan[2, 0, 0] = np.nan
    for p in (bad, nan):
        with pytest.raises(se3._lib.Se3tnError):
            e.scene_fit(objs, p, world["observed"], SS.K, tol_mm=SS.TOL)
        with pytest.raises(se3._lib.Se3tnError):
            e.scene_fit(objs, p, dev16(world["observed"]), SS.K, tol_mm=SS.TOL)
    with pytest.raises(se3._lib.Se3tnError, match="2048"):
        e.scene_fit(objs[:1], world["poses"][:1], np.zeros((2049, 8), np.uint16), SS.K, tol_mm=SS.TOL)
    assert np.array_equal(e.scene_fit(objs, world["poses"], world["observed"], SS.K, tol_mm=SS.TOL)[0], want)


# ---- MultiTracker.scene_check ---------------------------------------------------------------------------------------------------------
KEYS = ("pose", "trans", "rot", "bbox", "rgbA", "depthA")


@pytest.fixture(scope="module")
def trackers(se3):
    a = SS.make_tracker(se3, SS.slab_mesh(), 150.0, seed=0)
    b = SS.make_tracker(se3, SS.block_mesh(), 150.0, seed=1)
    return [a, b, a]                                                       # (a model may appear several times)


def snapshot(mt, out):
    lp = mt.last_prediction
    s = dict(pose=out.copy(), trans=lp["trans"].copy(), rot=lp["rot"].copy(), bbox=np.asarray(lp["bbox"]).copy(),
             rgbA=torch.stack(list(lp["rgbA"])).cpu().numpy(), depthA=torch.stack(list(lp["depthA"])).cpu().numpy())
    if "fit" in lp:
        s.update(fit=lp["fit"].copy(), pred_rgb=lp["pred_rgb"].cpu().numpy().copy(), pred_depth=lp["pred_depth"].cpu().numpy().copy())
    return s


def same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_multitracker_scene_check(se3, world, trackers):
    U = se3.utils
    rng = np.random.default_rng(9)
    rgb = rng.integers(0, 256, SS.HW + (3,), dtype=np.uint8)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    depth = world["observed"]                                              # holes included: also the live camera's raw frame
    poses = world["poses"]

    def run(mt, live):
        out = mt.on_track_live(poses, bgr, depth, bgr=True) if live else mt.on_track(poses, rgb, depth)
        return snapshot(mt, out)
    never = se3.MultiTracker(trackers)
    mt = se3.MultiTracker(trackers)
    assert never.scene_check is None and mt.scene_check is None
    ref = {live: run(never, live) for live in (False, True)}
    # set and taken back: the bits of a tracker that never had the property, and nothing of the scene in last_prediction
    mt.scene_check = SS.TOL
    mt.scene_check = None
    for live in (False, True):
        same(run(mt, live), ref[live], ("off", live))
        assert "scene_fit" not in mt.last_prediction and "ids" not in mt.last_prediction
        assert mt.last_scene_ratio is None and mt.last_visible_share is None
    # on: poses, trans, rot, bbox and image A unchanged bit for bit; the records are those of a direct call at the returned poses
    mt.scene_check = SS.TOL
    filled = mt.engine.fill_depth(depth, 2.0, False, "bilateral")
    for live in (False, True):
        for want_ids in (False, True):
            mt.scene_ids = want_ids
            got = run(mt, live)
            same(got, ref[live], ("on", live))
            lp = mt.last_prediction
            direct, ids_direct = mt.scene_fit(got["pose"], filled if live else depth, tol_mm=SS.TOL, ids=True)
            assert lp["scene_fit"].dtype == se3._lib.SCENE_FIT_DTYPE and np.array_equal(lp["scene_fit"], direct), (live, lp["scene_fit"], direct)
            assert int(direct["model_px"][0]) > 1000 and int(direct["hidden_px"][1]) > 100                 # (not vacuous)
            assert ("ids" in lp) == want_ids
            if want_ids:
                ids = lp["ids"]
                assert np.array_equal(ids.cpu().numpy() if torch.is_tensor(ids) else ids, ids_direct)
            assert np.array_equal(mt.last_scene_ratio, U.scene_ratio(direct), equal_nan=True)
            assert np.array_equal(mt.last_visible_share, U.visible_share(direct), equal_nan=True)
    mt.scene_ids = False
    # a caller's own depth_filled on the live path still receives the filled frame
    mine = torch.zeros(SS.HW, dtype=torch.int16, device="cuda")
    out = mt.on_track_live(poses, bgr, depth, bgr=True, depth_filled=mine)
    assert np.array_equal(out, ref[True]["pose"]) and np.array_equal(mine.cpu().numpy().view(np.uint16), filled)
    # fit_check and scene_check together: last_fit and the estimate renders as with scene_check off; a scene call between the tracking
    # call and se3tn_last_fit / se3tn_last_fit_images changes nothing of what they return
    never.fit_check = mt.fit_check = SS.TOL
    for live in (False, True):
        want, got = run(never, live), run(mt, live)
        assert "fit" in want
        same(got, want, ("fit + scene", live))
        mt.scene_fit(got["pose"], depth, tol_mm=3, ids=True)
        assert np.array_equal(mt.engine.last_fit(mt.n), want["fit"])
        pr, pd = mt.engine.last_fit_images(mt.n)
        assert np.array_equal(pr.cpu().numpy(), want["pred_rgb"]) and np.array_equal(pd.cpu().numpy(), want["pred_depth"])
    never.fit_check = mt.fit_check = None
    # a tracking call after all these scene calls: the bits of a fresh tracker
    mt.scene_check = None
    fresh = se3.MultiTracker(trackers)
    for live in (False, True):
        same(run(mt, live), run(fresh, live), ("fresh", live))
        same(run(mt, live), ref[live], ("ref", live))
    # the live front end passes the property on and reads the status
    lmt = se3.LiveMultiTracker(mt, poses, one_call=True)
    assert lmt.scene_check is None and lmt.scene_status() is None
    lmt.scene_check = SS.TOL
    lmt.grab_depth(depth)
    lmt.grab_color(bgr, stamp=1.0)
    assert len(lmt.on_track()) == 3
    status = lmt.scene_status(lost_below=0.5, min_visible=0.2)
    assert status == U.scene_status(mt.last_prediction["scene_fit"], 0.5, 0.2) and set(status) <= {"tracked", "lost", "occluded"}
    assert mt.scene_check == SS.TOL and len(lmt.last_scene_ratio) == 3
    for t in (never, mt, fresh):
        t.close()
