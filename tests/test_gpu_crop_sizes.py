"""GPU: the device's three copies of crop_bbox's NEAREST index rule, at the window sizes that decide it.

preprocess_kernel<TAB> and crop_raw_kernel (csrc/kernels_misc.hip) and crop_source() (csrc/crop_rule.h, read by fit_stats_kernel<COLOUR>) each
state  sx = min(floor(x * (1.0 / (176.0 / src))), src - 1)  in float64.  Where x * src / 176 is an exact integer the order of those
three operations decides the index, and tests/crop_rule_cases.py lists the 239 sizes up to 2000 at which another evaluation gives
another crop.  Here every one of them (and every size 1..352) goes through se3tn_preprocess and se3tn_crop_raw, 40 pairs of them
through se3tn_fit_stats, and poses whose window has such a size through the five tracking entry points, whose host code derives the
descriptors (crop_pair, the staged sub-window of track_plan.h).

The yardstick is oracle/se3_oracle.py throughout (crop_bbox, normalize_depth, normalize_channels, compute_bbox; utils.fit_stats for
the records), and every comparison is exact equality.  tests/test_crop_rule_cases.py shows, on the oracle alone, that each case here
fails under each alternative evaluation that differs at its sizes."""
import numpy as np
import pytest
import torch

import crop_rule_cases as CR
from oracle import fixtures as Fx
from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

H, W = 480, 640
K = Fx.K_YCB
INFO = dict(Fx.DATASET_INFO, object_width=CR.TRACK_WIDTH_MM)


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def dev_frame():
    rgb, depth = CR.frame()
    return torch.from_numpy(rgb.copy()).cuda(), torch.from_numpy(depth.view(np.int16).copy()).cuda()


@pytest.fixture(scope="module")
def oracle_crops():
    """(case index, placement) -> O.crop_bbox's (rgb, depth) of the sweep frame: computed once, shared by the sweeps, never written"""
    rgb, depth = CR.frame()
    cache = {}

    def get(case, placement):
        key = (case.index, placement)
        if key not in cache:
            r, d = CR.oracle_crop(rgb, depth, case.windows[placement])
            r.setflags(write=False); d.setflags(write=False)
            cache[key] = (r, d)
        return cache[key]
    return get


def first_difference(got, want):
    """(channel, y, x) of the first differing word of two [4,176,176] float32 images, or None; bit patterns, not values"""
    ne = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    if len(ne) == 0:
        return None
    ne = ne[np.lexsort((ne[:, 0], ne[:, 2], ne[:, 1]))]             # by row, then column, then channel
    return int(ne[0, 0]), int(ne[0, 1]), int(ne[0, 2])


# ---- a. se3tn_preprocess ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(CR.CHUNKS))
def test_preprocess_at_every_sweep_size(se3, dev_frame, oracle_crops, k):
    cases = [(c, p) for c in CR.chunk(k) for p in CR.PLACEMENTS]
    n = len(cases)
    assert n > 2 * 64                                              # several kernel-argument blocks (CropArgs::MAX descriptors each)
    mean, std = Fx.mean_std(3)
    eng = se3.Engine(0, 1)
    eng.set_normalization(mean, std)
    rule = cases[0][0].offset_rule
    eng.set_offset_rule(rule)
    out = torch.empty((n, 176, 176, 4), device="cuda")
    eng.preprocess([dict(rgb=dev_frame[0], depth=dev_frame[1], window=c.windows[p], z_offset_mm=c.z_offset_mm, stats=c.stats)
                    for c, p in cases], out)
    got = out.cpu().numpy()
    eng.close()
    for i, (c, p) in enumerate(cases):
        assert c.offset_rule == rule
        want = CR.oracle_preprocess(*oracle_crops(c, p), c, mean, std)
        g = got[i].transpose(2, 0, 1)
        if not np.array_equal(g.view(np.uint32), want.view(np.uint32)):
            ch, y, x = first_difference(g, want)
            pytest.fail("se3tn_preprocess differs from the oracle: size %d x %d, placement %s, crop x %d, y %d, channel %d: got %r, want %r "
                        "(descriptor %d of %d, rule %s)" % (c.width, c.height, p, x, y, ch, g[ch, y, x], want[ch, y, x], i, n, rule))


# ---- b. se3tn_crop_raw ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(CR.CHUNKS))
def test_crop_raw_at_every_sweep_size(se3, dev_frame, oracle_crops, k):
    cases = [(c, p) for c in CR.chunk(k) for p in CR.PLACEMENTS]
    eng = se3.Engine(0, 1)
    outs = [eng.crop_raw(dev_frame[0], dev_frame[1], c.windows[p], device=True) for c, p in cases]
    rgbs = torch.stack([o[0] for o in outs]).cpu().numpy()
    deps = torch.stack([o[1] for o in outs]).cpu().numpy().view(np.uint16)
    eng.close()
    for i, (c, p) in enumerate(cases):
        want_rgb, want_dep = oracle_crops(c, p)
        for what, g, w in (("rgb", rgbs[i], want_rgb), ("depth", deps[i], want_dep)):
            if not np.array_equal(g, w):
                ne = np.argwhere(g != w)[0]
                pytest.fail("se3tn_crop_raw differs from O.crop_bbox: size %d x %d, placement %s, %s at crop x %d, y %d: got %r, want %r"
                            % (c.width, c.height, p, what, ne[1], ne[0], g[tuple(ne)], w[tuple(ne)]))


# ---- c. se3tn_fit_stats -----------------------------------------------------------------------------------------------------------
def test_fit_stats_between_descriptors_of_different_decisive_sizes(se3):
    cases = CR.fit_cases()
    n = len(cases)
    assert n == CR.FIT_PAIRS > se3._lib.FIT_MAX_PAIRS              # more than one launch
    model, observed = (torch.from_numpy(d.view(np.int16).copy()).cuda() for d in CR.fit_frames())
    eng = se3.Engine(0, n)
    got = eng.fit_stats([dict(depth=model, window=mw) for _, mw, _ in cases], [dict(depth=observed, window=ow) for _, _, ow in cases],
                        CR.FIT_TOL)
    eng.close()
    assert got.dtype == se3._lib.FIT_DTYPE and got.shape == (n,)
    for i, (name, mw, ow) in enumerate(cases):
        want = CR.fit_expected(se3, name)
        assert got[i] == want, (name, mw, ow, got[i], want)


# ---- d. the tracking entry points -------------------------------------------------------------------------------------------------
TRACK = CR.track_cases()
TRACK_IDS = [t[0] for t in TRACK]
GROUPS = [(0, 3, 8), (1, 4, 7), (2, 5, 6)]                        # three cases of different sizes per call; every case once


@pytest.fixture(scope="module")
def poses():
    return {name: CR.find_pose(size, K, centre) for name, size, centre in TRACK}


@pytest.fixture(scope="module")
def frames():
    return [Fx.synthetic_frame(140 + i) for i in range(3)]


def _tracker(se3, seed, max_samples=1, frame_route=False):
    mean, std = Fx.mean_std(seed)
    info = dict(INFO, renderer="pyrenderer") if frame_route else INFO
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(seed, head_gain=0.01)}, max_samples=max_samples)
    if frame_route:
        m = Fx.textured_sphere(2, 0.05)
        trk.renderer = se3.HipRenderer(trk.engine, dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], uv=m["uv"],
                                                        texture=m["texture"], kd=m["kd"]), mode="pyrender", frame_size=(H, W))
    else:
        trk.renderer = se3.HipRenderer(trk.engine, Fx.icosphere(2, 0.05, 1))
    assert trk.one_call and bool(trk.renderer.full_frame) == frame_route
    return trk


@pytest.fixture(scope="module")
def window_trackers(se3):
    """three window-route trackers with their own weights, mean and std"""
    return [_tracker(se3, s) for s in (0, 3, 5)]


@pytest.fixture(scope="module")
def batch_tracker(se3):
    return _tracker(se3, 1, max_samples=3)


@pytest.fixture(scope="module")
def frame_tracker(se3):
    return _tracker(se3, 4, frame_route=True)


def expected_input(rgb, depth, P, mean, std, stats, rule, size=None):
    """the oracle's pre-processing of a frame under the window of pose P: float32 [4,176,176]"""
    bb = O.compute_bbox(P, K, CR.TRACK_WIDTH_MM, (1000, 1000, 1000))
    if size is not None:
        l, t, r, b = CR.window_of(P, K)
        assert (r - l, b - t) == (size, size)
    rgbc, depc = O.crop_bbox(rgb, depth, bb, (176, 176))
    d = O.normalize_depth(depc, P, rule)
    return O.normalize_channels(rgbc.astype(np.float32), d, mean[4 * stats:4 * stats + 4], std[4 * stats:4 * stats + 4])


def assert_input(eng, which, n, wants, what):
    """the first n images of the context's padded network input `which`: interiors equal wants bit for bit, 3-pixel borders zero"""
    buf = eng.debug_buffer(which, n).cpu().numpy()
    assert buf.shape == (n, 182, 182, 4)
    for i, want in enumerate(wants):
        g = buf[i, 3:-3, 3:-3].transpose(2, 0, 1)
        if not np.array_equal(g.view(np.uint32), want.view(np.uint32)):
            ch, y, x = first_difference(g, want)
            pytest.fail("%s of %s, image %d: differs from the oracle at crop x %d, y %d, channel %d: got %r, want %r"
                        % (which, what, i, x, y, ch, g[ch, y, x], want[ch, y, x]))
    border = buf.copy()
    border[:, 3:-3, 3:-3] = 0
    assert not border.view(np.uint32).any(), (which, what)


@pytest.mark.parametrize("name,size,centre", TRACK, ids=TRACK_IDS)
def test_on_track_window_route(se3, window_trackers, poses, frames, name, size, centre):
    trk = window_trackers[0]
    rgb, depth = frames[0]
    P = poses[name]
    out = trk.on_track(P, rgb, depth)
    assert np.isfinite(out).all()
    assert CR.window_of(P, K) == se3.crop_window(np.asarray(trk.last_prediction["bbox"]).reshape(4, 2))
    assert_input(trk.engine, "inB", 1, [expected_input(rgb, depth, P, trk.mean, trk.std, 1, "numpy1", size)], name)


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(TRACK_IDS[i] for i in g) for g in GROUPS])
def test_on_track_batch_of_three_sizes(se3, batch_tracker, poses, frames, group):
    trk = batch_tracker
    cases = [TRACK[i] for i in group]
    assert len({c[1] for c in cases}) == 3
    Ps = [poses[c[0]] for c in cases]
    out = trk.on_track_batch(Ps, [f[0] for f in frames], [f[1] for f in frames])
    assert out.shape == (3, 4, 4) and np.isfinite(out).all()
    wants = [expected_input(frames[i][0], frames[i][1], Ps[i], trk.mean, trk.std, 1, "numpy1", cases[i][1]) for i in range(3)]
    assert_input(trk.engine, "inB", 3, wants, [c[0] for c in cases])


@pytest.mark.parametrize("rule", ["numpy1", "numpy2"])
@pytest.mark.parametrize("group", GROUPS, ids=["-".join(TRACK_IDS[i] for i in g) for g in GROUPS])
def test_multi_tracker_three_objects(se3, window_trackers, poses, frames, group, rule):
    """se3tn_on_track_objects: mean / std per crop from the device table (preprocess_kernel<true>); the inputs of all objects lie in
    the EXECUTING context (the MultiTracker's engine)"""
    cases = [TRACK[i] for i in group]
    Ps = [poses[c[0]] for c in cases]
    rgb, depth = frames[1]
    for t in window_trackers:
        t.engine.set_offset_rule(rule)
    mt = se3.MultiTracker(window_trackers)
    try:
        out = mt.on_track(np.stack(Ps), rgb, depth)
        assert out.shape == (3, 4, 4) and np.isfinite(out).all()
        wants = [expected_input(rgb, depth, Ps[i], t.mean, t.std, 1, rule, cases[i][1]) for i, t in enumerate(window_trackers)]
        assert not np.array_equal(wants[0], expected_input(rgb, depth, Ps[0], window_trackers[1].mean, window_trackers[1].std, 1, rule))
        assert_input(mt.engine, "inB", 3, wants, [c[0] for c in cases])
    finally:
        mt.close()
        for t in window_trackers:
            t.engine.set_offset_rule("numpy1")


@pytest.mark.parametrize("name,size,centre", TRACK, ids=TRACK_IDS)
def test_live_tracker_one_call(se3, window_trackers, poses, frames, name, size, centre):
    trk = window_trackers[1]
    rgb, raw = frames[2]
    assert (raw == 0).mean() > 0.03                                 # holes for fill_depth to close
    P = poses[name]
    live = se3.LiveTracker(trk, P, one_call=True)
    assert live.one_call
    live.grab_color(np.ascontiguousarray(rgb[:, :, ::-1]), stamp=1.0)
    live.grab_depth(raw)
    assert live.on_track() is not None
    filled = trk.engine.fill_depth(raw, 2.0, False, "bilateral")      # held to its own oracle by the fill tests
    assert filled.dtype == np.uint16 and not np.array_equal(filled, raw)
    assert_input(trk.engine, "inB", 1, [expected_input(rgb, filled, P, trk.mean, trk.std, 1, "numpy1", size)], name)


@pytest.mark.parametrize("name,size,centre", TRACK, ids=TRACK_IDS)
def test_on_track_frame_route(se3, frame_tracker, poses, frames, name, size, centre):
    """pyrender route: image A is itself a crop -- of the scissored full-frame render, under a shifted window"""
    trk = frame_tracker
    trk.engine.set_offset_rule("numpy2")
    rgb, depth = frames[0]
    P = poses[name]
    out = trk.on_track(P, rgb, depth)
    assert np.isfinite(out).all()
    assert_input(trk.engine, "inB", 1, [expected_input(rgb, depth, P, trk.mean, trk.std, 1, "numpy2", size)], name)
    rend_rgb, rend_depth = trk.renderer.render_frame(P, K)          # se3tn_render_frame: held to its own oracle elsewhere
    assert rend_rgb.shape == (H, W, 3) and rend_depth.dtype == np.uint16
    if size >= 144:                                                 # (nearer than the renderer's far plane: the object shows)
        l, t, r, b = CR.window_of(P, K)
        assert (rend_depth[max(t, 0):b, max(l, 0):r] > 0).sum() > 300, name
    assert_input(trk.engine, "inA", 1, [expected_input(rend_rgb, rend_depth, P, trk.mean, trk.std, 0, "numpy2", size)], name)
