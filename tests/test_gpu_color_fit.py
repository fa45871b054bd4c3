"""GPU: the colour check -- se3tn_color_stats (csrc/fit_stats.hip, the colour instantiation) against the per-pixel loop of tests/color_fit_oracle.py,
se3tn_verify_poses_host against the step-by-step path (render_window per pose + Engine.color_stats), and the scene of
tests/color_fit_scene.py on the device: Tracker.verify, and Tracker.acquire with and without the colour switch.

Every record is integers, so every comparison is np.array_equal: no tolerance anywhere.  Without the feature every test fails: the
names do not exist."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import color_fit_oracle as CO
import color_fit_scene as CS
from oracle import fixtures as Fx
from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
TOL = CO.TOL


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, se3._lib.FIT_MAX_PAIRS + 1)          # max_batch just allows capacity + 1 pairs
    yield e
    e.close()


class Pairs:
    """the shared cases on the device"""

    def __init__(self, se3):
        self.se3 = se3
        self.cases = CO.cases()
        self.names = list(self.cases)
        self._dev = {}

    def dev(self, a):
        if id(a) not in self._dev:
            self._dev[id(a)] = torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).cuda()
        return self._dev[id(a)]

    def descriptors(self, names, rgb=True):
        out = []
        for side in (0, 1):
            group = []
            for k in names:
                c = self.cases[k][side]
                d = dict(depth=self.dev(c["depth"]), window=c["window"])
                if rgb:
                    d["rgb"] = self.dev(c["rgb"])
                group.append(d)
            out.append(group)
        return out

    def expected(self, names):
        want = CO.expected()
        return CO.as_arrays(self.se3, [want[k] for k in names])


@pytest.fixture(scope="module")
def pairs(se3):
    return Pairs(se3)


def crop_array(se3, group):
    arr = (se3._lib.Crop * len(group))()
    for i, c in enumerate(group):
        d = c["depth"]
        arr[i].rgb = c["rgb"].data_ptr() if c.get("rgb") is not None else None
        arr[i].depth = d.data_ptr()
        arr[i].H, arr[i].W = int(d.shape[0]), int(d.shape[1])
        arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = c["window"]
    return arr


# ---- se3tn_color_stats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 32, 33])
def test_color_stats_equals_the_oracle_and_fit_stats(se3, eng, pairs, n):
    assert se3._lib.FIT_MAX_PAIRS == 32 and eng.max_batch == 33                 # 33 pairs: two launches
    names = [pairs.names[(5 * i + n) % len(pairs.names)] for i in range(n)] if n < len(pairs.names) else \
        [pairs.names[i % len(pairs.names)] for i in range(n)]
    if n == 33:
        assert set(names) == set(pairs.names)                                     # every case, the saturating one included
    model, observed = pairs.descriptors(names)
    fit, col = eng.color_stats(model, observed, TOL)
    want_fit, want_col = pairs.expected(names)
    assert col.dtype == se3._lib.COLOR_FIT_DTYPE and fit.dtype == se3._lib.FIT_DTYPE
    for i, k in enumerate(names):
        assert np.array_equal(col[i], want_col[i]), (k, col[i], want_col[i])
        assert np.array_equal(fit[i], want_fit[i]), (k, fit[i], want_fit[i])
    # the depth record is se3tn_fit_stats' record, bit for bit
    m_d, o_d = pairs.descriptors(names, rgb=False)
    assert fit.tobytes() == eng.fit_stats(m_d, o_d, TOL).tobytes()
    # the same call again on the same context: the counters were re-armed
    fit2, col2 = eng.color_stats(model, observed, TOL)
    assert fit2.tobytes() == fit.tobytes() and col2.tobytes() == col.tobytes()
    # another tolerance re-classifies
    fit3, col3 = eng.color_stats(model[:1], observed[:1], TOL + 5)
    w = CO.as_arrays(se3, [CO.record(pairs.cases[names[0]][0], pairs.cases[names[0]][1], TOL + 5)])
    assert np.array_equal(fit3, w[0]) and np.array_equal(col3, w[1])


def test_color_stats_without_the_depth_records_and_back_to_back(se3, eng, pairs):
    """fit_out_dev = NULL; launches back to back with no synchronisation, a smaller batch after a larger one: stale counters or a
    wrong re-arm would show here; nothing past the n records is written"""
    big = [pairs.names[i % len(pairs.names)] for i in range(33)]
    small = ["down_nonsquare", "saturating", "identity"]
    outs = [torch.full((33, 112), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
    only = torch.full((34, 80), 0xAB, dtype=torch.uint8, device="cuda")
    mb, ob = pairs.descriptors(big)
    ms, os_ = pairs.descriptors(small)
    eng.color_stats(mb, ob, TOL, out=outs[0])
    eng.color_stats(ms, os_, TOL, out=outs[1])
    eng.color_stats(list(reversed(mb)), list(reversed(ob)), TOL, out=outs[2])
    rc = eng.lib.se3tn_color_stats(eng._h, crop_array(se3, mb), crop_array(se3, ob), 33, TOL, None, C.c_void_p(only.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.se3tn_last_error()
    torch.cuda.synchronize()
    for out, names in ((outs[0], big), (outs[1], small), (outs[2], list(reversed(big)))):
        fit, col = eng.color_records(out, len(names))
        want_fit, want_col = pairs.expected(names)
        assert np.array_equal(fit, want_fit) and np.array_equal(col, want_col)
    assert (outs[1].reshape(-1)[3 * 112:].cpu().numpy() == 0xAB).all()
    host = only.cpu().numpy()
    assert np.array_equal(host[:33].reshape(-1).view(se3._lib.COLOR_FIT_DTYPE), pairs.expected(big)[1]) and (host[33] == 0xAB).all()


def test_color_stats_same_records_from_a_captured_and_replayed_graph(se3, eng, pairs):
    names = [pairs.names[(3 * i) % len(pairs.names)] for i in range(33)]          # two launches inside the capture: a single chain
    model, observed = pairs.descriptors(names)
    out = torch.zeros((33, 112), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.color_stats(model, observed, TOL, out=out)                             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        eng.color_stats(model, observed, TOL, out=out)
    want_fit, want_col = pairs.expected(names)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        fit, col = eng.color_records(out, 33)
        assert np.array_equal(fit, want_fit) and np.array_equal(col, want_col)
    # ... and an eager launch after the replays finds the counters armed
    fit, col = eng.color_stats(model[:5], observed[:5], TOL)
    assert np.array_equal(fit, want_fit[:5]) and np.array_equal(col, want_col[:5])


def test_color_stats_refusals_leave_the_context_usable(se3, eng, pairs):
    lib = eng.lib
    model, observed = pairs.descriptors(["identity"] * 34)
    out = torch.zeros((34, 112), dtype=torch.uint8, device="cuda")
    m, o = crop_array(se3, model), crop_array(se3, observed)
    f, p = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 34 * 32)
    for n, tol in ((0, TOL), (34, TOL), (-1, TOL), (1, 0), (1, 65536), (1, -3)):
        assert lib.se3tn_color_stats(eng._h, m, o, n, tol, f, p, None) == E_ARG, (n, tol)
    assert lib.se3tn_color_stats(eng._h, None, o, 1, TOL, f, p, None) == E_ARG and lib.se3tn_color_stats(eng._h, m, None, 1, TOL, f, p, None) == E_ARG
    assert lib.se3tn_color_stats(eng._h, m, o, 1, TOL, f, None, None) == E_ARG
    empty = crop_array(se3, [dict(model[0], window=(10, 10, 10, 50))])
    assert lib.se3tn_color_stats(eng._h, empty, o, 1, TOL, f, p, None) == E_ARG
    for field in ("rgb", "depth"):                                                # a descriptor without rgb is refused too
        null = crop_array(se3, model[:1]); setattr(null[0], field, None)
        assert lib.se3tn_color_stats(eng._h, m, null, 1, TOL, f, p, None) == E_ARG and lib.se3tn_color_stats(eng._h, null, o, 1, TOL, f, p, None) == E_ARG
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                            # a refused call writes nothing
    fit, col = eng.color_stats(model[:1], observed[:1], TOL)
    want = pairs.expected(["identity"])
    assert np.array_equal(fit, want[0]) and np.array_equal(col, want[1])


# ---- se3tn_verify_poses_host against the step-by-step path -------------------------------------------------------------------------------
VH, VW = Fx.SOUP_FRAME_HW
VK = Fx.SOUP_FRAME_K
VWIDTH = 170.0
VTOL = 12
G_OBJECT = Fx.pose(11, (0.004, -0.003, 0.5))                # where the object is in the frame
P_EDGE = Fx.pose(3, (0.125, 0.085, 0.5))                    # a window over the right / bottom edge of the frame
P_MISS = Fx.pose(5, (0.6, 0.5, 0.9))                        # a window off the frame
ROUTES = ["window", "frame"]


def window_of(P):
    bb = O.compute_bbox(P, VK, VWIDTH, (1000, 1000, 1000))
    return int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())


def route_mesh(route):
    """a vertex-colour mesh on the window route, a textured one on the frame route"""
    if route == "window":
        return Fx.icosphere(2, 0.05, 1)
    ms = Fx.textured_sphere(2)
    return dict(vertices=ms["vertices"], faces=ms["faces"], colors=ms["colors"], uv=ms["uv"], texture=ms["texture"], kd=ms["kd"])


def make_verify_tracker(se3, route):
    info = dict(Fx.DATASET_INFO, object_width=VWIDTH,
                camera=dict(height=VH, width=VW, focalX=VK[0, 0], focalY=VK[1, 1], centerX=VK[0, 2], centerY=VK[1, 2]))
    if route == "frame":
        info = dict(info, renderer="pyrenderer")
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, max_samples=8)
    trk.renderer = se3.HipRenderer(trk.engine, route_mesh(route), mode="pyrender", frame_size=(VH, VW)) if route == "frame" \
        else se3.HipRenderer(trk.engine, route_mesh(route))
    assert trk.one_call and trk.renderer.full_frame == (route == "frame")
    return trk


@pytest.fixture(scope="module")
def verify_setup(se3):
    """route -> (tracker, a twin that never verifies, frame): the frame shows the route's own object at G_OBJECT -- its full-frame
    render (the frame route's renderer, or a full-frame renderer of the same mesh) over a textured wall at 900 mm with holes"""
    out = {}
    for route in ROUTES:
        trk, twin = make_verify_tracker(se3, route), make_verify_tracker(se3, route)
        painter = trk.renderer if route == "frame" else se3.HipRenderer(trk.engine, dict(route_mesh(route), kd=(1.0, 1.0, 1.0)), mode="pyrender",
                                                                        frame_size=(VH, VW))
        orgb, odep = painter.render_frame(G_OBJECT, VK)
        rng = np.random.default_rng(9)
        yy, xx = np.mgrid[0:VH, 0:VW]
        rgb = Fx.structured_frame(401, VH, VW)[0].copy()
        dep = (900 + 0.5 * (xx - VW / 2) + 0.3 * (yy - VH / 2)).astype(np.uint16)
        dep[rng.random((VH, VW)) < 0.04] = 0
        on = odep > 0
        rgb[on] = np.clip(orgb[on].astype(np.int64) * 3 // 4 + 30, 0, 255).astype(np.uint8)    # another gain and offset than the model's
        dep[on] = odep[on] + rng.integers(-4, 5, int(on.sum())).astype(np.uint16)
        assert on.sum() > 1500
        out[route] = (trk, twin, (np.ascontiguousarray(rgb), np.ascontiguousarray(dep)))
    return out


def hypotheses(n):
    """n poses around G_OBJECT; from three on, the last two are the one over the frame's edge and the one off the frame"""
    out = []
    for k in range(n):
        P = G_OBJECT.copy()
        P[:3, :3] = Fx.pose(40 + k, (0, 0, 1))[:3, :3] if k % 3 == 2 else P[:3, :3]
        P[:3, 3] += np.array([0.003, -0.002, 0.004]) * k
        out.append(P)
    if n >= 3:
        out[-2], out[-1] = P_EDGE, P_MISS
    return np.stack(out)


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("route", ROUTES)
def test_verify_poses_equals_the_step_by_step_path(se3, verify_setup, route, n):
    trk, twin, (rgb, dep) = verify_setup[route]
    poses = hypotheses(n)
    fit, col, bbox = trk.engine.verify_poses(trk.renderer, poses, rgb, dep, trk.K, trk.object_width, VTOL)
    want_fit, want_col = trk._verify_stepwise(poses, rgb, dep, VTOL)
    assert fit.dtype == se3._lib.FIT_DTYPE and col.dtype == se3._lib.COLOR_FIT_DTYPE and bbox.shape == (n, 4, 2)
    for i in range(n):
        assert np.array_equal(fit[i], want_fit[i]) and np.array_equal(col[i], want_col[i]), (route, n, i, fit[i], want_fit[i], col[i], want_col[i])
        assert np.array_equal(bbox[i], se3.compute_bbox(poses[i], trk.K, trk.object_width)), (route, n, i)
    assert int(col["px"][0]) > 1000 and (col["px"] == fit["inlier_px"]).all() and (col["tol_mm"] == VTOL).all()
    if n >= 3:
        l, t, r, b = window_of(P_EDGE)
        assert (r > VW or b > VH) and l < VW and t < VH                            # leaves the frame, still touches it
        l, t, r, b = window_of(P_MISS)
        assert l >= VW or t >= VH
        assert int(col["px"][-1]) == 0 and not col[-1]["sum_mo"].any() and int(fit["seen_px"][-1]) == 0
        assert int(fit["model_px"][-2]) > 0
    # Tracker.verify takes the one call with the built-in renderer, the step-by-step path otherwise: equal records, and the scores
    f1, c1, s1 = trk.verify(poses, rgb, dep, tol_mm=VTOL)
    trk.one_call = False
    try:
        f2, c2, s2 = trk.verify(poses, rgb, dep, tol_mm=VTOL)
    finally:
        trk.one_call = True
    assert f1.tobytes() == f2.tobytes() == fit.tobytes() and c1.tobytes() == c2.tobytes() == col.tobytes()
    assert np.array_equal(s1, s2) and np.array_equal(s1, se3.utils.color_score(col)) and s1[0] > 0.5
    # the verify calls left no state behind: a tracking call returns the bits it returns on a context that never verified
    prev = list(poses[:min(n, 3)])
    if n >= 3:
        prev[-1] = P_EDGE
    got = trk.on_track_batch(prev, [rgb] * len(prev), [dep] * len(prev))
    lp = trk.last_prediction
    want = twin.on_track_batch(prev, [rgb] * len(prev), [dep] * len(prev))
    lw = twin.last_prediction
    assert np.array_equal(got, want) and np.array_equal(lp["trans"], lw["trans"]) and np.array_equal(lp["rot"], lw["rot"])
    assert np.array_equal(lp["bbox"], lw["bbox"])
    for a, b_ in zip(lp["rgbA"] + lp["depthA"], lw["rgbA"] + lw["depthA"]):
        assert torch.equal(a, b_)


def test_verify_poses_refusals(se3, verify_setup):
    trk, _, (rgb, dep) = verify_setup["window"]
    ok = hypotheses(2)
    behind = ok.copy(); behind[1, 2, 3] = -0.5
    singular = ok.copy(); singular[0, :3, :3] = 0.0
    with pytest.raises(se3._lib.Se3tnError, match="not in front"):
        trk.engine.verify_poses(trk.renderer, behind, rgb, dep, trk.K, trk.object_width, VTOL)
    with pytest.raises(se3._lib.Se3tnError, match="singular"):
        trk.engine.verify_poses(trk.renderer, singular, rgb, dep, trk.K, trk.object_width, VTOL)
    with pytest.raises(se3._lib.Se3tnError, match="se3tn_max_batch"):
        trk.engine.verify_poses(trk.renderer, hypotheses(9), rgb, dep, trk.K, trk.object_width, VTOL)
    with pytest.raises(se3._lib.Se3tnError, match="tol_mm"):
        trk.engine.verify_poses(trk.renderer, ok, rgb, dep, trk.K, trk.object_width, 0)
    with pytest.raises(ValueError, match="max_samples"):
        trk.verify(hypotheses(9), rgb, dep)
    fit, col, _ = trk.engine.verify_poses(trk.renderer, ok, rgb, dep, trk.K, trk.object_width, VTOL)      # usable afterwards
    want_fit, want_col = trk._verify_stepwise(ok, rgb, dep, VTOL)
    assert np.array_equal(fit, want_fit) and np.array_equal(col, want_col)


def test_verify_poses_is_refused_inside_a_stream_capture(se3, verify_setup):
    """the call is synchronous: under a capture of the current stream it says so (SE3TN_E_STATE), the capture stays whole and replays,
    and the context gives the same records afterwards"""
    trk, _, (rgb, dep) = verify_setup["window"]
    poses = hypotheses(5)
    want = trk.verify(poses, rgb, dep, tol_mm=VTOL)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d.*captured" % E_STATE):
            trk.engine.verify_poses(trk.renderer, poses, rgb, dep, trk.K, trk.object_width, VTOL)
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d.*captured" % E_STATE):
            trk.verify(poses, rgb, dep, tol_mm=VTOL)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    got = trk.verify(poses, rgb, dep, tol_mm=VTOL)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])


# ---- the scene on the device ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_tracker(se3, tmp_path_factory):
    return CS.make_tracker(se3, tmp_path_factory.mktemp("color_fit"))


def test_scene_verify_orders_the_poses_as_the_cpu_evaluation(se3, scene_tracker):
    trk = scene_tracker
    rgb, depth = CS.frames()
    assert np.array_equal(trk.K, CS.K) and trk.object_width == CS.OBJECT_WIDTH_MM
    want_fit, want_col = CS.records(se3, CS.oracle_render)                          # oracle renderer + NumPy rule, all on the CPU
    # the HIP render equals the oracle renderer's, every byte (tests/test_gl_swiftshader.py): so do the records
    for G in (CS.true_pose(), CS.flipped_pose()):
        win = se3.HipRenderer.gl_window(G, trk.K, trk.object_width)
        hr, hd = trk.renderer.render(G, trk.K, win)
        orr, od = CS.oracle_render(G, win)
        assert np.array_equal(hr, orr) and np.array_equal(hd, od)
    fit, col, score = trk.verify([CS.true_pose(), CS.flipped_pose()], rgb, depth, tol_mm=CS.TOL)
    assert np.array_equal(fit, want_fit) and np.array_equal(col, want_col)
    want_score = se3.utils.color_score(want_col)
    assert np.array_equal(score, want_score) and score[0] > score[1] and score[1] < 0.5 * score[0]


def test_scene_acquire_with_and_without_colour(se3, scene_tracker, golden_dir):
    trk = scene_tracker
    rgb, depth = CS.frames()
    # colour off: the keys and the pose of the commit before the switch existed (recorded by running that commit)
    plain = trk.acquire(rgb, depth, **CS.ACQUIRE)
    la = trk.last_acquire
    assert not {"depth_chosen", "color_fit", "color_score", "candidates"} & set(la)
    golden = np.load(os.path.join(golden_dir, CS.GOLDEN_ACQUIRE))
    assert plain.tobytes() == golden["pose"].tobytes() and la["chosen"] == int(golden["chosen"])
    assert la["final_fit"].tobytes() == golden["final_fit"].tobytes()
    # colour on, both spellings
    pose = trk.acquire(rgb, depth, colour=True, **CS.ACQUIRE)
    lc = trk.last_acquire
    assert lc["depth_chosen"] == la["chosen"] and lc["final_fit"].tobytes() == la["final_fit"].tobytes()   # the pool is formed as before
    cand, score = lc["candidates"], lc["color_score"]
    d = lc["depth_chosen"]
    assert np.array_equal(cand, np.flatnonzero(lc["final_fit"]["inlier_pts"] >= 0.9 * int(lc["final_fit"]["inlier_pts"][d]))) and d in cand
    assert lc["chosen"] in cand and score[lc["chosen"]] == score[cand].max() > 0 and len(score) == len(lc["final_fit"])
    others = np.setdiff1d(np.arange(len(score)), cand)
    assert not score[others].any() and not lc["color_fit"][others]["px"].any()
    pool = np.concatenate([lc["aligned"], lc["local"]])
    for part in (cand[:8], cand[8:]):                                             # (the pool of 16 may hold more candidates than max_samples)
        if len(part):
            _, want_col, want_score = trk.verify(pool[part], rgb, depth, tol_mm=CS.TOL)
            assert np.array_equal(lc["color_fit"][part], want_col) and np.array_equal(score[part], want_score)
    err = CS.rotation_error_deg(pose)
    print("acquire: depth alone chose %d (%.1f deg from the truth), colour chose %d (%.1f deg); scores %s over candidates %s"
          % (d, CS.rotation_error_deg(plain), lc["chosen"], err, np.round(score[cand], 3), cand))
    assert err <= CS.SEARCH_STEP_DEG and np.linalg.norm(pose[:3, 3] - CS.true_pose()[:3, 3]) < 0.01
    pose2 = trk.acquire(rgb, depth, color=True, color_within=0.9, **CS.ACQUIRE)
    assert np.array_equal(pose2, pose) and trk.last_acquire["chosen"] == lc["chosen"]
    # colour_within = 0 admits the whole pool
    trk.acquire(rgb, depth, colour=True, colour_within=0.0, **CS.ACQUIRE)
    assert len(trk.last_acquire["candidates"]) == len(trk.last_acquire["final_fit"])
    # recover takes the same switch
    lost = CS.flipped_pose()
    lost[:3, 3] += (0.012, -0.008, 0.01)
    r_plain = trk.recover(lost, rgb, depth, tol_mm=CS.TOL, refine=0, facing=True, align=20)
    assert "color_score" not in trk.last_recover
    r_col = trk.recover(lost, rgb, depth, tol_mm=CS.TOL, refine=0, facing=True, align=20, colour=True)
    lr = trk.last_recover
    assert lr["color_score"][lr["chosen"]] == lr["color_score"][lr["candidates"]].max() and lr["depth_chosen"] in lr["candidates"]
    assert np.array_equal(r_plain, np.concatenate([lr["aligned"], trk._compose(*se3.recover.lattice_factors(lost), lr["top_idx"])])[lr["depth_chosen"]])
    assert np.array_equal(r_col, np.concatenate([lr["aligned"], trk._compose(*se3.recover.lattice_factors(lost), lr["top_idx"])])[lr["chosen"]])
