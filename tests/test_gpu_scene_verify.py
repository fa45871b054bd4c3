"""GPU: the scene-aware colour verification -- se3tn_color_stats_scene (csrc/fit_stats.hip, fit_stats_kernel<true, true>) against the
per-pixel loop of tests/scene_verify_oracle.py on the shared cases of tests/scene_verify_scene.py, at the batch sizes around the
launch's 16 pairs, under an all-zero scene against se3tn_color_stats, with its records in mapped pinned host memory, and the counters
it shares with the plain instantiations; se3tn_verify_poses_scene_host and MultiTracker.recover(colour=True) on the slab-and-plate scene,
against the oracle renderer and the loop.

Every record is integers, so every comparison is an equality: no tolerance anywhere.  Without the feature every test fails: the names
do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_fit_oracle as CO
import color_fit_scene as CS
import scene_verify_oracle as VO
import scene_verify_scene as VS
from mapped_memory import Mapped

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
TOL = VS.TOL


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def chunk(se3):
    assert se3._lib.FIT_SCENE_MAX_PAIRS == 16
    return se3._lib.FIT_SCENE_MAX_PAIRS


@pytest.fixture(scope="module")
def eng(se3, chunk):
    e = se3.Engine(0, 2 * chunk + 3)                        # max_batch: two full launches and a tail of three pairs
    yield e
    e.close()


class Triples:
    """the shared cases on the device"""

    def __init__(self, se3):
        self.se3 = se3
        self.cases = VS.cases()
        self.names = list(self.cases)
        self._dev = {}

    def dev(self, a):
        if id(a) not in self._dev:
            self._dev[id(a)] = (a, torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).cuda())
        return self._dev[id(a)][1]

    def descriptor(self, c):
        d = dict(depth=self.dev(c["depth"]), window=c["window"])
        if "rgb" in c:
            d["rgb"] = self.dev(c["rgb"])
        return d

    def descriptors(self, names):
        """(model, observed, scene) lists"""
        return tuple([self.descriptor(self.cases[k][side]) for k in names] for side in range(3))

    def cycle(self, n, start=0, step=1):
        return [self.names[(start + step * i) % len(self.names)] for i in range(n)]

    def expected(self, names):
        want = VS.expected()
        return VO.as_arrays(self.se3, [want[k] for k in names])


@pytest.fixture(scope="module")
def triples(se3):
    return Triples(se3)


def crop_array(se3, group):
    arr = (se3._lib.Crop * len(group))()
    for i, c in enumerate(group):
        d = c["depth"]
        arr[i].rgb = c["rgb"].data_ptr() if c.get("rgb") is not None else None
        arr[i].depth = d.data_ptr()
        arr[i].H, arr[i].W = int(d.shape[0]), int(d.shape[1])
        arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = c["window"]
    return arr


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- se3tn_color_stats_scene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 35])
def test_color_stats_scene_equals_the_loop_at_every_batch_size(se3, eng, triples, chunk, n):
    """n = 1, one launch's pairs, that plus one (the chunk seam) and max_batch (two full chunks and a tail): pair i is its case's record
    whatever n and wherever it stands in the call; the same call again finds the counters re-armed"""
    assert (1, chunk, chunk + 1, eng.max_batch) == (1, 16, 17, 35) and len(triples.names) == 10
    names = ["boundaries"] if n == 1 else triples.cycle(n, start=n, step=3 if n != 17 else 1)
    if n >= 16:
        assert set(names) == set(triples.names)                                   # every case, and around the seam
    model, observed, scene = triples.descriptors(names)
    fit, col = eng.color_stats(model, observed, TOL, scene=scene)
    want_fit, want_col = triples.expected(names)
    assert fit.dtype == se3._lib.SCENE_CROP_FIT_DTYPE and col.dtype == se3._lib.COLOR_FIT_DTYPE
    for i, k in enumerate(names):
        assert np.array_equal(fit[i], want_fit[i]), (k, i, fit[i], want_fit[i])
        assert np.array_equal(col[i], want_col[i]), (k, i, col[i], want_col[i])
    assert (col["px"] == fit["inlier_px"]).all() and (fit["seen_px"] == fit["inlier_px"] + fit["front_px"] + fit["behind_px"]).all()
    fit2, col2 = eng.color_stats(model, observed, TOL, scene=scene)
    assert fit2.tobytes() == fit.tobytes() and col2.tobytes() == col.tobytes()
    # the reversed order, enqueued back to back behind a smaller call: stale counters or a wrong re-arm would show
    out_small = torch.full((3, 112), 0xAB, dtype=torch.uint8, device="cuda")
    out_rev = torch.full((n + 1, 112), 0xAB, dtype=torch.uint8, device="cuda")
    eng.color_stats(model[:1], observed[:1], TOL, out=out_small, scene=scene[:1])
    eng.color_stats(model[::-1], observed[::-1], TOL, out=out_rev, scene=scene[::-1])
    torch.cuda.synchronize()
    f1, c1 = eng.color_records(out_small, 1, scene=True)
    assert np.array_equal(f1, want_fit[:1]) and np.array_equal(c1, want_col[:1]) and (out_small.cpu().numpy().reshape(-1)[112:] == 0xAB).all()
    fr, cr = eng.color_records(out_rev, n, scene=True)
    assert np.array_equal(fr, want_fit[::-1]) and np.array_equal(cr, want_col[::-1]) and (out_rev[n].cpu().numpy() == 0xAB).all()
    # another tolerance re-classifies
    m, o, s = triples.cases[names[0]]
    fit3, col3 = eng.color_stats(model[:1], observed[:1], TOL + 5, scene=scene[:1])
    w = VO.as_arrays(se3, [VO.record(m, o, s, TOL + 5)])
    assert np.array_equal(fit3, w[0]) and np.array_equal(col3, w[1])


def test_an_all_zero_scene_gives_the_bytes_of_color_stats(se3, eng, triples):
    cases = CO.cases()
    names = [list(cases)[i % len(cases)] for i in range(17)]                      # every case of the plain colour check, two launches
    model = [triples.descriptor(cases[k][0]) for k in names]
    observed = [triples.descriptor(cases[k][1]) for k in names]
    zero_frame = torch.zeros((CO.H, CO.W), dtype=torch.int16, device="cuda")
    zero_other = torch.zeros((7, 9), dtype=torch.int16, device="cuda")
    plain_fit, plain_col = eng.color_stats(model, observed, TOL)
    for scene in ([dict(depth=zero_frame, window=o["window"]) for o in observed], [dict(depth=zero_other, window=(0, 0, 9, 7))] * 17):
        fit, col = eng.color_stats(model, observed, TOL, scene=scene)
        assert fit.tobytes() == plain_fit.tobytes() and col.tobytes() == plain_col.tobytes()
    want = CO.as_arrays(se3, [CO.expected()[k] for k in names])
    assert np.array_equal(plain_fit, want[0]) and np.array_equal(plain_col, want[1])


def test_the_plain_calls_after_a_scene_call_return_a_fresh_engines_bytes(se3, eng, triples):
    """the scene instantiation uses the colour counters with one more sum: it leaves every word zero for the instantiations that
    share the layout, and the depth-only counters alone"""
    names = triples.cycle(35)
    model, observed, scene = triples.descriptors(names)
    depth_only = [[dict(depth=c["depth"], window=c["window"]) for c in group] for group in (model, observed)]
    fresh = se3.Engine(0, eng.max_batch)
    want_col = [a.tobytes() for a in fresh.color_stats(model, observed, TOL)]
    want_fit = fresh.fit_stats(depth_only[0], depth_only[1], TOL).tobytes()
    fresh.close()
    first = eng.color_stats(model, observed, TOL, scene=scene)
    got_col = [a.tobytes() for a in eng.color_stats(model, observed, TOL)]
    got_fit = eng.fit_stats(depth_only[0], depth_only[1], TOL).tobytes()
    assert got_col == want_col and got_fit == want_fit
    again = eng.color_stats(model, observed, TOL, scene=scene)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    assert np.array_equal(first[0], triples.expected(names)[0])


def test_records_into_mapped_pinned_host_memory(se3, eng, triples):
    n = 17
    names = triples.cycle(n, start=4)
    model, observed, scene = triples.descriptors(names)
    want_fit, want_col = eng.color_stats(model, observed, TOL, scene=scene)        # device memory
    m = Mapped(112 * n + 64)
    try:
        rc = eng.lib.se3tn_color_stats_scene(eng._h, crop_array(se3, model), crop_array(se3, observed), crop_array(se3, scene), n, TOL,
                                             C.c_void_p(m.d.value), C.c_void_p(m.d.value + 32 * n), stream())
        assert rc == 0, eng.lib.se3tn_last_error()
        torch.cuda.synchronize()
        host = m.read()
    finally:
        m.close()
    assert host[:32 * n].tobytes() == want_fit.tobytes() and host[32 * n:112 * n].tobytes() == want_col.tobytes()
    assert (host[112 * n:] == 0xEE).all()
    assert np.array_equal(want_fit, triples.expected(names)[0]) and np.array_equal(want_col, triples.expected(names)[1])


def test_color_stats_scene_refusals_leave_the_context_usable(se3, eng, triples):
    lib = eng.lib
    model, observed, scene = triples.descriptors(["same_identity"] * 36)
    out = torch.zeros((36, 112), dtype=torch.uint8, device="cuda")
    m, o, s = crop_array(se3, model), crop_array(se3, observed), crop_array(se3, scene)
    f, p = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 36 * 32)
    for n, tol in ((0, TOL), (36, TOL), (-1, TOL), (1, 0), (1, 65536)):
        assert lib.se3tn_color_stats_scene(eng._h, m, o, s, n, tol, f, p, None) == E_ARG, (n, tol)
    assert lib.se3tn_color_stats_scene(eng._h, m, o, None, 1, TOL, f, p, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, None, o, s, 1, TOL, f, p, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, m, o, s, 1, TOL, f, None, None) == E_ARG
    # a scene descriptor without depth, an empty scene window, an empty scene image -- also when it is the last of the call
    for edit in (dict(depth=None), dict(right=scene[0]["window"][0]), dict(bottom=scene[0]["window"][1]), dict(H=0)):
        for n, i in ((1, 0), (17, 16)):
            bad = crop_array(se3, scene)
            for key, v in edit.items():
                setattr(bad[i], key, v)
            assert lib.se3tn_color_stats_scene(eng._h, m, o, bad, n, TOL, f, p, None) == E_ARG, (edit, n)
            assert b"scene descriptor %d" % i in lib.se3tn_last_error()
    null = crop_array(se3, observed); null[0].rgb = None                           # the refusals of se3tn_color_stats
    assert lib.se3tn_color_stats_scene(eng._h, m, null, s, 1, TOL, f, p, None) == E_ARG
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                            # a refused call writes nothing
    fit, col = eng.color_stats(model[:1], observed[:1], TOL, scene=scene[:1])
    want = triples.expected(["same_identity"])
    assert np.array_equal(fit, want[0]) and np.array_equal(col, want[1])


# ---- the slab and the plate ------------------------------------------------------------------------------------------------------------
P_EDGE_SHIFT = (0.08, 0.05, 0.0)                            # a window over the right / bottom edge of the frame
P_MISS_SHIFT = (0.5, 0.3, 0.2)                              # a window off the frame


def shifted(G, d):
    P = G.copy()
    P[:3, 3] += d
    return P


def make_plate_tracker(se3, directory):
    """color_fit_scene.make_tracker for the plate: random-init fixture weights, the plate's cloud and normals, the built-in rasteriser
    on the plate's mesh"""
    import os
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    Hs, Ws = VS.HW
    info = dict(Fx.DATASET_INFO, object_width=VS.OBJECT_WIDTH_MM,
                camera=dict(height=Hs, width=Ws, focalX=VS.K[0, 0], focalY=VS.K[1, 1], centerX=VS.K[0, 2], centerY=VS.K[1, 2]))
    pts, nrm = VS.plate_model()
    ply = os.path.join(str(directory), "plate.ply")
    with open(ply, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % len(pts))
        f.write("".join("property double %s\n" % k for k in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n")
        for v, n in zip(pts, nrm):
            f.write("%.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(v) + tuple(n)))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, model_path=ply, max_samples=8)
    trk.renderer = se3.HipRenderer(trk.engine, VS.plate_mesh())
    return trk


@pytest.fixture(scope="module")
def slab(se3, tmp_path_factory):
    """(L, a twin of L that never verifies, P)"""
    d = tmp_path_factory.mktemp("scene_verify")
    return CS.make_tracker(se3, d), CS.make_tracker(se3, d), make_plate_tracker(se3, d)


@pytest.fixture(scope="module")
def device_scene(se3, slab):
    """the composed depth of the tracked plate as the library composes it (Engine.scene_fit), a cuda tensor; equal to the oracle's
    full-frame render, every pixel"""
    L, _, P = slab
    rgb, depth = VS.frames()
    dep_d = torch.from_numpy(np.array(depth.view(np.int16))).cuda()
    _, _, scene = L.engine.scene_fit([(P.renderer, VS.OBJECT_WIDTH_MM)], VS.plate_pose()[None], dep_d, VS.K, tol_mm=VS.STOL, scene=True)
    assert np.array_equal(scene.cpu().numpy().view(np.uint16), VS.oracle_scene())
    return scene


def oracle_records(se3, poses, tol=VS.STOL):
    """(fit, colour) of slab hypotheses by the oracle renderer and the loop"""
    return VO.as_arrays(se3, [VO.record(*VS.triple(G), tol) for G in poses])


def test_verify_poses_scene_host_equals_the_oracle(se3, slab, device_scene):
    L, twin, _ = slab
    rgb, depth = VS.frames()
    true, flipped = CS.true_pose(), CS.flipped_pose()
    poses = np.stack([true, flipped, shifted(true, P_EDGE_SHIFT), shifted(true, P_MISS_SHIFT)])
    Hs, Ws = VS.HW
    l, t, r, b = VS.crop_window(poses[2])
    assert (r > Ws and b > Hs) and l < Ws and t < Hs                              # leaves the frame, still touches it
    assert VS.crop_window(poses[3])[0] >= Ws
    # the window-route rasteriser is byte-identical to the oracle renderer, so the records are the loop's on the oracle's images
    for G in poses[:3]:
        win = se3.HipRenderer.gl_window(G, L.K, L.object_width)
        hr, hd = L.renderer.render(G, L.K, win)
        orr, od = CS.oracle_render(G, win)
        assert np.array_equal(hr, orr) and np.array_equal(hd, od)
    want_fit, want_col = oracle_records(se3, poses)
    for scene in (device_scene, VS.oracle_scene()):                               # the device tensor, and a host array that is uploaded
        fit, col, bbox = L.engine.verify_poses(L.renderer, poses, rgb, depth, L.K, L.object_width, VS.STOL, scene=scene)
        assert fit.dtype == se3._lib.SCENE_CROP_FIT_DTYPE and col.dtype == se3._lib.COLOR_FIT_DTYPE and bbox.shape == (4, 4, 2)
        for i in range(4):
            assert np.array_equal(fit[i], want_fit[i]) and np.array_equal(col[i], want_col[i]), (i, fit[i], want_fit[i], col[i], want_col[i])
            assert np.array_equal(bbox[i], se3.compute_bbox(poses[i], L.K, L.object_width)), i
    assert int(fit["hidden_px"][0]) == int(fit["hidden_px"][1]) > 0 and int(fit["model_px"][2]) > 0
    assert int(col["px"][3]) == 0 and int(fit["seen_px"][3]) == 0 and int(fit["hidden_px"][3]) == 0
    # Tracker.verify(scene=): the one call with the built-in renderer, the step-by-step path otherwise; and the scores order the poses
    f1, c1, s1 = L.verify(poses, rgb, depth, tol_mm=VS.STOL, scene=device_scene)
    L.one_call = False
    try:
        f2, c2, s2 = L.verify(poses, rgb, depth, tol_mm=VS.STOL, scene=device_scene)
    finally:
        L.one_call = True
    assert f1.tobytes() == f2.tobytes() == fit.tobytes() and c1.tobytes() == c2.tobytes() == col.tobytes() and np.array_equal(s1, s2)
    assert np.array_equal(s1, se3.utils.color_score(want_col)) and s1[1] < 0 < s1[0]
    _, _, plain = L.verify(poses[:2], rgb, depth, tol_mm=VS.STOL)                 # the plain rule confirms the wrong pose
    assert plain[0] < 0 < plain[1]
    # the calls left no state behind: a tracking call returns the bits it returns on a tracker that never verified
    prev = [true, flipped, poses[2]]
    got = L.on_track_batch(prev, [rgb] * 3, [depth] * 3)
    want = twin.on_track_batch(prev, [rgb] * 3, [depth] * 3)
    lp, lw = L.last_prediction, twin.last_prediction
    assert np.array_equal(got, want) and np.array_equal(lp["trans"], lw["trans"]) and np.array_equal(lp["rot"], lw["rot"])
    assert np.array_equal(lp["bbox"], lw["bbox"])
    for a, b_ in zip(lp["rgbA"] + lp["depthA"], lw["rgbA"] + lw["depthA"]):
        assert torch.equal(a, b_)


def test_verify_poses_scene_host_refusals_write_nothing(se3, slab, device_scene):
    L, _, _ = slab
    rgb, depth = VS.frames()
    poses = np.stack([CS.true_pose(), CS.flipped_pose()])
    want = L.engine.verify_poses(L.renderer, poses, rgb, depth, L.K, L.object_width, VS.STOL, scene=device_scene)
    with pytest.raises(se3._lib.Se3tnError, match="se3tn_max_batch"):
        L.engine.verify_poses(L.renderer, np.stack([poses[0]] * 9), rgb, depth, L.K, L.object_width, VS.STOL, scene=device_scene)
    with pytest.raises(ValueError, match="max_samples"):
        L.verify(np.stack([poses[0]] * 9), rgb, depth, scene=device_scene)
    # NULL scene_dev, and n > max_batch, through the C ABI: E_ARG and the outputs keep their bytes
    p = np.ascontiguousarray(np.stack([poses[0]] * 9).reshape(-1, 16))
    Kc = np.ascontiguousarray(L.K, np.float64)
    rgb_c, dep_c = np.ascontiguousarray(rgb), np.ascontiguousarray(depth)
    fit = np.full(9 * 32, 0xCD, np.uint8); col = np.full(9 * 80, 0xCD, np.uint8); bb = np.full(9 * 32, 0xCD, np.uint8)

    def call(n, scene):
        return L.engine.lib.se3tn_verify_poses_scene_host(
            L.engine._h, L.renderer._m, C.c_void_p(p.ctypes.data), n, Kc.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(L.object_width),
            C.c_void_p(rgb_c.ctypes.data), C.c_void_p(dep_c.ctypes.data), scene, VS.HW[0], VS.HW[1], VS.STOL, C.c_void_p(fit.ctypes.data),
            C.c_void_p(col.ctypes.data), C.c_void_p(bb.ctypes.data))
    assert call(2, None) == E_ARG and b"NULL" in L.engine.lib.se3tn_last_error()
    assert call(9, C.c_void_p(device_scene.data_ptr())) == E_ARG and call(0, C.c_void_p(device_scene.data_ptr())) == E_ARG
    assert (fit == 0xCD).all() and (col == 0xCD).all() and (bb == 0xCD).all()
    # inside a capture of the current stream the synchronous call says so; the capture stays whole
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(se3._lib.Se3tnError, match="rc=%d.*captured" % E_STATE):
            L.engine.verify_poses(L.renderer, poses, rgb, depth, L.K, L.object_width, VS.STOL, scene=device_scene)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    got = L.engine.verify_poses(L.renderer, poses, rgb, depth, L.K, L.object_width, VS.STOL, scene=device_scene)   # usable afterwards
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(got, want))


def test_multitracker_recover_with_colour_among_the_plate(se3, slab, device_scene, monkeypatch):
    """L lost, the plate P tracked on it; rot_deg = 180, trans_radius = 0.01, refine = 0, so the pool is the ranked top of a lattice of
    half turns.  recover.lattice_factors turns about the CAMERA axes (dR . R_base), and the slab's own axis is tilted 40 degrees from the
    optical one, so a lattice holds the slab's true pose OR its half turn about its own z, never both.
    (1) L last seen half a turn about its own z off: the pool holds depth-equal poses that are all colour-wrong (an MI355X run:
        candidates [0, 1], scores -0.764 / -0.566); the mechanics are held -- without the switch not one call more and the depth
        winner, with it the pool's scene-rule colour records and scores EQUAL the oracle's and the highest score is chosen.
    (2) L last seen half a turn about the camera's x axis off: the lattice holds the true pose; with the switch the result is within
        a degree of it, without it the result is the depth winner, byte for byte the pool member.
    (3) the choice itself on the pool [half-turned, true] with equal depth records: the plain rule takes the plate's swapped colours for
        the slab's and keeps the half-turned pose, the scene rule chooses the true one."""
    L, _, P = slab
    rgb, depth = VS.frames()
    rgb, depth = np.array(rgb), np.array(depth)
    mt = se3.MultiTracker([L, P])
    poses = np.stack([CS.flipped_pose(), VS.plate_pose()])                        # (1) L was last seen half a turn about its z off
    mt.scene_check = VS.STOL
    mt.on_track(poses, rgb, depth)
    # random weights move the estimates off the objects; the records a trained tracker would leave are those at the poses themselves
    mt.last_prediction["scene_fit"] = mt.scene_fit(poses, depth, tol_mm=VS.STOL)
    assert se3.utils.scene_status(mt.last_prediction["scene_fit"], 0.5, 0.2)[1] == "tracked", mt.last_prediction["scene_fit"]
    kw = dict(lost=[0], rot_deg=(180.0,), trans_radius=0.01, refine=0, tol_mm=VS.STOL)
    calls = []
    real = L.engine.verify_poses
    monkeypatch.setattr(L.engine, "verify_poses", lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))

    def both(prev):
        """recover around prev without and with the switch -> (plain pose, its info, coloured pose, its info, the pool)"""
        del calls[:]
        plain = mt.recover(prev, rgb, depth, **kw)
        ip = mt.last_recover[0]
        assert calls == [] and not {"depth_chosen", "color_fit", "color_score", "candidates"} & set(ip)  # colour off: not one call more
        assert ip["chosen"] == 0 and len(ip["final_fit"]) == 1 and ip["occluders"] == [1]
        out = mt.recover(prev, rgb, depth, colour=True, **kw)
        info = mt.last_recover[0]
        assert len(calls) == 1 and np.array_equal(out[1], prev[1]) and np.array_equal(plain[1], prev[1])
        rots, trans = se3.recover.lattice_factors(prev[0], 0.01, 0.01, (180.0,))
        pool = L._compose(rots, trans, info["top_idx"])
        cand, score, d = info["candidates"], info["color_score"], info["depth_chosen"]
        # the pool and its depth records are formed as without the switch, and without it the result is the depth winner's bytes
        assert d == 0 and np.array_equal(info["top_idx"], ip["top_idx"]) and info["top_fit"].tobytes() == ip["top_fit"].tobytes()
        assert info["final_fit"].tobytes() == info["top_fit"].tobytes() and np.array_equal(plain[0], pool[d])
        assert np.array_equal(cand, np.flatnonzero(info["final_fit"]["inlier_pts"] >= 0.9 * int(info["final_fit"]["inlier_pts"][d]))) and d in cand
        others = np.setdiff1d(np.arange(len(pool)), cand)
        assert not score[others].any() and not info["color_fit"][others]["px"].any()
        # the scores of the pool are the oracle's, to the last bit: the oracle renderer, the loop, utils.color_score
        want_fit, want_col = oracle_records(se3, pool[cand])
        assert np.array_equal(info["color_fit"][cand], want_col)
        assert np.array_equal(score[cand], np.atleast_1d(se3.utils.color_score(want_col, 64)))
        assert info["chosen"] in cand and score[info["chosen"]] == score[cand].max() and np.array_equal(out[0], pool[info["chosen"]])
        assert info["hidden_pts"] == int(info["final_fit"]["hidden_pts"][info["chosen"]])
        print("recover among the plate: depth alone chose %d (%.1f deg from the truth), colour chose %d (%.1f deg); scores %s over candidates %s"
              % (d, CS.rotation_error_deg(plain[0]), info["chosen"], CS.rotation_error_deg(out[0]), np.round(score[cand], 3), cand))
        return plain, ip, out, info, pool, (want_fit, want_col)

    plain, ip, out, info, pool, (want_fit, want_col) = both(poses)
    cand, score = info["candidates"], info["color_score"]
    assert (score[cand] < 0).all()                                                # every depth-equal member of this pool is colour-wrong
    # (2) last seen half a turn about the camera's x axis off: the lattice holds the true pose
    seen_last = CS.true_pose()
    seen_last[:3, :3] = np.diag([1.0, -1.0, -1.0]) @ seen_last[:3, :3]
    _, _, out2, info2, _, _ = both(np.stack([seen_last, VS.plate_pose()]))
    assert CS.rotation_error_deg(out2[0]) < 1 and info2["color_score"][info2["chosen"]] > 0
    assert np.linalg.norm(out2[0][:3, 3] - CS.true_pose()[:3, 3]) <= 0.01
    # (3) the choice on [half-turned, true] with equal depth records
    pair = np.stack([CS.flipped_pose(), CS.true_pose()])
    equal_fit = np.zeros(2, se3._lib.SCENE_POINT_FIT_DTYPE)
    equal_fit["points"], equal_fit["inlier_pts"] = 200, 100
    chosen = {}
    for rule, sc in (("plain", None), ("scene", device_scene)):
        picked = dict(chosen=0)
        chosen[rule] = L._choose_by_colour(picked, pair, equal_fit, rgb, depth, VS.STOL, 0.9, scene=sc)
        assert picked["depth_chosen"] == 0 and list(picked["candidates"]) == [0, 1]
    assert chosen == dict(plain=0, scene=1)
    # MultiTracker.verify composes the same scene from its own objects
    fit_v, col_v, score_v = mt.verify(0, pool[cand], rgb, depth, poses[1:], tol_mm=VS.STOL)
    assert np.array_equal(fit_v, want_fit) and np.array_equal(col_v, want_col) and np.array_equal(score_v, score[cand])
    with pytest.raises(ValueError, match="occluders"):
        mt.verify(0, pool[cand], rgb, depth, poses[:1], occluders=[0])
    # the live front end hands the switch through
    seen = []
    monkeypatch.setattr(mt, "recover", lambda *a, **k: seen.append(k) or np.asarray(a[0]).copy())
    lmt = se3.LiveMultiTracker(mt, poses, recover_lost=dict(lost_below=1.1, min_visible=0.0, refine=0, colour=True, colour_within=0.8))
    lmt.grab_depth(depth)
    lmt.grab_color(np.ascontiguousarray(rgb[:, :, ::-1]), stamp=1.0)
    assert len(lmt.on_track()) == 2
    assert len(seen) == 1 and seen[0]["colour"] is True and seen[0]["colour_within"] == 0.8 and seen[0]["refine"] == 0
    monkeypatch.undo()
    mt.close()
