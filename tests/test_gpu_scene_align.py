"""GPU: the pose alignment among tracked objects -- se3tn_align_poses_scene, se3tn_align_poses_scene_host,
Engine.align_poses(scene=...), MultiTracker.align, MultiTracker.recover(scene_align=True).

The yardstick is the numpy oracle of tests/scene_align_oracle.py (the rule of include/se3tracknet.h in float64, in the stated operation
order, held to a per-point loop, to the plain oracle and to the host build of the kernel's own statements by
tests/test_scene_align_host.py), never the library.  The arithmetic is IEEE float64 with no contraction on both sides and every sum is
an integer, so the expectation is EXACT EQUALITY of every pose (bytes), record and sum: there is no tolerance in this file except the
stated distance to the true pose.  Without the feature every test fails: the symbols, the keywords and the attributes do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_fit_scene as CS
import pose_align_oracle as PAO
import scene_align_oracle as SAO
import scene_align_scene as AS
import scene_search_scene as SS
from test_gpu_scene_fit import dev16

pytestmark = pytest.mark.gpu

LOST = 1                                   # the object order is SS.NAMES: T, L, O
FINITE = 8                                 # AS.device_poses: the first 8 poses are finite (the host entry refuses the others)


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small():
    """SS.device_case() as an alignment case: 1,100 points (past four strides of 256 threads, a tail that is no multiple of 64), 12
    poses (a NaN rotation and a translation behind the camera among them), the 24 x 32 frame and its boundary scene for tol 10"""
    case = SS.device_case()
    pts, nrm, _, _, depth, K = case
    scene, _ = SS.boundary_scene(case, 10)
    return dict(pts=pts, nrm=nrm, poses=AS.device_poses(case), depth=depth, scene=scene, K=K, tol=10)


def same(got, want, what):
    for name, g, w in zip(("poses", "records", "sums"), got, want):
        g = np.asarray(g)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()]
            raise AssertionError((what, name, bad[:8], g[bad[0]], w[bad[0]]))


def on_device(se3, eng, mp, poses, depth, scene, K, tol, **prm):
    """se3tn_align_poses_scene on uploaded copies -> (poses, records, sums) as numpy arrays (the device entry does not inspect the poses)"""
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4))
    out, rec, sums = eng.align_poses(mp, torch.from_numpy(poses).cuda(), dev16(depth), K, sums=True, scene=dev16(scene), scene_tol_mm=tol, **prm)
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (len(poses), 40)
    return out.cpu().numpy(), rec.cpu().numpy().view(se3._lib.SCENE_ALIGN_REC_DTYPE).reshape(len(poses)), sums.cpu().numpy()


# ---- 1. every word equals the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, 257, 1100])
def test_device_and_host_entries_equal_the_oracle(se3, eng, small, P):
    """P points (a slice of the case's) x iters in (1, 3, 20) x n in (1, 7, 12): the device entry on all poses, the host entry on the
    finite ones, with and without the sums; a cuda scene beside numpy poses goes through the device entry."""
    c = small
    pts, nrm = np.ascontiguousarray(c["pts"][:P]), np.ascontiguousarray(c["nrm"][:P])
    mp = eng.model_points(pts, nrm)
    hidden = 0
    for iters in (1, 3, 20):
        prm = dict(AS.DEFAULTS, iters=iters, min_pairs=6)
        want = SAO.align(pts, nrm, c["poses"], c["depth"], c["scene"], c["K"], c["tol"], **prm)
        assert (want[1]["pairs"] + want[1]["hidden_pts"] <= want[1]["facing_pts"]).all()
        hidden += int(want[1]["hidden_pts"].sum())
        for n in (1, 7, 12):
            got = on_device(se3, eng, mp, c["poses"][:n], c["depth"], c["scene"], c["K"], c["tol"], **prm)
            same(got, [w[:n] for w in want], (P, iters, n))
            m = min(n, FINITE)
            host = eng.align_poses(mp, c["poses"][:m], c["depth"], c["K"], sums=True, scene=c["scene"], scene_tol_mm=c["tol"], **prm)
            assert host[1].dtype == se3._lib.SCENE_ALIGN_REC_DTYPE
            same(host, [w[:m] for w in want], ("host", P, iters, n))
        two = eng.align_poses(mp, c["poses"][:7], c["depth"], c["K"], scene=c["scene"], scene_tol_mm=c["tol"], **prm)       # sums NULL
        assert len(two) == 2 and two[0].tobytes() == want[0][:7].tobytes() and two[1].tobytes() == want[1][:7].tobytes()
        mixed = eng.align_poses(mp, c["poses"][:7], c["depth"], c["K"], sums=True, scene=dev16(c["scene"]), scene_tol_mm=c["tol"], **prm)
        same(mixed, [w[:7] for w in want], ("numpy poses, cuda scene", P, iters))
    if P >= 63:
        assert hidden > 0
    mp.close()


def test_in_place_sentinels_no_sums_and_refusals_on_a_live_context(se3, eng, small):
    L, lib, c = se3._lib, eng.lib, small
    mp = eng.model_points(c["pts"], c["nrm"])
    n = 7
    H, W = c["depth"].shape
    prm_kw = dict(AS.DEFAULTS, min_pairs=6)
    want = SAO.align(c["pts"], c["nrm"], c["poses"][:n], c["depth"], c["scene"], c["K"], c["tol"], **prm_kw)
    Kp = np.ascontiguousarray(c["K"].reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    prm = L.AlignParams(20, 20, 6, 0, 1e-6, 1e-6)
    depth_d, scene_d = dev16(c["depth"]), dev16(c["scene"])
    io = torch.full((n + 1, 16), -7.25, dtype=torch.float64, device="cuda")
    io[:n] = torch.from_numpy(c["poses"][:n].reshape(n, 16))
    rec = torch.full((n + 1, 40), 0x5A, dtype=torch.uint8, device="cuda")
    sums = torch.full((n + 1, 28), -99, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.se3tn_align_poses_scene(eng._h, mp._h, n, vp(io), vp(depth_d), vp(scene_d), H, W, Kp, C.byref(prm), c["tol"], vp(io), vp(rec),
                                       vp(sums), st) == 0, lib.se3tn_last_error()
    torch.cuda.synchronize()
    same((io[:n].cpu().numpy().reshape(n, 4, 4), rec[:n].cpu().numpy().view(L.SCENE_ALIGN_REC_DTYPE).reshape(n), sums[:n].cpu().numpy()), want,
         "in place")
    assert (io[n] == -7.25).all() and (rec[n] == 0x5A).all() and (sums[n] == -99).all()
    poses_d = torch.from_numpy(c["poses"][:n].copy()).cuda()
    out2 = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    assert lib.se3tn_align_poses_scene(eng._h, mp._h, n, vp(poses_d), vp(depth_d), vp(scene_d), H, W, Kp, C.byref(prm), c["tol"], vp(out2), vp(rec),
                                       None, st) == 0
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == want[0].tobytes() and rec[:n].cpu().numpy().tobytes() == want[1].tobytes()
    # refusals leave the context usable
    for kw, word in ((dict(scene=None), b"NULL"), (dict(tol=0), b"scene_tol_mm"), (dict(tol=65536), b"scene_tol_mm")):
        rc = lib.se3tn_align_poses_scene(eng._h, mp._h, n, vp(poses_d), vp(depth_d), kw.get("scene", vp(scene_d)), H, W, Kp, C.byref(prm),
                                         kw.get("tol", c["tol"]), vp(out2), vp(rec), None, st)
        assert rc == -1 and word in lib.se3tn_last_error(), kw
    with pytest.raises(L.Se3tnError, match="scene_tol_mm"):
        eng.align_poses(mp, c["poses"][:n], c["depth"], c["K"], scene=c["scene"], scene_tol_mm=0)
    with pytest.raises(L.Se3tnError, match="rc=-1.*pose 8"):
        eng.align_poses(mp, c["poses"][:9], c["depth"], c["K"], scene=c["scene"])          # the host entry inspects the poses
    with pytest.raises(ValueError, match="shape"):
        eng.align_poses(mp, c["poses"][:n], c["depth"], c["K"], scene=c["scene"][:-1])
    same(eng.align_poses(mp, c["poses"][:n], c["depth"], c["K"], sums=True, scene=c["scene"], scene_tol_mm=c["tol"], **prm_kw), want,
         "after the refusals")
    mp.close()


# ---- 2. an all-zero scene, and the plain path after a scene-aware call -----------------------------------------------------------------------
def test_an_all_zero_scene_is_se3tn_align_poses_and_the_plain_path_is_left_alone(se3, small):
    """On ONE fresh context: the plain alignment first (the bits of a context that never saw the feature), then the scene-aware one
    with an all-zero scene -- every byte of pose, record and sums equal --, then with the boundary scene, then the plain one again:
    the bits of the first call, device entry and host entry alike, records of ALIGN_REC_DTYPE with _reserved 0."""
    L, c = se3._lib, small
    e = se3.Engine(0, 1)
    mp = e.model_points(c["pts"], c["nrm"])
    prm = dict(AS.DEFAULTS, min_pairs=6)
    depth_d, poses_d = dev16(c["depth"]), torch.from_numpy(c["poses"].copy()).cuda()

    def plain():
        out, rec, sums = e.align_poses(mp, poses_d, depth_d, c["K"], sums=True, **prm)
        host = e.align_poses(mp, c["poses"][:FINITE], c["depth"], c["K"], sums=True, **prm)
        assert host[1].dtype == L.ALIGN_REC_DTYPE and len(e.align_poses(mp, c["poses"][:FINITE], c["depth"], c["K"], **prm)) == 2
        return (out.cpu().numpy(), rec.cpu().numpy().view(L.ALIGN_REC_DTYPE).reshape(-1), sums.cpu().numpy()), host

    first, first_host = plain()
    same(first, PAO.align(c["pts"], c["nrm"], c["poses"], c["depth"], c["K"], **prm), "plain, fresh context")
    zero = on_device(se3, e, mp, c["poses"], c["depth"], np.zeros_like(c["scene"]), c["K"], c["tol"], **prm)
    assert all(z.tobytes() == f.tobytes() for z, f in zip(zero, first)) and (zero[1]["hidden_pts"] == 0).all()
    zero_host = e.align_poses(mp, c["poses"][:FINITE], c["depth"], c["K"], sums=True, scene=np.zeros_like(c["scene"]), scene_tol_mm=c["tol"], **prm)
    assert all(z.tobytes() == f.tobytes() for z, f in zip(zero_host, first_host))
    full = on_device(se3, e, mp, c["poses"], c["depth"], c["scene"], c["K"], c["tol"], **prm)
    assert full[1]["hidden_pts"].max() > 0 and full[1].tobytes() != first[1].tobytes()
    e.align_poses(mp, c["poses"][:FINITE], c["depth"], c["K"], sums=True, scene=c["scene"], scene_tol_mm=c["tol"], **prm)
    again, again_host = plain()
    assert all(a.tobytes() == f.tobytes() for a, f in zip(again, first)) and (again[1]["_reserved"] == 0).all()
    assert all(a.tobytes() == f.tobytes() for a, f in zip(again_host, first_host))
    mp.close()
    e.close()


# ---- 3. a pose's output is the same in any call ----------------------------------------------------------------------------------------------
def test_a_pose_is_aligned_the_same_at_any_n_and_in_any_place(se3, eng, small):
    c = small
    mp = eng.model_points(c["pts"], c["nrm"])
    prm = dict(AS.DEFAULTS, min_pairs=6)
    args = (c["depth"], c["scene"], c["K"], c["tol"])
    full = on_device(se3, eng, mp, c["poses"], *args, **prm)
    again = on_device(se3, eng, mp, c["poses"], *args, **prm)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
    order = np.random.default_rng(3).permutation(len(c["poses"]))
    perm = on_device(se3, eng, mp, c["poses"][order], *args, **prm)
    assert all(p.tobytes() == np.ascontiguousarray(f[order]).tobytes() for p, f in zip(perm, full))
    for lo, hi in ((0, 1), (5, 9), (11, 12)):
        sub = on_device(se3, eng, mp, c["poses"][lo:hi], *args, **prm)
        assert all(s.tobytes() == np.ascontiguousarray(f[lo:hi]).tobytes() for s, f in zip(sub, full)), (lo, hi)
    mp.close()


# ---- 4. one linear stream capture -------------------------------------------------------------------------------------------------------------
def test_a_captured_scene_alignment_replays_with_a_changed_scene(se3, eng, small):
    L, c = se3._lib, small
    mp = eng.model_points(c["pts"], c["nrm"])
    n = 7
    H, W = c["depth"].shape
    poses_d, depth_d, scene_d = torch.from_numpy(c["poses"][:n].copy()).cuda(), dev16(c["depth"]), dev16(c["scene"])
    out_d = torch.zeros((n, 16), dtype=torch.float64, device="cuda")
    rec_d = torch.zeros((n, 40), dtype=torch.uint8, device="cuda")
    sums_d = torch.zeros((n, 28), dtype=torch.int64, device="cuda")
    Kp = np.ascontiguousarray(c["K"].reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    prm = L.AlignParams(20, 20, 6, 0, 1e-6, 1e-6)

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return eng.lib.se3tn_align_poses_scene(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()),
                                               C.c_void_p(scene_d.data_ptr()), H, W, Kp, C.byref(prm), c["tol"], C.c_void_p(out_d.data_ptr()),
                                               C.c_void_p(rec_d.data_ptr()), C.c_void_p(sums_d.data_ptr()), st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert enqueue() == 0                                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert enqueue() == 0                                                          # one launch
        with pytest.raises(L.Se3tnError, match="rc=-2"):                               # the host entry is synchronous: refused, the capture whole
            eng.align_poses(mp, c["poses"][:n], c["depth"], c["K"], scene=c["scene"])
    for turn in range(2):
        changed = np.ascontiguousarray(np.roll(c["scene"], turn + 1, axis=1))
        scene_d.copy_(torch.from_numpy(changed.view(np.int16)))
        out_d.zero_(); rec_d.zero_(); sums_d.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = SAO.align(c["pts"], c["nrm"], c["poses"][:n], c["depth"], changed, c["K"], c["tol"], **dict(AS.DEFAULTS, min_pairs=6))
        same((out_d.cpu().numpy().reshape(n, 4, 4), rec_d.cpu().numpy().view(L.SCENE_ALIGN_REC_DTYPE).reshape(n), sums_d.cpu().numpy()), want,
             ("replay", turn))
    mp.close()


# ---- 5. the stacked scene ---------------------------------------------------------------------------------------------------------------------
def test_stacked_scene_forty_perturbations_equal_the_oracle(se3, eng):
    """(poses, records, sums) of the 40 perturbations under both rules, device entry and host entry: the oracle's, whose distances to
    the truth tests/test_scene_align_host.py holds to the bound (0 of 40 plain, at least 38 of 40 under the scene rule)."""
    pts, nrm = SS.slab_model()
    depth, scene, poses = AS.stacked_frame(0), AS.stacked_scene(), AS.perturbed(40)
    want = AS.stacked_aligned(0)
    mp = eng.model_points(pts, nrm)
    same(on_device(se3, eng, mp, poses, depth, scene, AS.K, AS.TOL, **AS.DEFAULTS), want["scene"], "device")
    same(eng.align_poses(mp, poses, depth, AS.K, sums=True, scene=scene, scene_tol_mm=AS.TOL, **AS.DEFAULTS), want["scene"], "host")
    same(eng.align_poses(mp, poses, depth, AS.K, sums=True, **AS.DEFAULTS), want["plain"], "plain")
    good, _ = AS.within(want["scene"][0], AS.stacked_poses()["L"])
    assert good.sum() >= 38 and AS.within(want["plain"][0], AS.stacked_poses()["L"])[0].sum() == 0
    mp.close()


# ---- 6. the trackers --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_tracker(se3, tmp_path_factory):
    """random-init fixture weights, max_samples = 8, the slab's cloud and normals (color_fit_scene.make_tracker)"""
    return CS.make_tracker(se3, tmp_path_factory.mktemp("scene_align"))


def test_multitracker_align_and_recover_with_scene_align(se3, slab_tracker, monkeypatch):
    """The scene of tests/scene_search_scene.py, L last seen off the lattice (+ (4, -3, 5) mm and 5 degrees about the camera's z).
    MultiTracker.align is Engine.align_poses(scene=...) on the scene scene_fit composes, and leaves tracking alone.
    recover(align=20, refine=0): by default the bits of the parent's path, taken by calling its pieces step by step, with plain
    records; with scene_align=True `aligned` is the scene-aware oracle's 8 poses bit for bit, the records carry hidden_pts, and the
    returned pose is the oracle's pool choice, within 2.9 mm / 1.85 degrees of the truth (measured: 1.12 mm / 1.23 degrees)."""
    L = se3._lib
    P = SS.poses()
    depth = SS.frame(0)
    rgb = np.random.default_rng(9).integers(0, 256, SS.HW + (3,), dtype=np.uint8)
    last = AS.off_node_last(True)
    poses = np.stack([P["T"], last, P["O"]])
    mt = se3.MultiTracker([slab_tracker] * 3)
    first = mt.on_track(poses, rgb, depth).copy()                                        # a fresh context's tracking bits
    cloud, normals = np.asarray(slab_tracker.object_cloud.points, np.float64), slab_tracker.object_normals
    handle = slab_tracker._facing_handle(None, "test")
    occ = [(slab_tracker.renderer, SS.OBJECT_WIDTH_MM)] * 2
    occ_poses = poses[[0, 2]]
    _, _, scene = mt.engine.scene_fit(occ, occ_poses, depth, SS.K, tol_mm=SS.TOL, scene=True)
    print("the composed scene equals the oracle's render: %s" % np.array_equal(scene, SS.scene()))
    # MultiTracker.align
    hyps = AS.perturbed(3)
    hyps[:, :3, 3] += P["L"][:3, 3] - AS.stacked_poses()["L"][:3, 3]                     # around L's place in THIS scene
    got = mt.align(LOST, hyps, depth, occ_poses, sums=True)
    direct = slab_tracker.engine.align_poses(handle, hyps, depth, SS.K, sums=True, scene=scene, scene_tol_mm=SS.TOL)
    assert got[1].dtype == L.SCENE_ALIGN_REC_DTYPE
    same(got, direct, "MultiTracker.align")
    same(got, SAO.align(cloud, normals, hyps, depth, scene, SS.K, SS.TOL, **AS.DEFAULTS), "MultiTracker.align, oracle")
    same(mt.align(LOST, hyps, depth, occ_poses, occluders=[0, 2], sums=True, iters=3),
         SAO.align(cloud, normals, hyps, depth, scene, SS.K, SS.TOL, **dict(AS.DEFAULTS, iters=3)), "occluders given")
    with pytest.raises(ValueError, match="occluders"):
        mt.align(LOST, hyps, depth, occ_poses, occluders=[LOST, 2])
    assert np.array_equal(mt.on_track(poses, rgb, depth), first)                         # tracking after scene-aware calls: the same bits
    # recover
    mt.scene_check = SS.TOL
    mt.on_track(poses, rgb, depth)
    mt.last_prediction["scene_fit"] = mt.scene_fit(poses, depth, tol_mm=SS.TOL)          # (as tests/test_gpu_scene_search.py: T and O tracked)
    status = se3.utils.scene_status(mt.last_prediction["scene_fit"], 0.5, 0.2)
    assert status[0] == "tracked" and status[2] == "tracked", status
    # the parent's path, piece by piece
    rots, trans = se3.recover.lattice_factors(last, 0.05, 0.01, (15.0,))
    top_idx, top_fit, _, kept = mt.engine.search_pose_grid_scene(handle, rots, trans, depth, SS.K, occ, occ_poses, tol_mm=SS.TOL, facing=True,
                                                                 top=8, keep_scene=True)
    unrefined = slab_tracker._compose(rots, trans, top_idx)
    p_aligned, p_rec = slab_tracker.engine.align_poses(handle, unrefined, depth, SS.K, iters=20)
    p_final = np.concatenate([p_aligned, unrefined])
    grid = mt.engine.score_pose_grid(handle, p_final[:, :3, :3], p_final[:, :3, 3], depth, SS.K, SS.TOL, facing=True, scene=kept)
    p_fit = grid[np.arange(16) * 17]
    p_chosen = int(np.argmax(se3.recover.pose_key(p_fit)))
    out = mt.recover(poses, rgb, depth, lost=[LOST], refine=0, align=20)
    info = mt.last_recover[LOST]
    assert info["scene_align"] is False and info["align_rec"].dtype == L.ALIGN_REC_DTYPE
    assert info["aligned"].tobytes() == p_aligned.tobytes() and info["align_rec"].tobytes() == p_rec.tobytes()
    assert info["final_fit"].tobytes() == p_fit.tobytes() and info["chosen"] == p_chosen and np.array_equal(out[LOST], p_final[p_chosen])
    assert np.array_equal(out[[0, 2]], poses[[0, 2]])
    e_plain = PAO.pose_error(out[LOST], P["L"])
    # scene_align=True
    want = SAO.align(cloud, normals, unrefined, depth, scene, SS.K, SS.TOL, **AS.DEFAULTS)
    w_final, w_fit, w_chosen = AS.pool_from(cloud, normals, unrefined, want[0], depth, scene)
    out2 = mt.recover(poses, rgb, depth, lost=[LOST], refine=0, align=20, scene_align=True)
    info = mt.last_recover[LOST]
    assert info["scene_align"] is True and info["align_rec"].dtype == L.SCENE_ALIGN_REC_DTYPE
    assert np.array_equal(info["top_idx"], top_idx) and info["aligned"].tobytes() == want[0].tobytes()
    assert info["align_rec"].tobytes() == want[1].tobytes() and info["align_rec"]["hidden_pts"].min() > 0
    assert info["final_fit"].tobytes() == w_fit.tobytes() and info["chosen"] == w_chosen and np.array_equal(out2[LOST], w_final[w_chosen])
    e_scene = PAO.pose_error(out2[LOST], P["L"])
    print("recover: plain alignment %.2f mm / %.2f deg from the truth, scene_align %.2f mm / %.2f deg" % (
        1000 * e_plain[0], e_plain[1], 1000 * e_scene[0], e_scene[1]))
    assert e_scene[0] <= AS.BOUND_M and e_scene[1] <= AS.BOUND_DEG and e_plain[0] > 0.015
    if np.array_equal(scene, SS.scene()):                                                # the oracle's own render: its pool choice, bit for bit
        assert np.array_equal(out2[LOST], AS.pool(True, True)["pose"]) and info["aligned"].tobytes() == AS.pool(True, True)["aligned"].tobytes()
    # scene_align without align changes nothing; the default afterwards is the parent's path again
    out3 = mt.recover(poses, rgb, depth, lost=[LOST], refine=0, scene_align=True)
    assert mt.last_recover[LOST]["scene_align"] is False and "aligned" not in mt.last_recover[LOST]
    assert np.array_equal(out3[LOST], unrefined[0])
    assert np.array_equal(mt.recover(poses, rgb, depth, lost=[LOST], refine=0, align=20), out)
    # the live front end passes the key through
    calls = []
    monkeypatch.setattr(mt, "recover", lambda *a, **k: calls.append(k) or np.asarray(a[0]).copy())
    lmt = se3.LiveMultiTracker(mt, poses, recover_lost=dict(lost_below=1.1, min_visible=0.0, refine=0, align=20, scene_align=True))
    lmt.grab_depth(depth)
    lmt.grab_color(np.ascontiguousarray(rgb[:, :, ::-1]), stamp=1.0)
    assert len(lmt.on_track()) == 3
    assert len(calls) == 1 and calls[0]["scene_align"] is True and calls[0]["align"] == 20
    monkeypatch.undo()
    mt.close()
