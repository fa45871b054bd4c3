"""GPU: the lattice search among tracked objects -- se3tn_score_pose_grid_scene, se3tn_search_pose_grid_scene_host,
Engine.score_pose_grid(scene=...), Engine.search_pose_grid_scene, MultiTracker.recover, LiveMultiTracker(recover_lost=...).

The yardstick is the numpy oracle of tests/scene_search_oracle.py (the rule of include/se3tracknet.h in float64, in the stated operation
order, held to a per-point loop and to the plain oracle by tests/test_scene_search_host.py), never the library.  The arithmetic is IEEE
float64 with no contraction on both sides and every counter is an integer sum, so the expectation is EXACT EQUALITY of every counter
and of every ranked index: there is no tolerance in this file.  The scene is that of tests/scene_search_scene.py.  Without the feature
every test fails: the symbols and attributes do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_fit_scene as CS
import scene_search_oracle as SSO
import scene_search_scene as SS
from test_gpu_scene_fit import Mapped, dev16

pytestmark = pytest.mark.gpu

TOL = SS.TOL
LOST = 1                                   # the object order is SS.NAMES: T, L, O


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, max_batch=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(se3):
    """the scene, the default lattice around the place L was last seen, and the oracle's winner on the oracle's scene (CPU test 4)"""
    P = SS.poses()
    pts, nrm = SS.slab_model()
    depth = SS.frame()
    rots, trans = se3.recover.lattice_factors(P["last"], 0.05, SS.TRANS_STEP, (15.0,))
    best = int(SSO.rank(SSO.score(pts, nrm, rots, trans, depth, SS.scene(), SS.K, TOL, 1), 1)[0])
    rng = np.random.default_rng(9)
    return dict(P=P, pts=pts, nrm=nrm, depth=depth, rots=rots, trans=trans, best=best,
                poses=np.stack([P["T"], P["last"], P["O"]]), rgb=rng.integers(0, 256, SS.HW + (3,), dtype=np.uint8))


def same_records(got, want, what):
    assert got.dtype.names == SSO.FIELDS and got.shape == want.shape, what
    for k in SSO.FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])


def compose(rots, trans, i):
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = rots[i // len(trans)], trans[i % len(trans)]
    return G


# ---- 1. the device entry ------------------------------------------------------------------------------------------------------------
def test_device_entry_equals_the_oracle_word_for_word(se3, eng):
    """SS.device_case(): P = 1,100 (a full point tile and a 76-point tail), 19 translations (a full tile and a tail that leaves a wave
    idle, one behind the camera), 3 rotations (one with a NaN), both facing values, tol 1 and 30, the 24 x 32 frame with a scene that
    holds 0, 100, 101, 1999, 2000 and sits on both sides of s == m + tol."""
    case = SS.device_case()
    pts, nrm, rots, trans, depth, K = case
    assert len(pts) == 1100 and len(trans) == 19 and len(rots) == 3
    mp = eng.model_points(pts, nrm)
    lib = eng.lib
    n = len(rots) * len(trans)
    for tol in (1, 30):
        scene, marks = SS.boundary_scene(case, tol)
        assert scene[marks[0][0]] == marks[0][1] + tol and scene[marks[1][0]] == marks[1][1] + tol + 1
        for facing in (0, 1):
            want = SSO.score(pts, nrm, rots, trans, depth, scene, K, tol, facing)
            SSO.check_invariants(want, len(pts), tol, facing)
            got = eng.score_pose_grid(mp, rots, trans, depth, K, tol, facing=bool(facing), scene=scene)
            assert got.dtype == se3._lib.SCENE_POINT_FIT_DTYPE
            same_records(got, want, (tol, facing))
            assert want["hidden_pts"].max() > 0 and want["inlier_pts"].max() > 0 and (want["in_frame_pts"][3::19] == 0).all()
            assert (want["in_frame_pts"][2 * 19:] == 0).all()                            # the rotation with the NaN
            # the best k on the device (se3tn_rank_poses reads these records through a cast)
            idx, top = eng.score_pose_grid(mp, rots, trans, depth, K, tol, facing=bool(facing), scene=scene, top=5)
            assert np.array_equal(idx, SSO.rank(want, 5)) and top.tobytes() == want[idx].tobytes()
            # an all-zero scene: the words of se3tn_score_pose_grid on the device
            none = eng.score_pose_grid(mp, rots, trans, depth, K, tol, facing=bool(facing), scene=np.zeros_like(depth))
            plain = eng.score_pose_grid(mp, rots, trans, depth, K, tol, facing=bool(facing))
            assert plain.dtype == se3._lib.POINT_FIT_DTYPE and none.tobytes() == plain.tobytes(), (tol, facing)
            # records in mapped pinned host memory: every word stored once, the same words
            m = Mapped(32 * n)
            try:
                r_d, t_d = torch.from_numpy(rots.reshape(-1, 9)).cuda(), torch.from_numpy(trans).cuda()
                d_d, s_d = dev16(depth), dev16(scene)
                Kh = np.ascontiguousarray(K.reshape(9))
                rc = lib.se3tn_score_pose_grid_scene(eng._h, mp._h, len(rots), C.c_void_p(r_d.data_ptr()), len(trans), C.c_void_p(t_d.data_ptr()),
                                                     C.c_void_p(d_d.data_ptr()), C.c_void_p(s_d.data_ptr()), depth.shape[0], depth.shape[1],
                                                     Kh.ctypes.data_as(C.POINTER(C.c_double)), tol, facing, m.d, None)
                assert rc == 0, lib.se3tn_last_error()
                torch.cuda.synchronize()
                assert m.read().tobytes() == want.tobytes(), (tol, facing, "mapped")
            finally:
                m.close()
    # tensors in, tensors out; a NULL scene is refused and the context stays usable
    got_t = eng.score_pose_grid(mp, r_d, t_d, d_d, K, 30, facing=True, scene=s_d)
    assert torch.is_tensor(got_t) and got_t.cpu().numpy().view(se3._lib.SCENE_POINT_FIT_DTYPE).reshape(-1).tobytes() == want.tobytes()
    rc = lib.se3tn_score_pose_grid_scene(eng._h, mp._h, 3, C.c_void_p(r_d.data_ptr()), 19, C.c_void_p(t_d.data_ptr()), C.c_void_p(d_d.data_ptr()),
                                         None, 24, 32, Kh.ctypes.data_as(C.POINTER(C.c_double)), 30, 1, C.c_void_p(got_t.data_ptr()), None)
    assert rc == -1 and b"NULL" in lib.se3tn_last_error()
    same_records(eng.score_pose_grid(mp, rots, trans, depth, K, 30, facing=True, scene=scene), want, "after a refusal")
    mp.close()


# ---- 2. the one-call host entry -----------------------------------------------------------------------------------------------------
def test_one_call_host_entry_on_the_scene(se3, eng, world):
    """T and O as occluders, the default lattice around L's last place: the indices and records are the oracle's on the scene frame
    Engine.scene_fit composes of the same occluders, the occluders' records are scene_fit's, and the winner is the oracle's winner
    on the oracle's scene -- the true place of L."""
    w = world
    slab = se3.HipRenderer(eng, SS.slab_mesh())
    objs = [(slab, SS.OBJECT_WIDTH_MM)] * 2
    occ_poses = np.stack([w["P"]["T"], w["P"]["O"]])
    mp = eng.model_points(w["pts"], w["nrm"])
    rec, _, scene = eng.scene_fit(objs, occ_poses, w["depth"], SS.K, tol_mm=TOL, scene=True)
    assert scene.dtype == np.uint16 and (scene > 0).sum() > 3000
    want = SSO.score(w["pts"], w["nrm"], w["rots"], w["trans"], w["depth"], scene, SS.K, TOL, 1)
    idx, fit, occ_fit, kept = eng.search_pose_grid_scene(mp, w["rots"], w["trans"], w["depth"], SS.K, objs, occ_poses, tol_mm=TOL, facing=True,
                                                         top=8, keep_scene=True)
    assert idx.dtype == np.int32 and np.array_equal(idx, SSO.rank(want, 8))
    assert fit.dtype == se3._lib.SCENE_POINT_FIT_DTYPE and fit.tobytes() == want[idx].tobytes()
    assert occ_fit.dtype == se3._lib.SCENE_FIT_DTYPE and np.array_equal(occ_fit, rec)
    assert np.array_equal(kept.cpu().numpy().view(np.uint16), scene)                     # the scene the search read
    assert int(idx[0]) == w["best"]
    assert np.linalg.norm(compose(w["rots"], w["trans"], int(idx[0]))[:3, 3] - w["P"]["L"][:3, 3]) < 1e-9     # the true place of L
    assert int(fit["hidden_pts"][0]) > int(fit["inlier_pts"][0]) > 0
    # without the occluders' records, without facing, one occluder: the same rule
    i2, f2, o2 = eng.search_pose_grid_scene(mp, w["rots"][:2], w["trans"][:40], w["depth"], SS.K, objs[:1], occ_poses[:1], tol_mm=TOL,
                                            facing=False, top=3)
    rec1, _, scene1 = eng.scene_fit(objs[:1], occ_poses[:1], w["depth"], SS.K, tol_mm=TOL, scene=True)
    want1 = SSO.score(w["pts"], None, w["rots"][:2], w["trans"][:40], w["depth"], scene1, SS.K, TOL, 0)
    assert np.array_equal(i2, SSO.rank(want1, 3)) and f2.tobytes() == want1[i2].tobytes() and np.array_equal(o2, rec1)
    # a refusal (a pose behind the camera) leaves the context usable
    bad = occ_poses.copy()
    bad[1, 2, 3] = -0.5
    with pytest.raises(se3._lib.Se3tnError, match="not in front"):
        eng.search_pose_grid_scene(mp, w["rots"], w["trans"], w["depth"], SS.K, objs, bad, tol_mm=TOL)
    i3, f3, _ = eng.search_pose_grid_scene(mp, w["rots"], w["trans"], w["depth"], SS.K, objs, occ_poses, tol_mm=TOL, top=8)
    assert np.array_equal(i3, idx) and f3.tobytes() == fit.tobytes()
    mp.close()


# ---- 3 and 4: the trackers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_tracker(se3, tmp_path_factory):
    """random-init fixture weights, max_samples = 8, the slab's cloud and normals (color_fit_scene.make_tracker)"""
    return CS.make_tracker(se3, tmp_path_factory.mktemp("scene_search"))


def test_a_search_leaves_tracking_and_the_fit_records_alone(se3, world, slab_tracker):
    """MultiTracker.on_track before and after a scene search returns the same bits; se3tn_last_fit is unchanged by a search in
    between; and a second search over a larger grid, which grows the staging, repeats the first one's records for the candidates
    the two share."""
    w = world
    mt = se3.MultiTracker([slab_tracker] * 3)
    mt.fit_check = TOL
    handle = slab_tracker._facing_handle(None, "test")
    occ = [(slab_tracker.renderer, SS.OBJECT_WIDTH_MM)] * 2
    occ_poses = w["poses"][[0, 2]]
    first = mt.on_track(w["poses"], w["rgb"], w["depth"]).copy()
    fit_before = mt.engine.last_fit(3).copy()
    idx, fit, occ_fit = mt.engine.search_pose_grid_scene(handle, w["rots"], w["trans"], w["depth"], SS.K, occ, occ_poses, tol_mm=TOL, top=8)
    assert np.array_equal(mt.engine.last_fit(3), fit_before)
    again = mt.on_track(w["poses"], w["rgb"], w["depth"])
    assert np.array_equal(again, first) and np.array_equal(mt.engine.last_fit(3), fit_before)
    # 900 more translations, all behind the camera (they score nothing): a larger staging, the same winners
    extra = np.column_stack([np.zeros(900), np.zeros(900), -1.0 - np.arange(900) * 1e-3])
    wide = np.concatenate([w["trans"], extra])
    idx2, fit2, occ2 = mt.engine.search_pose_grid_scene(handle, w["rots"], wide, w["depth"], SS.K, occ, occ_poses, tol_mm=TOL, top=8)
    assert fit2.tobytes() == fit.tobytes() and np.array_equal(occ2, occ_fit)
    assert np.array_equal(idx2 // len(wide), idx // len(w["trans"])) and np.array_equal(idx2 % len(wide), idx % len(w["trans"]))
    assert np.array_equal(mt.on_track(w["poses"], w["rgb"], w["depth"]), first)
    mt.close()


def key(rec):
    return (int(rec["inlier_pts"]), -int(rec["behind_pts"]))


def test_multitracker_recover_among_the_tracked_objects(se3, world, slab_tracker, monkeypatch):
    """Random-init weights.  refine=0: the pose returned for the lost slab is the scene-aware winner of the lattice (the oracle's, on
    the scene Engine.scene_fit composes of T and O at their given poses), the other rows are untouched, last_recover carries the
    stated keys; lost=[] calls nothing; without scene records ValueError.  refine=1: the chosen pose's key is at least the refine=0
    key (random weights guarantee no more).  LiveMultiTracker(recover_lost=...) adopts what recover returns; without it, no call."""
    w = world
    mt = se3.MultiTracker([slab_tracker] * 3)
    with pytest.raises(ValueError, match="scene_check"):
        mt.recover(w["poses"], w["rgb"], w["depth"], lost=[LOST])
    mt.scene_check = TOL
    mt.on_track(w["poses"], w["rgb"], w["depth"])
    # random weights move every estimate off its object, so the records on_track left call all three lost; the records a tracker
    # with trained weights would leave are those at the poses themselves: T and O tracked
    mt.last_prediction["scene_fit"] = mt.scene_fit(w["poses"], w["depth"], tol_mm=TOL)
    status = se3.utils.scene_status(mt.last_prediction["scene_fit"], 0.5, 0.2)
    assert status[0] == "tracked" and status[2] == "tracked", (status, mt.last_prediction["scene_fit"])
    # the expectation, from the oracle alone
    cloud, normals = np.asarray(slab_tracker.object_cloud.points, np.float64), slab_tracker.object_normals
    occ = [(slab_tracker.renderer, SS.OBJECT_WIDTH_MM)] * 2
    _, _, scene = mt.engine.scene_fit(occ, w["poses"][[0, 2]], w["depth"], SS.K, tol_mm=TOL, scene=True)
    want = SSO.score(cloud, normals, w["rots"], w["trans"], w["depth"], scene, SS.K, TOL, 1)
    best = SSO.rank(want, 8)
    assert int(best[0]) == w["best"]
    out = mt.recover(w["poses"], w["rgb"], w["depth"], lost=[LOST], refine=0)
    assert out.shape == (3, 4, 4) and np.array_equal(out[[0, 2]], w["poses"][[0, 2]])
    assert np.array_equal(out[LOST], compose(w["rots"], w["trans"], int(best[0])))
    assert np.linalg.norm(out[LOST][:3, 3] - w["P"]["L"][:3, 3]) < 1e-9                  # the true place of L
    info = mt.last_recover[LOST]
    assert set(mt.last_recover) == {LOST}
    assert {"n", "top_idx", "top_fit", "refined", "final_fit", "chosen", "inlier_frac", "occluders", "hidden_pts", "visible_frac"} <= set(info)
    assert info["occluders"] == [0, 2] and info["n"] == 9317 and info["refined"] is None and info["chosen"] == 0
    assert np.array_equal(info["top_idx"], best) and info["top_fit"].tobytes() == want[best].tobytes()
    rec0 = want[best[0]]
    assert info["hidden_pts"] == int(rec0["hidden_pts"]) > 0
    assert info["inlier_frac"] == int(rec0["inlier_pts"]) / int(rec0["points"])
    assert info["visible_frac"] == int(rec0["inlier_pts"]) / (int(rec0["points"]) - int(rec0["hidden_pts"]))
    # refine=1 and align: the pool holds the lattice's best, the choice is made under the scene rule
    for kw in (dict(refine=1), dict(refine=1, align=5)):
        out1 = mt.recover(w["poses"], w["rgb"], w["depth"], lost=[LOST], **kw)
        i1 = mt.last_recover[LOST]
        assert len(i1["final_fit"]) == 8 * (2 + ("align" in kw)) and i1["final_fit"].dtype == se3._lib.SCENE_POINT_FIT_DTYPE
        assert key(i1["final_fit"][i1["chosen"]]) >= key(rec0), kw
        assert i1["final_fit"][-8:].tobytes() == want[best].tobytes()                    # the unrefined part, rescored against the kept scene
        assert np.array_equal(out1[[0, 2]], w["poses"][[0, 2]])
    # lost=[]: nothing is called
    calls = []
    monkeypatch.setattr(mt.engine, "search_pose_grid_scene", lambda *a, **k: calls.append("search"))
    monkeypatch.setattr(mt.engine, "score_pose_grid", lambda *a, **k: calls.append("score"))
    none = mt.recover(w["poses"], w["rgb"], w["depth"], lost=[])
    assert np.array_equal(none, w["poses"]) and mt.last_recover == {} and calls == []
    # the live front end: off by default, not one call more; on: what recover returns is adopted
    monkeypatch.setattr(mt, "recover", lambda *a, **k: calls.append("recover") or np.asarray(a[0]).copy())
    bgr = np.ascontiguousarray(w["rgb"][:, :, ::-1])
    for opts in (None, dict(lost_below=1.1, min_visible=0.0, refine=0)):                  # 1.1: every object that is not occluded is "lost"
        lmt = se3.LiveMultiTracker(mt, w["poses"], recover_lost=opts)
        lmt.grab_depth(w["depth"])
        lmt.grab_color(bgr, stamp=1.0)
        assert len(lmt.on_track()) == 3
        assert calls == ([] if opts is None else ["recover"])
    monkeypatch.undo()
    mt.close()
