"""GPU: searching a product lattice of poses -- se3tn_points_set_normals, se3tn_score_pose_grid, se3tn_search_pose_grid_host,
Engine.score_pose_grid, Tracker.recover(facing=True), Tracker.acquire.

The yardstick is the numpy oracle of tests/pose_grid_oracle.py (the rule of include/se3tracknet.h in float64, in the stated operation
order, held to a per-point loop and to the oracle of se3tn_score_poses by tests/test_pose_grid_host.py), never the library.  The
arithmetic is IEEE float64 with no contraction on both sides and every counter is an integer sum, so the expectation is EXACT
EQUALITY of every counter and of every ranked index: there is no tolerance in this file.

Small cases: a 48 x 64 frame around 500 mm with holes and borderline values, a blob of P points whose normals point away from its
centre, random rotations, translations around (0, 0, 0.5).  The tracker tests use the scene of tests/pose_grid_scene.py.  Without the
feature every case fails: the symbols and attributes do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import pose_grid_oracle as PGO
import pose_grid_scene as SC
import pose_search_cases as PC
import pose_search_oracle as PSO
from oracle import fixtures as Fx
from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
H, W = PC.GRID_HW
K = PC.GRID_K
TOL = 5
TT = PC.GRID_TT                            # csrc/pose_grid_plan.h PG_TT: translations per workgroup
P_EDGES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]      # lanes of one wave, and the 1,024-point tile of LDS one short, full, one over, two and one
NT_EDGES = [1, TT - 1, TT, TT + 1, 3 * TT + 5]
NR_EDGES = [1, 3]


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
def depth():
    return PC.grid_depth()


@pytest.fixture(scope="module")
def factors():
    return PC.grid_factors()


blob = PC.blob


def same_records(got, want, what):
    assert got.dtype == PSO.DTYPE and got.shape == want.shape, what
    for k in PSO.FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])


# ---- 1. facing = 0: the words of se3tn_score_poses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_EDGES)
def test_without_facing_every_word_is_that_of_score_poses_on_the_composed_pose(se3, eng, depth, factors, P):
    pts, nrm = blob(P)
    mp = eng.model_points(pts)                                   # no normals: facing = 0 does not need them
    assert mp.normals is None and eng.lib.se3tn_points_has_normals(mp._h) == 0
    for n_rot in NR_EDGES:
        for n_trans in NT_EDGES:
            rots, trans = factors[0][:n_rot], factors[1][:n_trans]
            poses = PGO.compose(rots, trans)
            want = PSO.score(pts, poses, depth, K, TOL)
            assert np.array_equal(want, PGO.score(pts, None, rots, trans, depth, K, TOL, 0))
            got = eng.score_pose_grid(mp, rots, trans, depth, K, TOL)
            same_records(got, want, (P, n_rot, n_trans))
            assert got.tobytes() == eng.score_poses(mp, poses, depth, K, TOL).tobytes(), (P, n_rot, n_trans)
    assert want["inlier_pts"].max() > 0 and want["in_frame_pts"][7] == 0 and want["in_frame_pts"][11] == 0
    mp.close()


# ---- 2. facing = 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_EDGES)
def test_with_facing_the_records_equal_the_oracle(se3, eng, depth, factors, P):
    pts, nrm = blob(P)
    mp = eng.model_points(pts, nrm)
    assert np.array_equal(mp.normals, nrm) and eng.lib.se3tn_points_has_normals(mp._h) == 1
    for n_rot in NR_EDGES:
        for n_trans in NT_EDGES:
            rots, trans = factors[0][:n_rot], factors[1][:n_trans]
            want = PGO.score(pts, nrm, rots, trans, depth, K, TOL, 1)
            PGO.check_invariants(want, P, TOL, 1)
            got = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=True)
            same_records(got, want, (P, n_rot, n_trans))
    if P >= 63:   # the cases show what they are meant to show (on the oracle alone): about half the blob faces, and some of it is confirmed
        assert 0.3 * P < want["points"][0] < 0.7 * P and want["inlier_pts"].max() > 0
        plain = PGO.score(pts, nrm, rots, trans, depth, K, TOL, 0)
        assert (want["in_frame_pts"] <= plain["in_frame_pts"]).all() and want["front_pts"].sum() < plain["front_pts"].sum()
    # the normals can be replaced and removed; without them facing = 1 is a state error and facing = 0 still works
    flipped = eng.model_points(pts, -nrm)
    other = eng.score_pose_grid(flipped, factors[0][:1], factors[1][:2], depth, K, TOL, facing=True)
    same_records(other, PGO.score(pts, -nrm, factors[0][:1], factors[1][:2], depth, K, TOL, 1), "flipped")
    flipped.close()
    assert eng.lib.se3tn_points_set_normals(mp._h, None) == 0 and eng.lib.se3tn_points_has_normals(mp._h) == 0
    with pytest.raises(se3._lib.Se3tnError, match="rc=%d.*no normals" % E_STATE):
        eng.score_pose_grid(mp, factors[0][:1], factors[1][:2], depth, K, TOL, facing=True)
    same_records(eng.score_pose_grid(mp, factors[0][:1], factors[1][:2], depth, K, TOL),
                 PGO.score(pts, None, factors[0][:1], factors[1][:2], depth, K, TOL, 0), "normals removed")
    mp.close()


@pytest.mark.parametrize("hw", [(6, 6), (7, 7), (6, 7), (7, 6)])
def test_exact_boundaries_with_facing(se3, eng, hw):
    """Identity rotation (and a quarter turn about the optical axis), points at z = 1 and K = [[1, 0, 0.5], [0, 1, 1.5]]: u = x + 0.5 and
    v = y + 1.5 are exact, so points sit ON -0.5 (rounds to -0.0: inside), 0.5, W - 1.5 and W - 0.5 (to W for even W: outside).
    Normals: (0, 0, -1) faces (f = -c.z), (0, 0, 1) faces only BEHIND the camera (c.z <= 0: counted as a point, never in frame).  One
    point lies on the optical axis with the normal (1, 0, 0): f = (1 * 0 + 0 * 0) + 0 * c.z = 0 exactly, the grazing point, never
    counted.  Translations: none, half a millimetre (m rounds half to even), behind the camera, c.z = 0 exactly, and one with a NaN."""
    Hh, Ww = hw
    Kc = np.array([[1.0, 0, 0.5], [0, 1.0, 1.5], [0, 0, 1.0]])
    xs = [-1.0, 0.0, Ww - 2.0, Ww - 1.0]
    ys = [-2.0, -1.0, Hh - 3.0, Hh - 2.0]
    pts = np.array([(x, y, 1.0) for x in xs for y in ys] + [(1e18, 0.0, 1.0), (0.0, -1e300, 1.0), (0.0, 0.0, 1.0)])
    nrm = np.array([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0)] * 9 + [(1.0, 0.0, 0.0)])    # alternating; the last is the point on the axis
    assert len(pts) == 19 and len(nrm) == 19
    rots = np.array([np.eye(3), Rotation.from_euler("z", 90, degrees=True).as_matrix()])
    rots[1] = np.rint(rots[1])                                                     # an exact quarter turn
    trans = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0005), (0.0, 0.0, -2.0), (0.0, 0.0, -1.0), (np.nan, 0.0, 0.0)])
    tol = 7
    vals = np.array([0, 100, 101, 1999, 2000, 65535] + [1000 + s * (tol + e) for s in (-1, 1) for e in (-1, 0, 1)], np.uint16)
    mp = eng.model_points(pts, nrm)
    toward = int((nrm[:, 2] < 0).sum())
    for shift in range(len(vals)):
        depth = vals[(np.arange(Hh * Ww) + shift) % len(vals)].reshape(Hh, Ww)
        want = PGO.score(pts, nrm, rots, trans, depth, Kc, tol, 1)
        # by hand: in front of the camera exactly the (0, 0, -1) normals face -- the grazing point does not; behind it the (0, 0, 1)
        # ones do, and nothing is in frame; at c.z = 0 nothing faces (f = -+0); with a NaN nothing does
        assert want["points"][0] == toward and want["points"][2] == 18 - toward and want["in_frame_pts"][2] == 0
        assert want["points"][3] == 0 and want["points"][4] == 0 and want["in_frame_pts"][4] == 0
        got = eng.score_pose_grid(mp, rots, trans, depth, Kc, tol, facing=True)
        same_records(got, want, (hw, shift))
        PGO.check_invariants(got, len(pts), tol, 1)
        # the same points without the rule: every boundary point of test_gpu_pose_search's case is still where it was
        same_records(eng.score_pose_grid(mp, rots, trans, depth, Kc, tol), PSO.score(pts, PGO.compose(rots, trans), depth, Kc, tol), (hw, shift, 0))
    # every other record is untouched by the NaN translation: the grid without it gives the same words
    depth = vals[np.arange(Hh * Ww) % len(vals)].reshape(Hh, Ww)
    full = eng.score_pose_grid(mp, rots, trans, depth, Kc, tol, facing=True).reshape(2, 5)
    clean = eng.score_pose_grid(mp, rots, trans[:4], depth, Kc, tol, facing=True).reshape(2, 4)
    assert full[:, :4].tobytes() == clean.tobytes()
    mp.close()


# ---- 3. a record is the same in any grid -----------------------------------------------------------------------------------------------------
def test_a_record_is_the_same_in_any_grid(se3, eng, depth, factors):
    pts, nrm = blob(1025)
    rots, trans = factors
    mp = eng.model_points(pts, nrm)
    for facing in (False, True):
        full = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=facing)
        assert full.tobytes() == eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=facing).tobytes()     # on every run
        full = full.reshape(3, len(trans))
        for r0, r1, t0, t1 in ((0, 1, 0, len(trans)), (1, 3, 0, TT), (0, 3, TT - 1, TT + 2), (2, 3, 5, 6), (0, 2, 2 * TT + 1, len(trans))):
            sub = eng.score_pose_grid(mp, rots[r0:r1], trans[t0:t1], depth, K, TOL, facing=facing)
            assert sub.reshape(r1 - r0, t1 - t0).tobytes() == np.ascontiguousarray(full[r0:r1, t0:t1]).tobytes(), (facing, r0, r1, t0, t1)
        order_r, order_t = np.array([2, 0, 1]), np.random.default_rng(3).permutation(len(trans))
        perm = eng.score_pose_grid(mp, rots[order_r], trans[order_t], depth, K, TOL, facing=facing).reshape(3, len(trans))
        assert perm.tobytes() == np.ascontiguousarray(full[order_r][:, order_t]).tobytes(), facing
        for r, t in ((0, 0), (1, TT), (2, len(trans) - 1)):
            one = eng.score_pose_grid(mp, rots[r:r + 1], trans[t:t + 1], depth, K, TOL, facing=facing)
            assert one.tobytes() == full[r, t:t + 1].tobytes(), (facing, r, t)
        # a rotation that is not finite harms only its own candidates
        bad = rots.copy()
        bad[1, 0, 2] = np.inf
        got = eng.score_pose_grid(mp, bad, trans, depth, K, TOL, facing=facing).reshape(3, len(trans))
        assert got[0].tobytes() == full[0].tobytes() and got[2].tobytes() == full[2].tobytes() and (got[1]["in_frame_pts"] == 0).all()
        same_records(got.reshape(-1), PGO.score(pts, nrm, bad, trans, depth, K, TOL, int(facing)), ("inf rotation", facing))
    mp.close()


# ---- 4. rank and the host entry point ---------------------------------------------------------------------------------------------------------
def test_host_entry_point_rank_and_refusals(se3, eng, depth, factors):
    L, lib = se3._lib, eng.lib
    pts, nrm = blob(257)
    rots, trans = factors
    n_rot, n_trans = len(rots), len(trans)
    n = n_rot * n_trans
    mp = eng.model_points(pts, nrm)
    rots_d, trans_d = torch.from_numpy(rots.reshape(-1, 9)).cuda(), torch.from_numpy(trans).cuda()
    depth_d = torch.from_numpy(depth.view(np.int16)).cuda()
    for facing in (False, True):
        want = PGO.score(pts, nrm, rots, trans, depth, K, TOL, int(facing))
        fit_t = eng.score_pose_grid(mp, rots_d, trans_d, depth_d, K, TOL, facing=facing)                # tensors in, tensors out
        assert fit_t.is_cuda and fit_t.dtype == torch.int32 and tuple(fit_t.shape) == (n, 8)
        same_records(fit_t.cpu().numpy().view(PSO.DTYPE).reshape(n), want, ("device", facing))
        for k in (1, 8, 64):
            idx, fit = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=facing, top=k)        # the host entry point
            assert idx.dtype == np.int32 and np.array_equal(idx, PSO.rank(want, k)), (facing, k)
            same_records(fit, want[idx], (facing, k))
            idx_t, top_t = eng.score_pose_grid(mp, rots_d, trans_d, depth_d, K, TOL, facing=facing, top=k)   # se3tn_rank_poses on the device call's output
            assert np.array_equal(idx_t.cpu().numpy(), idx) and top_t.cpu().numpy().view(PSO.DTYPE).reshape(k).tobytes() == fit.tobytes()
    good = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=True, top=8)

    def still_right(what):
        got = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=True, top=8)
        assert np.array_equal(got[0], good[0]) and got[1].tobytes() == good[1].tobytes(), what

    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    idx, fit = np.full(64, -1, np.int32), np.zeros(64, L.POINT_FIT_DTYPE)
    hp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    r9 = np.ascontiguousarray(rots.reshape(-1, 9))

    def host(nr=n_rot, nt=n_trans, k=4, tol=TOL, fc=1):
        return lib.se3tn_search_pose_grid_host(eng._h, mp._h, nr, hp(r9), nt, hp(trans), hp(depth), H, W, Kp, tol, fc, k, hp(idx), hp(fit), None)

    assert host() == 0
    for kw in (dict(nr=0), dict(nt=0), dict(nr=2 ** 20, nt=2), dict(tol=0), dict(tol=65536), dict(fc=2), dict(k=0), dict(k=65), dict(nr=1, nt=3, k=4)):
        assert host(**kw) == E_ARG, kw
    still_right("after bad numbers")
    for bad in (np.nan, np.inf, -np.inf):
        broken = rots.copy()
        broken[1, 2, 0] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*rotation 1" % E_ARG):
            eng.score_pose_grid(mp, broken, trans, depth, K, TOL, facing=True, top=4)
        broken = trans.copy()
        broken[9, 1] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*translation 9" % E_ARG):
            eng.score_pose_grid(mp, rots, broken, depth, K, TOL, facing=True, top=4)
        Kb = K.copy()
        Kb[1, 1] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*K entry 4" % E_ARG):
            eng.score_pose_grid(mp, rots, trans, depth, Kb, TOL, facing=True, top=4)
        bad_n = nrm.copy()
        bad_n[200, 2] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*component 602" % E_ARG):
            eng.model_points(pts, bad_n)
        assert lib.se3tn_points_set_normals(mp._h, hp(bad_n)) == E_ARG and lib.se3tn_points_has_normals(mp._h) == 1   # the handle keeps what it had
    still_right("after inputs that are not finite")
    plain = eng.model_points(pts)
    with pytest.raises(L.Se3tnError, match="rc=%d" % E_STATE):
        eng.score_pose_grid(plain, rots, trans, depth, K, TOL, facing=True, top=4)
    plain.close()
    # the host variant waits for its stream: inside a capture it says so and leaves the capture whole
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(L.Se3tnError, match="rc=%d" % E_STATE):
            eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=True, top=4)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    still_right("after the refused capture")
    # the existing search shares the staging: it still gives its own answer afterwards
    poses = PGO.compose(rots, trans)
    i2, f2 = eng.score_poses(mp, poses, depth, K, TOL, top=8)
    w2 = PSO.score(pts, poses, depth, K, TOL)
    assert np.array_equal(i2, PSO.rank(w2, 8)) and f2.tobytes() == w2[i2].tobytes()
    still_right("after se3tn_search_poses_host")
    mp.close()


# ---- 5. one linear stream capture ------------------------------------------------------------------------------------------------------------
def test_a_captured_score_and_rank_replays_with_changed_depth(se3, eng, depth, factors):
    pts, nrm = blob(1025)
    rots, trans = factors
    n_rot, n_trans, k = len(rots), len(trans), 8
    n = n_rot * n_trans
    mp = eng.model_points(pts, nrm)
    rots_d, trans_d = torch.from_numpy(rots.reshape(-1, 9)).cuda(), torch.from_numpy(trans).cuda()
    depth_d = torch.from_numpy(depth.view(np.int16)).cuda()
    fit_d = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    idx_d = torch.zeros((k,), dtype=torch.int32, device="cuda")
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = eng.lib.se3tn_score_pose_grid(eng._h, mp._h, n_rot, C.c_void_p(rots_d.data_ptr()), n_trans, C.c_void_p(trans_d.data_ptr()),
                                           C.c_void_p(depth_d.data_ptr()), H, W, Kp, TOL, 1, C.c_void_p(fit_d.data_ptr()), st)
        return rc or eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()), st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert enqueue() == 0                                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert enqueue() == 0                                                          # two launches, one after the other
    for turn in range(2):
        changed = np.ascontiguousarray(np.roll(depth, 5 * turn + 3, axis=1) + np.uint16(2 * turn))
        depth_d.copy_(torch.from_numpy(changed.view(np.int16)))
        fit_d.zero_(); idx_d.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = PGO.score(pts, nrm, rots, trans, changed, K, TOL, 1)
        same_records(fit_d.cpu().numpy().view(PSO.DTYPE).reshape(n), want, ("replay", turn))
        assert np.array_equal(idx_d.cpu().numpy(), PSO.rank(want, k)), turn
        eager = eng.score_pose_grid(mp, rots, trans, changed, K, TOL, facing=True, top=k)
        assert np.array_equal(eager[0], idx_d.cpu().numpy()) and eager[1].tobytes() == want[eager[0]].tobytes()
    mp.close()


# ---- 6. Tracker.recover(facing=True) and Tracker.acquire ------------------------------------------------------------------------------------
def write_ply_with_normals(path, verts, normals):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % len(verts))
        f.write("".join("property double %s\n" % k for k in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n")
        for v, n in zip(verts, normals):
            f.write("%.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(v) + tuple(n)))


@pytest.fixture(scope="module")
def tracker(se3, tmp_path_factory):
    """Random-init fixture weights, the built-in rasteriser on the L of tests/pose_grid_scene.py, max_samples = 4; object_cloud and
    object_normals from a .ply of the L's points with their normals"""
    Hs, Ws = SC.HW
    info = dict(Fx.DATASET_INFO, object_width=180.0,
                camera=dict(height=Hs, width=Ws, focalX=SC.K[0, 0], focalY=SC.K[1, 1], centerX=SC.K[0, 2], centerY=SC.K[1, 2]))
    pts, nrm = SC.l_model()
    ply = str(tmp_path_factory.mktemp("pose_grid") / "l.ply")
    write_ply_with_normals(ply, pts, nrm)
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, model_path=ply, max_samples=4)
    assert trk.renderer is None and trk.last_acquire is None
    cloud = np.asarray(trk.object_cloud.points)
    assert trk.object_normals.shape == cloud.shape and len(cloud) > 200
    p2, n2 = se3.utils.voxel_down_sample_normals(pts, nrm, 0.005)
    assert np.array_equal(cloud, p2) and np.array_equal(trk.object_normals, n2)
    trk.renderer = se3.HipRenderer(trk.engine, SC.l_mesh())
    return trk


def key_of(rec, index=0):
    return PSO.key(rec["inlier_pts"], rec["behind_pts"], index)


def test_tracker_recover_facing_and_acquire(se3, tracker):
    depth = SC.frame(0)
    rgb = np.ascontiguousarray(Fx.structured_frame(7, *SC.HW)[0])
    G = SC.true_pose()
    cloud, normals = np.asarray(tracker.object_cloud.points, np.float64), tracker.object_normals
    lost = G.copy()
    lost[:3, :3] = Rotation.from_rotvec((0.1, -0.15, 0.1)).as_matrix() @ G[:3, :3]
    lost[:3, 3] += (0.023, -0.017, 0.031)
    # the default path before any facing call: its bits are the reference for "untouched"
    before = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL)
    before_info = tracker.last_recover
    # recover(facing=True): the factored lattice, the oracle's ranking
    rots, trans = se3.recover.lattice_factors(lost)
    want = PGO.score(cloud, normals, rots, trans, depth, SC.K, SC.TOL, 1)
    top = PSO.rank(want, 4)
    got0 = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, refine=0, facing=True)
    lr = tracker.last_recover
    assert lr["n"] == 9317 and np.array_equal(lr["top_idx"], top) and lr["facing"] is True
    same_records(lr["top_fit"], want[top], "recover top_fit")
    assert np.array_equal(got0, PGO.compose(rots, trans)[top[0]])
    assert lr["inlier_frac"] == int(want["inlier_pts"][top[0]]) / int(want["points"][top[0]])
    got1 = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, facing=True)
    lr = tracker.last_recover
    final = np.concatenate([lr["refined"], PGO.compose(rots, trans)[top]])
    diag = PGO.score(cloud, normals, final[:, :3, :3], final[:, :3, 3], depth, SC.K, SC.TOL, 1)[np.arange(8) * 9]
    same_records(lr["final_fit"], diag, "recover final_fit")
    assert lr["chosen"] == int(np.argmax(PSO.keys(diag))) and np.array_equal(got1, final[lr["chosen"]])
    assert key_of(lr["final_fit"][lr["chosen"]]) >= key_of(want[top[0]])
    with pytest.raises(ValueError, match="extra"):
        tracker.recover(lost, rgb, depth, extra=[G], facing=True)
    # acquire: no pose at all
    pose = tracker.acquire(rgb, depth, views=40, inplane=6, stride=8, tol_mm=SC.TOL)
    la = tracker.last_acquire
    grid_r, seeds = se3.recover.rotation_grid(40, 6), se3.recover.depth_seeds(depth, SC.K, 8, 0.03)
    stage1 = PGO.score(cloud, normals, grid_r, seeds, depth, SC.K, SC.TOL, 1)
    top1 = PSO.rank(stage1, 4)
    assert la["n"] == len(grid_r) * len(seeds) and la["n_rot"] == 240 and np.array_equal(la["stage1_idx"], top1)
    same_records(la["stage1_fit"], stage1[top1], "acquire stage 1")
    assert np.array_equal(la["hypotheses"], PGO.compose(grid_r, seeds)[top1]) and la["local"].shape == (4, 4, 4)
    for i in range(4):   # step 2: each hypothesis's own lattice, its best candidate
        lr_, lt_ = se3.recover.lattice_factors(la["hypotheses"][i])
        w = PGO.score(cloud, normals, lr_, lt_, depth, SC.K, SC.TOL, 1)
        b = int(PSO.rank(w, 1)[0])
        assert la["local_idx"][i] == b and la["local_fit"][i].tobytes() == w[b].tobytes() and np.array_equal(la["local"][i], PGO.compose(lr_, lt_)[b])
    final = np.concatenate([la["refined"], la["local"]])
    diag = PGO.score(cloud, normals, final[:, :3, :3], final[:, :3, 3], depth, SC.K, SC.TOL, 1)[np.arange(8) * 9]
    same_records(la["final_fit"], diag, "acquire final_fit")
    assert la["chosen"] == int(np.argmax(PSO.keys(diag))) and np.array_equal(pose, final[la["chosen"]])
    best_unrefined = max(key_of(r) for r in la["local_fit"])
    assert key_of(la["final_fit"][la["chosen"]]) >= best_unrefined
    print("acquire: stage 1 %s; local %s; chosen %d %s; %.1f mm from the truth" % (
        la["stage1_fit"]["inlier_pts"], la["local_fit"]["inlier_pts"], la["chosen"], la["final_fit"][la["chosen"]],
        1000 * np.linalg.norm(pose[:3, 3] - G[:3, 3])))
    with pytest.raises(ValueError, match="stride"):
        tracker.acquire(rgb, depth, views=400, inplane=12, stride=1)
    # the default path after the facing calls: the bits it gave before them
    after = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL)
    assert np.array_equal(after, before) and tracker.last_recover["final_fit"].tobytes() == before_info["final_fit"].tobytes()
    assert np.array_equal(tracker.last_recover["top_idx"], before_info["top_idx"]) and "facing" not in tracker.last_recover
    # without normals the facing paths say so
    keep, tracker.object_normals = tracker.object_normals, None
    try:
        with pytest.raises(ValueError, match="object_normals"):
            tracker.recover(lost, rgb, depth, facing=True)
        with pytest.raises(ValueError, match="object_normals"):
            tracker.acquire(rgb, depth)
    finally:
        tracker.object_normals = keep
