"""GPU: aligning pose hypotheses to the depth frame -- se3tn_align_poses, se3tn_align_poses_host, Engine.align_poses, Tracker.align,
Tracker.recover(align=) and Tracker.acquire(align=).

The yardstick is the numpy oracle of tests/pose_align_oracle.py (the rule of include/se3tracknet.h in float64, in the stated operation
order, held to a per-point loop and to the host build of the kernel's own statements by tests/test_pose_align_host.py), never the
library.  The arithmetic is IEEE float64 with no contraction on both sides and every sum is an integer, so the expectation is EXACT
EQUALITY of every pose (bytes), record and sum: there is no tolerance in this file except the stated distance to the true pose.

Without the feature every case fails: the symbols and attributes do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import pose_align_cases as CS
import pose_align_oracle as PAO
import pose_grid_oracle as PGO
import pose_grid_scene as SC
import pose_search_oracle as PSO
from oracle import fixtures as Fx
from oracle import se3_oracle as O
from test_gpu_pose_grid import write_ply_with_normals

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
T = 256                                    # csrc/pose_align_plan.h PA_THREADS: threads per pose
P_EDGES = [6, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]    # six unknowns; the lanes of one wave; the threads of a workgroup one short, full, one over; two walks and one
N_EDGES = [1, 2, 7, 65]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, 1)
    yield e
    e.close()


def cloud(P):
    """P points of the L with their normals: an evenly spread subset (of the upper face alone below 12 points), or the cloud and copies of
    it shifted by 0.1 mm per copy"""
    pts, nrm, _ = CS.l_scene()
    if P <= len(pts):
        last = len(pts) - 1 if P >= 12 else int((nrm[:, 2] > 0).sum()) - 1          # a handful: all of them on the upper face, so that they pair
        idx = np.linspace(0, last, P).astype(int)
        return np.ascontiguousarray(pts[idx]), np.ascontiguousarray(nrm[idx])
    reps = -(-P // len(pts))
    big = np.concatenate([pts + 1e-4 * k for k in range(reps)])[:P]
    return np.ascontiguousarray(big), np.ascontiguousarray(np.tile(nrm, (reps, 1))[:P])


def frames():
    """the 120 x 160 frame of the scene, and every fifth pixel of it as a 24 x 32 frame with the camera scaled to match"""
    depth = CS.l_scene()[2]
    small_K = SC.K.copy()
    small_K[:2] /= 5.0
    return ((depth, SC.K), (np.ascontiguousarray(depth[::5, ::5]), small_K))


@pytest.fixture(scope="module")
def poses65():
    """61 perturbations of the true pose, then one behind the camera, one with a NaN, one off the frame and the true pose itself"""
    G = SC.true_pose()
    return np.ascontiguousarray(np.array([*CS.perturbed(61, seed=3), *CS.bad_poses(), G]))


def same(got, want, what):
    for name, g, w in zip(("poses", "records", "sums"), got, want):
        g = np.asarray(g)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()]
            raise AssertionError((what, name, bad[:8], g[bad[0]], w[bad[0]]))


def on_device(se3, eng, mp, poses, depth, K, **prm):
    """se3tn_align_poses on uploaded copies -> (poses, records, sums) as numpy arrays.  The device entry point does not inspect the
    poses; the host entry point refuses one that is not finite, so the calls that carry such a pose come through here."""
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4))
    out, rec, sums = eng.align_poses(mp, torch.from_numpy(poses).cuda(), torch.from_numpy(depth.view(np.int16)).cuda(), K, sums=True, **prm)
    return out.cpu().numpy(), rec.cpu().numpy().view(se3._lib.ALIGN_REC_DTYPE).reshape(len(poses)), sums.cpu().numpy()


# ---- 1. every word equals the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_EDGES)
def test_poses_records_and_sums_equal_the_oracle(se3, eng, poses65, P):
    """P x {n = 1, 2, 7, 65} x {iters = 1, 2, 20} x {stop = 0, 1e-6} x {gate = 5, 20} x {120 x 160, 24 x 32}.  The oracle walks the 65
    poses once per (frame, stop, gate) -- the three iteration limits share their start (PAO.align_limits, held to PAO.align by
    tests/test_pose_align_host.py) -- and by guarantee (a) the calls with fewer poses must give its first n rows."""
    pts, nrm = cloud(P)
    mp = eng.model_points(pts, nrm)
    seen = set()
    for depth, K in frames():
        for stop in (0.0, 1e-6):
            for gate in (5, 20):
                prm = dict(gate_mm=gate, min_pairs=6, damping=1e-6, stop=stop)
                wants = PAO.align_limits(pts, nrm, poses65, depth, K, (1, 2, 20), **prm)
                for iters, want in wants.items():
                    seen.update(int(s) for s in want[1]["status"])
                    for n in N_EDGES:
                        got = on_device(se3, eng, mp, poses65[:n], depth, K, iters=iters, **prm)
                        same(got, [w[:n] for w in want], (P, depth.shape, iters, stop, gate, n))
                        if n <= 7:   # the host entry point (finite poses only): the same words
                            same(eng.align_poses(mp, poses65[:n], depth, K, sums=True, iters=iters, **prm), got, ("host", P, iters, stop, gate, n))
    # the cases show what they are meant to show (on the oracle alone)
    assert want[1]["pairs"][61] == 0 and want[1]["pairs"][62] == 0 and want[1]["pairs"][63] == 0 and want[1]["status"][61] == PAO.FEW
    if P >= 63:
        assert {PAO.ITERS, PAO.CONVERGED, PAO.FEW} <= seen, seen
    mp.close()


# ---- 2. bad poses -----------------------------------------------------------------------------------------------------------------------------
def test_bad_poses_get_their_status_and_harm_no_neighbour(se3, eng):
    pts, nrm, poses, depth, K = CS.plane_case()
    behind, nan, off = np.eye(4), np.eye(4), np.eye(4)
    behind[:3, 3] = (0.0, 0.0, -0.5)
    nan[:3, 3] = (0.0, np.nan, 0.5)
    off[:3, 3] = (2.0, 0.0, 0.5)
    mixed = np.array([poses[1], behind, poses[0], nan, poses[1], off, poses[0]])       # poses[0]: exactly frontal, singular without damping
    mp = eng.model_points(pts, nrm)
    prm = dict(CS.DEFAULTS, damping=0.0)
    got = on_device(se3, eng, mp, mixed, depth, K, **prm)
    same(got, PAO.align(pts, nrm, mixed, depth, K, **prm), "mixed")
    S = se3._lib
    assert list(got[1]["status"][[1, 2, 3, 5, 6]]) == [S.ALIGN_FEW, S.ALIGN_SINGULAR, S.ALIGN_FEW, S.ALIGN_FEW, S.ALIGN_SINGULAR]
    assert list(got[1]["iterations"][[1, 2, 3, 5, 6]]) == [1] * 5 and got[1]["pairs"][2] == len(pts) and got[1]["pairs"][3] == 0
    for i in (1, 2, 3, 5, 6):
        assert got[0][i, :3].tobytes() == mixed[i, :3].tobytes(), i                    # the bits they came in with
    assert (got[0][:, 3] == (0.0, 0.0, 0.0, 1.0)).all()
    alone = eng.align_poses(mp, mixed[:1], depth, K, sums=True, **prm)
    for i in (0, 4):
        assert all(np.asarray(g)[i].tobytes() == np.asarray(a)[0].tobytes() for g, a in zip(got, alone)), i
    mp.close()
    # the same on the L: behind, NaN and off the frame between two poses that align
    pts, nrm, poses, depth, K = CS.l_case()
    mp = eng.model_points(pts, nrm)
    got = on_device(se3, eng, mp, poses, depth, K)
    same(got, PAO.align(pts, nrm, poses, depth, K, **CS.DEFAULTS), "l_case")
    assert list(got[1]["status"]) == [S.ALIGN_CONVERGED, S.ALIGN_FEW, S.ALIGN_FEW, S.ALIGN_FEW, S.ALIGN_CONVERGED]
    clean = eng.align_poses(mp, poses[[0, 4]], depth, K, sums=True)
    assert all(np.asarray(g)[[0, 4]].tobytes() == np.asarray(c).tobytes() for g, c in zip(got, clean))
    mp.close()


# ---- 3. a pose's output is the same in any call -----------------------------------------------------------------------------------------------
def test_a_pose_is_aligned_the_same_at_any_n_and_in_any_order(se3, eng, poses65):
    pts, nrm = cloud(2 * T + 1)
    depth, K = frames()[0]
    mp = eng.model_points(pts, nrm)
    full = on_device(se3, eng, mp, poses65, depth, K)
    again = on_device(se3, eng, mp, poses65, depth, K)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))               # on every run
    order = np.random.default_rng(3).permutation(len(poses65))
    perm = on_device(se3, eng, mp, poses65[order], depth, K)
    assert all(p.tobytes() == np.ascontiguousarray(f[order]).tobytes() for p, f in zip(perm, full))
    for lo, hi in ((0, 1), (5, 12), (60, 65), (64, 65)):
        sub = on_device(se3, eng, mp, poses65[lo:hi], depth, K)
        assert all(s.tobytes() == np.ascontiguousarray(f[lo:hi]).tobytes() for s, f in zip(sub, full)), (lo, hi)
    mp.close()


# ---- 4. the entry points -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_in_place_sentinels_and_refusals(se3, eng, poses65):
    L, lib = se3._lib, eng.lib
    pts, nrm = cloud(T + 1)
    depth, K = frames()[0]
    H, W = depth.shape
    n = 7
    mp = eng.model_points(pts, nrm)
    want = PAO.align(pts, nrm, poses65[:n], depth, K, **CS.DEFAULTS)
    host = eng.align_poses(mp, poses65[:n], depth, K, sums=True)                      # se3tn_align_poses_host
    same(host, want, "host")
    two = eng.align_poses(mp, poses65[:n], depth, K)                                   # without the sums: two values
    assert len(two) == 2 and two[0].tobytes() == want[0].tobytes() and two[1].tobytes() == want[1].tobytes()
    poses_d = torch.from_numpy(poses65[:n].copy()).cuda()
    depth_d = torch.from_numpy(depth.view(np.int16)).cuda()
    dev = eng.align_poses(mp, poses_d, depth_d, K, sums=True)                          # se3tn_align_poses: tensors in, tensors out
    assert dev[0].is_cuda and dev[0].dtype == torch.float64 and tuple(dev[0].shape) == (n, 4, 4)
    assert dev[1].dtype == torch.uint8 and tuple(dev[1].shape) == (n, 40) and dev[2].dtype == torch.int64 and tuple(dev[2].shape) == (n, 28)
    same((dev[0].cpu().numpy(), dev[1].cpu().numpy().view(L.ALIGN_REC_DTYPE).reshape(n), dev[2].cpu().numpy()), want, "device")
    assert torch.equal(poses_d.cpu(), torch.from_numpy(poses65[:n]))                   # the input is left alone
    # in place, with sentinel rows after the n-th pose, record and sums row
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    prm = L.AlignParams(20, 20, 12, 0, 1e-6, 1e-6)
    io = torch.full((n + 1, 16), -7.25, dtype=torch.float64, device="cuda")
    io[:n] = torch.from_numpy(poses65[:n].reshape(n, 16))
    rec = torch.full((n + 1, 40), 0x5A, dtype=torch.uint8, device="cuda")
    sums = torch.full((n + 1, 28), -99, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.se3tn_align_poses(eng._h, mp._h, n, vp(io), vp(depth_d), H, W, Kp, C.byref(prm), vp(io), vp(rec), vp(sums), st) == 0
    torch.cuda.synchronize()
    same((io[:n].cpu().numpy().reshape(n, 4, 4), rec[:n].cpu().numpy().view(L.ALIGN_REC_DTYPE).reshape(n), sums[:n].cpu().numpy()), want, "in place")
    assert (io[n] == -7.25).all() and (rec[n] == 0x5A).all() and (sums[n] == -99).all()
    # the sums are optional
    out2 = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    assert lib.se3tn_align_poses(eng._h, mp._h, n, vp(poses_d), vp(depth_d), H, W, Kp, C.byref(prm), vp(out2), vp(rec), None, st) == 0
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == want[0].tobytes()
    # refusals on a live context
    bad = L.AlignParams(20, 65, 12, 0, 1e-6, 1e-6)
    assert lib.se3tn_align_poses(eng._h, mp._h, n, vp(poses_d), vp(depth_d), H, W, Kp, C.byref(bad), vp(out2), vp(rec), None, st) == E_ARG
    assert lib.se3tn_align_poses(eng._h, mp._h, 4097, vp(poses_d), vp(depth_d), H, W, Kp, C.byref(prm), vp(out2), vp(rec), None, st) == E_ARG
    plain = eng.model_points(pts)
    with pytest.raises(L.Se3tnError, match="rc=%d.*no normals" % E_STATE):
        eng.align_poses(plain, poses65[:n], depth, K)
    with pytest.raises(L.Se3tnError, match="rc=%d.*no normals" % E_STATE):
        eng.align_poses(plain, poses_d, depth_d, K)
    plain.close()
    for val in (np.nan, np.inf):
        broken = poses65[:n].copy()
        broken[3, 1, 2] = val
        with pytest.raises(L.Se3tnError, match="rc=%d.*pose 3" % E_ARG):
            eng.align_poses(mp, broken, depth, K)
        Kb = K.copy()
        Kb[1, 1] = val
        with pytest.raises(L.Se3tnError, match="rc=%d.*K entry 4" % E_ARG):
            eng.align_poses(mp, poses65[:n], depth, Kb)
    row3 = poses65[:n].copy()
    row3[:, 3] = np.nan                                                                # row 3 is not read
    same(eng.align_poses(mp, row3, depth, K, sums=True), want, "row 3")
    # the host variant waits for its stream: inside a capture it says so and leaves the capture whole
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(L.Se3tnError, match="rc=%d" % E_STATE):
            eng.align_poses(mp, poses65[:n], depth, K)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    same(eng.align_poses(mp, poses65[:n], depth, K, sums=True), want, "after the refused capture")
    # the searches share the staging: they still give their own answers afterwards, and so does the alignment after them
    i2, f2 = eng.score_poses(mp, poses65[:61], depth, K, SC.TOL, top=8)
    w2 = PSO.score(pts, poses65[:61], depth, K, SC.TOL)
    assert np.array_equal(i2, PSO.rank(w2, 8)) and f2.tobytes() == w2[i2].tobytes()
    same(eng.align_poses(mp, poses65[:n], depth, K, sums=True), want, "after se3tn_search_poses_host")
    mp.close()


# ---- 5. one linear stream capture ----------------------------------------------------------------------------------------------------------------
def test_a_captured_alignment_replays_with_a_changed_frame(se3, eng, poses65):
    L = se3._lib
    pts, nrm = cloud(T + 1)
    depth, K = frames()[0]
    H, W = depth.shape
    n = 7
    mp = eng.model_points(pts, nrm)
    poses_d = torch.from_numpy(poses65[:n].copy()).cuda()
    depth_d = torch.from_numpy(depth.view(np.int16)).cuda()
    out_d = torch.zeros((n, 16), dtype=torch.float64, device="cuda")
    rec_d = torch.zeros((n, 40), dtype=torch.uint8, device="cuda")
    sums_d = torch.zeros((n, 28), dtype=torch.int64, device="cuda")
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    prm = L.AlignParams(20, 20, 12, 0, 1e-6, 1e-6)

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return eng.lib.se3tn_align_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, C.byref(prm),
                                         C.c_void_p(out_d.data_ptr()), C.c_void_p(rec_d.data_ptr()), C.c_void_p(sums_d.data_ptr()), st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert enqueue() == 0                                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert enqueue() == 0                                                          # one launch
    for turn in range(2):
        changed = np.ascontiguousarray(np.roll(depth, turn + 1, axis=1) + np.uint16(2 * turn))
        depth_d.copy_(torch.from_numpy(changed.view(np.int16)))
        out_d.zero_(); rec_d.zero_(); sums_d.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = PAO.align(pts, nrm, poses65[:n], changed, K, **CS.DEFAULTS)
        same((out_d.cpu().numpy().reshape(n, 4, 4), rec_d.cpu().numpy().view(L.ALIGN_REC_DTYPE).reshape(n), sums_d.cpu().numpy()), want, ("replay", turn))
    mp.close()


# ---- 6. Tracker.align, recover(align=) and acquire(align=) -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracker(se3, tmp_path_factory):
    """The fixture of tests/test_gpu_pose_grid.py: random-init weights, the built-in rasteriser on the L, max_samples = 4, object_cloud and
    object_normals from a .ply of the L's points with their normals"""
    Hs, Ws = SC.HW
    info = dict(Fx.DATASET_INFO, object_width=180.0,
                camera=dict(height=Hs, width=Ws, focalX=SC.K[0, 0], focalY=SC.K[1, 1], centerX=SC.K[0, 2], centerY=SC.K[1, 2]))
    pts, nrm = SC.l_model()
    ply = str(tmp_path_factory.mktemp("pose_align") / "l.ply")
    write_ply_with_normals(ply, pts, nrm)
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, model_path=ply, max_samples=4)
    trk.renderer = se3.HipRenderer(trk.engine, SC.l_mesh())
    return trk


def test_tracker_align_recover_and_acquire(se3, tracker):
    depth = SC.frame(0)
    rgb = np.ascontiguousarray(Fx.structured_frame(7, *SC.HW)[0])
    G = SC.true_pose()
    cloud_, normals = np.asarray(tracker.object_cloud.points, np.float64), tracker.object_normals
    acq = dict(views=40, inplane=6, stride=8, tol_mm=SC.TOL, refine=0)
    # the default path before any aligned call: its bits and keys are the reference for "untouched"
    before = tracker.acquire(rgb, depth, **acq)
    before_info = tracker.last_acquire
    assert "aligned" not in before_info and "align_rec" not in before_info
    # Tracker.align is Engine.align_poses on the facing handle
    two = CS.perturbed(2, seed=11)
    got = tracker.align(two, depth, sums=True)
    same(got, PAO.align(cloud_, normals, two, depth, SC.K, **CS.DEFAULTS), "Tracker.align")
    # acquire with alignment
    pose = tracker.acquire(rgb, depth, align=20, **acq)
    la = tracker.last_acquire
    for k in ("stage1_idx", "hypotheses", "local", "local_idx"):
        assert np.array_equal(la[k], before_info[k]), k
    want = PAO.align(cloud_, normals, la["local"], depth, SC.K, **CS.DEFAULTS)
    assert la["aligned"].tobytes() == want[0].tobytes() and la["align_rec"].tobytes() == want[1].tobytes()
    pool = np.concatenate([la["aligned"], la["local"]])
    fit = CS.facing_fit(cloud_, normals, pool, depth, SC.K, SC.TOL)
    assert la["final_fit"].tobytes() == fit.tobytes() and la["refined"] is None
    assert la["chosen"] == int(np.argmax(PSO.keys(fit))) and np.array_equal(pose, pool[la["chosen"]])
    err = PAO.pose_error(pose, G)
    print("acquire(align=20): local %s -> aligned %s; chosen %d, %.2f mm / %.3f deg from the truth" % (
        la["local_fit"]["inlier_pts"], la["final_fit"]["inlier_pts"][:len(la["local"])], la["chosen"], 1000 * err[0], err[1]))
    assert err[0] <= CS.BOUND_M and err[1] <= CS.BOUND_DEG
    key = lambda r: PSO.key(r["inlier_pts"], r["behind_pts"], 0)   # noqa: E731
    assert key(fit[la["chosen"]]) > max(key(r) for r in before_info["final_fit"])      # strictly above the best lattice node
    # the same call with align=0 afterwards: identical bits, no new keys
    after = tracker.acquire(rgb, depth, align=0, **acq)
    assert np.array_equal(after, before) and sorted(tracker.last_acquire) == sorted(before_info)
    for k, v in before_info.items():
        w = tracker.last_acquire[k]
        assert (v is None and w is None) or np.asarray(w).tobytes() == np.asarray(v).tobytes(), k
    # recover: with alignment the result never scores below the one without
    lost = G.copy()
    lost[:3, :3] = Rotation.from_rotvec((0.1, -0.15, 0.1)).as_matrix() @ G[:3, :3]
    lost[:3, 3] += (0.023, -0.017, 0.031)
    plain = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, facing=True, refine=0)
    plain_info = tracker.last_recover
    assert "aligned" not in plain_info
    better = tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, facing=True, refine=0, align=20)
    lr = tracker.last_recover
    want = PAO.align(cloud_, normals, PGO.compose(*se3.recover.lattice_factors(lost))[lr["top_idx"]], depth, SC.K, **CS.DEFAULTS)
    assert np.array_equal(lr["top_idx"], plain_info["top_idx"]) and lr["aligned"].tobytes() == want[0].tobytes()
    assert lr["align_rec"].tobytes() == want[1].tobytes() and len(lr["final_fit"]) == 2 * len(lr["top_idx"])
    assert key(lr["final_fit"][lr["chosen"]]) >= key(plain_info["final_fit"][0])
    print("recover: %d inliers without alignment, %d with; %.2f mm from the truth" % (
        plain_info["final_fit"]["inlier_pts"][0], lr["final_fit"]["inlier_pts"][lr["chosen"]], 1000 * PAO.pose_error(better, G)[0]))
    assert np.array_equal(tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, facing=True, refine=0), plain)
    # the plain search may be aligned too (its scoring stays plain), and with the network the pool has three parts
    tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, refine=0, align=20)
    assert "facing" not in tracker.last_recover and len(tracker.last_recover["final_fit"]) == 8
    tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, facing=True, refine=1, align=5)
    assert len(tracker.last_recover["final_fit"]) == 12 and tracker.last_recover["refined"].shape == (4, 4, 4)
    # without normals every aligned path says so
    keep, tracker.object_normals = tracker.object_normals, None
    try:
        with pytest.raises(ValueError, match="object_normals"):
            tracker.acquire(rgb, depth, align=20, **acq)
        with pytest.raises(ValueError, match="object_normals"):
            tracker.recover(lost, rgb, depth, facing=True, align=20)
        with pytest.raises(ValueError, match="object_normals"):
            tracker.recover(lost, rgb, depth, align=20)
        with pytest.raises(ValueError, match="object_normals"):
            tracker.align(two, depth)
        assert tracker.recover(lost, rgb, depth, tol_mm=SC.TOL, refine=0).shape == (4, 4)     # the plain search needs none
    finally:
        tracker.object_normals = keep
