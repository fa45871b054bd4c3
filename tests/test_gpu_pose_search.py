"""GPU: re-acquiring a lost object -- se3tn_score_poses / se3tn_rank_poses / se3tn_search_poses_host, Engine.score_poses,
Tracker.recover, LiveTracker(recover_below=...).

The yardstick is the numpy oracle of tests/pose_search_oracle.py (the rule of include/se3tracknet.h in float64, in the stated
operation order, held to a per-point loop by tests/test_pose_search_host.py), never the library.  The arithmetic is IEEE float64
with no contraction on both sides and every counter is an integer sum, so the expectation is EXACT EQUALITY of every counter and of
every ranked index: there is no tolerance in this file.

Scene (that of tests/test_gpu_fit_check.py): the 120 x 160 camera Fx.SOUP_FRAME_K, the ellipsoid ST.make_object(4) composed into
the frame at G_TRUE = Fx.pose(11, (0.004, -0.003, 0.5)) with a distractor sphere, before a wall at 900 mm with holes.  Model points
are subsampled from the ellipsoid's 2,562 vertices.  Without the feature every case fails: the symbols and attributes do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import pose_search_cases as PC
import pose_search_oracle as PSO
from oracle import closed_loop as CL
from oracle import fixtures as Fx
from oracle import free_run as FR
from oracle import synth_track as ST

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2
H, W = Fx.SOUP_FRAME_HW
K = Fx.SOUP_FRAME_K
WIDTH = ST.OBJECT_WIDTH_MM
INFO = dict(Fx.DATASET_INFO, object_width=WIDTH,
            camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
MESH = ST.make_object(4)
VERTS = np.asarray(MESH["vertices"], np.float64)
G_TRUE = Fx.pose(11, (0.004, -0.003, 0.5))
G_SPHERE = Fx.pose(12, (-0.05, 0.02, 0.62))
TOL = 5
# the four off-lattice lost poses of the issue's prototype: translation offsets (metres) and rotation vectors (camera frame)
LOST_OFFSETS = [(0.033, -0.024, 0.046), (-0.037, 0.031, -0.028), (-0.046, 0.017, 0.044), (0.012, 0.043, -0.049)]
LOST_ROTVECS = [(0.1, 0.2, -0.15), (0.0, 0.0, 0.0), (0.2, -0.1, 0.1), (-0.15, 0.1, 0.2)]
STEP, RADIUS_STEPS, ROT_DEG = 0.01, 5, (15.0,)


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
def frame():
    """(rgb, depth) of the fit-check scene: both objects before the wall with holes"""
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = Fx.structured_frame(401, H, W)[0]
    wall = (900 + 0.5 * (xx - W / 2) + 0.3 * (yy - H / 2)).astype(np.uint16)
    wall[rng.random((H, W)) < 0.04] = 0
    obj = (rgb, wall)
    for mesh, G in ((Fx.icosphere(2, 0.05, 1), G_SPHERE), (MESH, G_TRUE)):
        obj = ST.compose_frame(obj, ST.object_patch(CL.oracle_mesh(mesh), G, K))
    assert (obj[1] != wall).sum() > 1500
    return np.ascontiguousarray(obj[0]), np.ascontiguousarray(obj[1])


def subsample(P):
    """P of the ellipsoid's vertices, spread over the whole list"""
    return np.ascontiguousarray(VERTS[np.round(np.linspace(0, len(VERTS) - 1, P)).astype(int)])


def moved(G, rotvec, offset):
    """G rotated by rotvec and shifted by offset in the camera frame: R = dR . R_G, t = t_G + offset"""
    T = G.copy()
    T[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix() @ G[:3, :3]
    T[:3, 3] = G[:3, 3] + np.asarray(offset, np.float64)
    return T


def lost_pose(i):
    return moved(G_TRUE, LOST_ROTVECS[i], LOST_OFFSETS[i])


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def poses37():
    """near the truth (12), lost (8), rotated by up to 3 rad (12), and five special ones: behind the camera, all points off the frame
    to the right, all points above it, straddling the right edge, straddling the bottom edge"""
    rng = np.random.default_rng(37)
    out = [G_TRUE]
    out += [moved(G_TRUE, unit(rng) * rng.uniform(0, 0.05), rng.uniform(-0.004, 0.004, 3)) for _ in range(11)]
    out += [moved(G_TRUE, unit(rng) * rng.uniform(0, 0.26), unit(rng) * rng.uniform(0.05, 0.07)) for _ in range(8)]
    out += [moved(G_TRUE, unit(rng) * rng.uniform(0.5, 3.0), rng.uniform(-0.02, 0.02, 3)) for _ in range(12)]
    zc = G_TRUE[2, 3]
    right = (W - 0.5 - K[0, 2]) / K[0, 0] * zc      # x of the camera ray through the frame's right edge at the object's depth
    bottom = (H - 0.5 - K[1, 2]) / K[1, 1] * zc
    out.append(moved(G_TRUE, (0, 0, 0), (0, 0, -2 * zc)))                          # behind the camera
    out.append(moved(G_TRUE, (0, 0, 0), (2.0, 0, 0)))                              # off the frame
    out.append(moved(G_TRUE, (0, 0, 0), (0, -2.0, 0)))
    out.append(moved(G_TRUE, (0.3, 0, 0), (right - G_TRUE[0, 3], 0, 0)))           # the object's centre ON the right edge
    out.append(moved(G_TRUE, (0, 0.3, 0), (0, bottom - G_TRUE[1, 3], 0)))          # ... on the bottom edge
    assert len(out) == 37
    return np.array(out)


def host_all(eng, mp, poses, depth, tol=TOL, Kc=K):
    """every record of a call (the device entry point behind Engine.score_poses)"""
    return eng.score_poses(mp, poses, depth, Kc, tol)


def same_records(got, want, what):
    assert got.dtype == PSO.DTYPE and got.shape == want.shape, what
    for k in PSO.FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])


# ---- 5. tiling edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2562])
def test_every_tiling_edge_equals_the_oracle(se3, eng, frame, P):
    """One workgroup of 256 threads (four waves) per pose, thread t taking points t, t + 256, ...: 1 and 2 -- single lanes of wave 0,
    three waves without a point; 63, 64, 65 -- the first wave one short, full, and the second wave's first lane; 255, 256, 257 --
    the workgroup one short, every thread exactly one point, and thread 0's second trip; 1,025 -- four full trips and one lane of
    a fifth; 2,562 -- the whole model, ten trips and two lanes of an eleventh."""
    pts = subsample(P)
    poses = poses37()
    want = PSO.score(pts, poses, frame[1], K, TOL)
    PSO.check_invariants(want, P, TOL)
    # the cases show what they are meant to show (on the oracle alone)
    assert want["in_frame_pts"][32] == 0 and want["in_frame_pts"][33] == 0 and want["in_frame_pts"][34] == 0
    if P >= 63:
        assert want["inlier_pts"][0] > 0 and 0 < want["in_frame_pts"][35] < P and 0 < want["in_frame_pts"][36] < P
        assert want["inlier_pts"][:12].min() > want["inlier_pts"][12:20].max()       # near the truth beats lost
    mp = eng.model_points(pts)
    got = host_all(eng, mp, poses, frame[1])
    print("P = %d: inliers of the truth %d, counters differing %d" % (P, want["inlier_pts"][0], sum(int((got[k] != want[k]).sum()) for k in PSO.FIELDS)))
    same_records(got, want, P)
    PSO.check_invariants(got, P, TOL)
    # the host entry point: the k best, indices and records
    for k in (1, 8, 37):
        idx, fit = eng.score_poses(mp, poses, frame[1], K, TOL, top=k)
        assert idx.dtype == np.int32 and np.array_equal(idx, PSO.rank(want, k)), (P, k)
        same_records(fit, want[idx], (P, k))
    mp.close()


# ---- 6. exact boundaries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(6, 6), (7, 7), (6, 7), (7, 6)])
@pytest.mark.parametrize("tol", [1, 7, 65535])
def test_exact_boundaries(se3, eng, hw, tol):
    """Identity rotation, points at z = 1 and K = [[1, 0, 0.5], [0, 1, 1.5]]: u = x + 0.5 and v = y + 1.5 are exact, so points sit ON
    -0.5 (rounds to -0.0: inside), 0.5 (to 0), W - 1.5 and W - 0.5 (to W for even W: outside; to W - 1 for odd W), and the same for
    v; two points are far beyond any integer.  m = 1000 exactly; the frame's pixels cycle through 0, 100, 101, 1999, 2000, 65535
    and 1000 -+ (tol - 1, tol, tol + 1) where a uint16 holds them, shifted one place per call so that every hit pixel takes every value."""
    Hh, Ww = hw
    Kc = PC.BOUNDARY_K
    pts = PC.boundary_points(hw)
    poses = PC.boundary_poses()
    vals = PC.boundary_values(tol)
    mp = eng.model_points(pts)
    n_in_x = 3 if Ww % 2 == 0 else 4
    n_in_y = 3 if Hh % 2 == 0 else 4
    seen_total = 0
    for shift in range(len(vals)):
        depth = PC.boundary_depth(hw, vals, shift)
        want = PSO.score(pts, poses, depth, Kc, tol)
        # by hand, for the identity pose: which boundary points are inside does not depend on the depth
        assert want["in_frame_pts"][0] == n_in_x * n_in_y and want["in_frame_pts"][2] == 0, (hw, want)
        got = eng.score_poses(mp, poses, depth, Kc, tol)
        same_records(got, want, (hw, tol, shift))
        PSO.check_invariants(got, len(pts), tol)
        seen_total += int(want["seen_pts"][0])
    # over the shifts every hit pixel has taken every value: the valid ones of `vals` are seen once per inside point
    n_valid = int(((vals > 100) & (vals < 2000)).sum())
    assert seen_total == n_in_x * n_in_y * n_valid
    mp.close()


# ---- 7. independence -------------------------------------------------------------------------------------------------------------------------
def test_a_pose_has_the_same_record_alone_in_any_call_at_any_position_and_on_every_run(se3, eng, frame):
    rng = np.random.default_rng(7)
    pts = subsample(257)
    others = np.array([moved(G_TRUE, unit(rng) * rng.uniform(0, 1.0), rng.uniform(-0.06, 0.06, 3)) for _ in range(256)])
    mine = moved(G_TRUE, (0.02, -0.03, 0.01), (0.002, -0.001, 0.003))
    want = PSO.score(pts, mine[None], frame[1], K, TOL)
    assert want["inlier_pts"][0] > 0 and want["front_pts"][0] > 0
    mp = eng.model_points(pts)
    alone = host_all(eng, mp, mine[None], frame[1])
    same_records(alone, want, "alone")
    for n in (1, 2, 7, 257):
        for pos in sorted({0, n // 2, n - 1}):
            poses = np.concatenate([others[:pos], mine[None], others[pos:n - 1]])
            assert len(poses) == n
            got = host_all(eng, mp, poses, frame[1])
            again = host_all(eng, mp, poses, frame[1])
            assert got.tobytes() == again.tobytes(), (n, pos)
            assert got[pos:pos + 1].tobytes() == alone.tobytes(), (n, pos)
    # a pose that is not finite harms no other pose of the call (the device entry point does not inspect poses)
    poses = np.concatenate([others[:3], mine[None], others[3:6]])
    poses[2, 1, 1] = np.nan
    got = host_all(eng, mp, poses, frame[1])
    assert got["in_frame_pts"][2] == 0 and got[3:4].tobytes() == alone.tobytes()
    same_records(got, PSO.score(pts, poses, frame[1], K, TOL), "NaN pose")
    mp.close()


# ---- 8. ranking --------------------------------------------------------------------------------------------------------------------------------
def rank_call(eng, fit_d, n, k, idx_d):
    return eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_ranking_equals_the_oracles_sort(se3, eng, n):
    """Records synthesised on the host with many repeated (inlier, behind) pairs -- ties down to the index -- and behind counts at
    and above the clamp; n around the workgroup's 256 threads."""
    rng = np.random.default_rng(n)
    fit = np.zeros(n, PSO.DTYPE)
    fit["inlier_pts"] = rng.integers(0, 4, n)
    fit["behind_pts"] = rng.choice(np.array([0, 1, 5, 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20 + 5, 3000000], np.uint32), n)
    fit["points"] = 2 ** 20
    fit_d = torch.from_numpy(fit.view(np.int32).reshape(n, 8).copy()).cuda()
    for k in sorted({1, min(n, 8), min(n, 64)}):
        idx_d = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        assert rank_call(eng, fit_d, n, k, idx_d) == 0
        assert np.array_equal(idx_d.cpu().numpy(), PSO.rank(fit, k)), (n, k)
    idx_d = torch.full((65,), -1, dtype=torch.int32, device="cuda")
    assert rank_call(eng, fit_d, n, min(n, 64) + 1, idx_d) == E_ARG          # k > n, or k > 64
    assert rank_call(eng, fit_d, n, 65, idx_d) == E_ARG and rank_call(eng, fit_d, n, 0, idx_d) == E_ARG
    assert b"SE3TN_POSE_RANK_MAX" in eng.lib.se3tn_last_error()
    assert (idx_d.cpu().numpy() == -1).all()


# ---- 9. the device-pointer entry points ------------------------------------------------------------------------------------------------------
def test_device_pointers_give_the_host_variants_bits_also_from_a_replayed_graph(se3, eng, frame):
    pts = subsample(257)
    rng = np.random.default_rng(9)
    n, k = 300, 8
    poses = np.array([moved(G_TRUE, unit(rng) * rng.uniform(0, 0.3), rng.uniform(-0.05, 0.05, 3)) for _ in range(n)])
    want = PSO.score(pts, poses, frame[1], K, TOL)
    mp = eng.model_points(pts)
    h_idx, h_fit = eng.score_poses(mp, poses, frame[1], K, TOL, top=k)                 # the host entry point
    assert np.array_equal(h_idx, PSO.rank(want, k))
    same_records(h_fit, want[h_idx], "host")
    poses_d = torch.from_numpy(poses.reshape(n, 16)).cuda()
    depth_d = torch.from_numpy(frame[1].view(np.int16)).cuda()
    fit_t = eng.score_poses(mp, poses_d, depth_d, K, TOL)                              # tensors in, tensors out
    assert fit_t.is_cuda and fit_t.dtype == torch.int32 and tuple(fit_t.shape) == (n, 8)
    same_records(fit_t.cpu().numpy().view(PSO.DTYPE).reshape(n), want, "device")
    idx_t, top_t = eng.score_poses(mp, poses_d, depth_d, K, TOL, top=k)
    assert np.array_equal(idx_t.cpu().numpy(), h_idx) and top_t.cpu().numpy().view(PSO.DTYPE).reshape(k).tobytes() == h_fit.tobytes()
    # capture score + rank on a side stream, replay with the CONTENTS of the pose buffer changed
    fit_d = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    idx_d = torch.zeros((k,), dtype=torch.int32, device="cuda")
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = eng.lib.se3tn_score_poses(eng._h, mp._h, n, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, TOL,
                                       C.c_void_p(fit_d.data_ptr()), st)
        return rc or eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()), st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert enqueue() == 0                                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert enqueue() == 0
    for turn in range(3):
        order = np.roll(np.arange(n), 7 * turn + 1)
        poses_d.copy_(torch.from_numpy(poses[order].reshape(n, 16)))
        fit_d.zero_(); idx_d.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_records(fit_d.cpu().numpy().view(PSO.DTYPE).reshape(n), want[order], ("replay", turn))
        assert np.array_equal(idx_d.cpu().numpy(), PSO.rank(want[order], k)), turn
    again = eng.score_poses(mp, poses, frame[1], K, TOL, top=k)                        # an eager host call after the replays
    assert np.array_equal(again[0], h_idx) and again[1].tobytes() == h_fit.tobytes()
    mp.close()


# ---- 10. the search on the scene ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searches(frame):
    """per lost pose: the lattice of 9,317 candidates, the oracle's records of all of them and its top 8 (computed once)"""
    pts = subsample(257)
    out = []
    for i in range(4):
        lost = lost_pose(i)
        lat = PSO.lattice(lost, RADIUS_STEPS, STEP, ROT_DEG)
        fit = PSO.score(pts, lat, frame[1], K, TOL)
        out.append(dict(lost=lost, lattice=lat, fit=fit, top=PSO.rank(fit, 8)))
    return dict(pts=pts, cases=out)


@pytest.mark.parametrize("i", range(4))
def test_search_on_the_scene_finds_what_the_oracle_finds(se3, eng, frame, searches, i):
    c, pts = searches["cases"][i], searches["pts"]
    assert len(c["lattice"]) == 9317
    # input condition, on the oracle alone: its best candidate lies within one lattice step (per axis) of the true translation
    best = c["lattice"][c["top"][0]]
    assert np.linalg.norm(best[:3, 3] - G_TRUE[:3, 3]) <= np.sqrt(3) * STEP
    lat = se3.pose_lattice(c["lost"], RADIUS_STEPS * STEP, STEP, ROT_DEG)
    assert np.array_equal(lat, c["lattice"])
    mp = eng.model_points(pts)
    idx, fit = eng.score_poses(mp, lat, frame[1], K, TOL, top=8)
    print("lost pose %d: oracle top %s inliers %s; library top %s" % (i, c["top"], c["fit"]["inlier_pts"][c["top"]], idx))
    assert np.array_equal(idx, c["top"])
    same_records(fit, c["fit"][c["top"]], i)
    mp.close()


# ---- 11. Tracker.recover and LiveTracker -------------------------------------------------------------------------------------------------
def write_ply(path, verts):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\nend_header\n" % len(verts))
        for v in verts:
            f.write("%.17g %.17g %.17g\n" % tuple(v))


@pytest.fixture(scope="module")
def tracker(se3, tmp_path_factory):
    """The trained stand-in weights, the built-in rasteriser on the ellipsoid, max_samples = 8; object_cloud from a .ply of its vertices"""
    sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights("ycbineoat_30deg"))
    tn, rn = CL.REGIMES["ycbineoat_30deg"]
    ply = str(tmp_path_factory.mktemp("pose_search") / "ellipsoid.ply")
    write_ply(ply, VERTS)
    trk = se3.Tracker(INFO, mean, std, {"state_dict": sd}, model_path=ply, trans_normalizer=tn, rot_normalizer=rn, max_samples=8)
    assert trk.renderer is None and trk.object_cloud is not None and len(trk.object_cloud.points) > 100
    trk.renderer = se3.HipRenderer(trk.engine, MESH)
    assert trk.one_call and trk.last_recover is None
    return trk


def key_of(rec, index=0):
    return PSO.key(rec["inlier_pts"], rec["behind_pts"], index)


def test_tracker_recover(se3, tracker, frame, searches):
    rgb, depth = frame
    c, pts = searches["cases"][0], searches["pts"]
    lost = c["lost"]
    eng = tracker.engine
    kw = dict(trans_radius=RADIUS_STEPS * STEP, trans_step=STEP, rot_deg=ROT_DEG, tol_mm=TOL, points=pts)
    # refine = 0: exactly the oracle's best lattice candidate, no network call
    calls = tracker.frame_cnt
    got0 = tracker.recover(lost, rgb, depth, refine=0, **kw)
    assert tracker.frame_cnt == calls
    assert np.array_equal(got0, c["lattice"][c["top"][0]])
    lr = tracker.last_recover
    assert lr["n"] == 9317 and np.array_equal(lr["top_idx"], c["top"]) and lr["refined"] is None and lr["chosen"] == 0
    same_records(lr["top_fit"], c["fit"][c["top"]], "top_fit")
    assert lr["inlier_frac"] == int(c["fit"]["inlier_pts"][c["top"][0]]) / 257
    # refine = 1: exactly what the public calls give
    got1 = tracker.recover(lost, rgb, depth, refine=1, **kw)
    lr = tracker.last_recover
    mp = eng.model_points(pts)
    top_poses = c["lattice"][c["top"]]
    refined = tracker.on_track_batch(list(top_poses), [rgb] * 8, [depth] * 8)
    final = np.concatenate([refined, top_poses])
    final_fit = eng.score_poses(mp, final, depth, K, TOL)
    same_records(final_fit, PSO.score(pts, final, depth, K, TOL), "final")
    keys = PSO.keys(final_fit)
    chosen = int(np.argmax(keys))
    assert np.array_equal(lr["refined"], refined) and lr["chosen"] == chosen and lr["final_fit"].tobytes() == final_fit.tobytes()
    assert np.array_equal(got1, final[chosen])
    assert lr["inlier_frac"] == int(final_fit["inlier_pts"][chosen]) / 257
    # comparisons against the inputs, no thresholds: never below the lattice's best, above the lost pose, nearer to the truth
    lost_fit = eng.score_poses(mp, lost[None], depth, K, TOL)[0]
    print("lost: %s; lattice best: %s; recovered (candidate %d of 16): %s; translation error %.4f -> %.4f m" % (
        lost_fit, c["fit"][c["top"][0]], chosen, final_fit[chosen],
        np.linalg.norm(lost[:3, 3] - G_TRUE[:3, 3]), np.linalg.norm(got1[:3, 3] - G_TRUE[:3, 3])))
    assert key_of(final_fit[chosen]) >= key_of(c["fit"][c["top"][0]]) and key_of(final_fit[chosen]) > key_of(lost_fit)
    assert np.linalg.norm(got1[:3, 3] - G_TRUE[:3, 3]) < np.linalg.norm(lost[:3, 3] - G_TRUE[:3, 3])
    # extra poses are appended after the lattice; the default points are object_cloud; neither given: ValueError
    got_e = tracker.recover(lost, rgb, depth, refine=0, extra=[G_TRUE], **kw)
    assert tracker.last_recover["n"] == 9318
    want_e = PSO.score(pts, np.concatenate([c["lattice"], G_TRUE[None]]), depth, K, TOL)
    assert np.array_equal(tracker.last_recover["top_idx"], PSO.rank(want_e, 8))
    assert np.array_equal(got_e, np.concatenate([c["lattice"], G_TRUE[None]])[PSO.rank(want_e, 1)[0]])
    cloud = np.asarray(tracker.object_cloud.points, np.float64)
    got_c = tracker.recover(lost, rgb, depth, refine=0, trans_radius=0.02, tol_mm=TOL)
    lat_c = PSO.lattice(lost, 2, STEP, ROT_DEG)
    assert np.array_equal(got_c, lat_c[PSO.rank(PSO.score(cloud, lat_c, depth, K, TOL), 1)[0]])
    keep, tracker.object_cloud, tracker._model_points = (tracker.object_cloud, tracker._model_points), None, None
    try:
        with pytest.raises(ValueError):
            tracker.recover(lost, rgb, depth)
    finally:
        tracker.object_cloud, tracker._model_points = keep
    mp.close()


def test_live_tracker_recovers_when_the_fit_drops(se3, tracker, frame):
    rgb, depth = frame
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    lost = lost_pose(0)
    with pytest.raises(ValueError):
        se3.LiveTracker(tracker, lost, recover_below=0.3)            # needs the fit check
    tracker.fit_check = 20
    try:
        # recover_below = None: the bits of today's on_track
        plain = se3.LiveTracker(tracker, lost)
        plain.grab_depth(depth); plain.grab_color(bgr, 1.0)
        filled = plain.depth.copy()
        t0, q0, s0 = plain.on_track()
        ratio = tracker.last_fit_ratio
        direct = tracker.on_track(lost, rgb, filled)
        assert np.array_equal(plain.A_in_cam, direct) and np.array_equal(t0, direct[:3, 3]) and tracker.last_fit_ratio == ratio
        # recover_below at or below the frame's ratio: nothing more happens either
        same = se3.LiveTracker(tracker, lost, recover_below=ratio)
        same.grab_depth(depth); same.grab_color(bgr, 1.0)
        same.on_track()
        assert np.array_equal(same.A_in_cam, direct)
        # above it: the recovered pose is adopted -- Tracker.recover around the pose the frame started from, the estimate among the candidates
        live = se3.LiveTracker(tracker, lost, recover_below=float(np.nextafter(ratio, 2.0)))
        live.grab_depth(depth); live.grab_color(bgr, 1.0)
        t1, q1, s1 = live.on_track()
        assert tracker.last_recover["n"] == 9318
        want = tracker.recover(lost, rgb, filled, extra=[direct])
        assert np.array_equal(live.A_in_cam, want) and np.array_equal(t1, want[:3, 3])
    finally:
        tracker.fit_check = None


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_tracking_and_scoring(se3, tracker, frame):
    eng, lib, L = tracker.engine, tracker.engine.lib, se3._lib
    rgb, depth = frame
    prev = Fx.pose(11, (0.004, -0.003, 0.5))
    pts = subsample(257)
    rng = np.random.default_rng(12)
    poses = np.array([moved(G_TRUE, unit(rng) * rng.uniform(0, 0.3), rng.uniform(-0.05, 0.05, 3)) for _ in range(9)])
    mp = eng.model_points(pts)
    pose0 = tracker.on_track(prev, rgb, depth)
    score0 = eng.score_poses(mp, poses, depth, K, TOL, top=4)
    same_records(score0[1], PSO.score(pts, poses, depth, K, TOL)[score0[0]], "before")

    def still_right(what):
        assert np.array_equal(tracker.on_track(prev, rgb, depth), pose0), what
        got = eng.score_poses(mp, poses, depth, K, TOL, top=4)
        assert np.array_equal(got[0], score0[0]) and got[1].tobytes() == score0[1].tobytes(), what

    p16 = np.ascontiguousarray(poses.reshape(-1, 16))
    Kh = np.ascontiguousarray(K.reshape(9))
    Kp = Kh.ctypes.data_as(C.POINTER(C.c_double))
    idx, fit = np.full(64, -1, np.int32), np.zeros(64, L.POINT_FIT_DTYPE)
    hp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    dp = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
    poses_d, depth_d = torch.from_numpy(p16).cuda(), torch.from_numpy(depth.view(np.int16)).cuda()
    fit_d = torch.zeros((9, 8), dtype=torch.int32, device="cuda")
    idx_d = torch.zeros((64,), dtype=torch.int32, device="cuda")

    def host(n=9, k=4, tol=TOL, h=H, w=W, p=hp(p16), d=hp(depth), Kq=Kp, pts_h=mp._h, io=hp(idx), fo=hp(fit)):
        return lib.se3tn_search_poses_host(eng._h, pts_h, n, p, d, h, w, Kq, tol, k, io, fo, None)

    def dev(n=9, tol=TOL, h=H, w=W, p=dp(poses_d), d=dp(depth_d), Kq=Kp, pts_h=mp._h, fo=dp(fit_d)):
        return lib.se3tn_score_poses(eng._h, pts_h, n, p, d, h, w, Kq, tol, fo, None)

    assert host() == 0 and dev() == 0                                               # the defaults of these helpers are a good call
    for n in (0, -3, L.POSE_SEARCH_MAX_POSES + 1):
        assert host(n=n) == E_ARG and dev(n=n) == E_ARG
        assert lib.se3tn_rank_poses(eng._h, n, dp(fit_d), 1, dp(idx_d), None) == E_ARG
    assert b"SE3TN_POSE_SEARCH_MAX_POSES" in lib.se3tn_last_error()
    still_right("after a bad n")
    for k in (0, -1, 10, 65):                                                       # k > n = 9, k > 64
        assert host(k=k) == E_ARG and lib.se3tn_rank_poses(eng._h, 9, dp(fit_d), k, dp(idx_d), None) == E_ARG
    still_right("after a bad k")
    for tol in (0, -5, 65536):
        assert host(tol=tol) == E_ARG and dev(tol=tol) == E_ARG
    assert host(h=0) == E_ARG and host(w=0) == E_ARG and dev(h=-1) == E_ARG and dev(w=0) == E_ARG
    still_right("after a bad tolerance or frame size")
    for kw in (dict(p=None), dict(d=None), dict(Kq=None), dict(pts_h=None), dict(io=None), dict(fo=None)):
        assert host(**kw) == E_ARG, kw
    for kw in (dict(p=None), dict(d=None), dict(Kq=None), dict(pts_h=None), dict(fo=None)):
        assert dev(**kw) == E_ARG, kw
    assert lib.se3tn_rank_poses(eng._h, 9, None, 4, dp(idx_d), None) == E_ARG and lib.se3tn_rank_poses(eng._h, 9, dp(fit_d), 4, None, None) == E_ARG
    still_right("after NULL pointers")
    for bad in (np.nan, np.inf, -np.inf):
        broken = poses.copy()
        broken[2, 1, 3] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*pose 2" % E_ARG):
            eng.score_poses(mp, broken, depth, K, TOL, top=4)
        Kb = K.copy()
        Kb[1, 1] = bad
        with pytest.raises(L.Se3tnError, match="rc=%d.*K entry 4" % E_ARG):
            eng.score_poses(mp, poses, depth, Kb, TOL, top=4)
    still_right("after a pose or a K that is not finite")
    # row 3 of a pose is not read
    odd = poses.copy()
    odd[:, 3, :] = [7.0, -2.0, 0.5, 3.0]
    got = eng.score_poses(mp, odd, depth, K, TOL, top=4)
    assert np.array_equal(got[0], score0[0]) and got[1].tobytes() == score0[1].tobytes()
    # the host variant waits for its stream: inside a capture it says so and leaves the capture whole
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1.0)
        with pytest.raises(L.Se3tnError, match="rc=%d" % E_STATE):
            eng.score_poses(mp, poses, depth, K, TOL, top=4)
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    still_right("after the refused capture")
    mp.close()
