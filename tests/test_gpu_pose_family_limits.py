"""GPU: the pose-search family at the sizes include/se3tracknet.h admits -- se3tn_score_poses / se3tn_rank_poses /
se3tn_search_poses_host, se3tn_score_pose_grid / se3tn_search_pose_grid_host and the _scene form, se3tn_align_poses and its _scene
form, se3tn_pose_errors -- and their outputs in mapped pinned host memory.  tests/test_pose_family_limits_plan.py (no GPU) derives
the sizes and shows every 32-bit expression of the kernels in range at them; the lists come from tests/pose_family_limits.py.

The yardsticks are the family's numpy oracles (pose_search_oracle, pose_grid_oracle, scene_search_oracle, pose_align_oracle,
scene_align_oracle) and metrics.add / metrics.adi, never the library.  Every comparison of records, indices, poses and sums is an
EQUALITY.  Where n is at its limit the oracle does not walk n x P points: the n slots are filled from a small pool of distinct inputs
by a seeded draw (every member present, first and last slot different); the header guarantees that a record depends on its own
inputs alone, so every slot must equal its pool member's oracle record word for word -- one gather and one torch.equal on the
device, and slots 0, n - 1 and a few seeded ones on the host as well.  The one floating-point comparison (ADD / ADD-S at 2^20 points)
carries a derived bound and prints the measured distance.

Each case prints its time and the peak device memory; no test asserts a time."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch
from scipy import spatial
from scipy.spatial.transform import Rotation

import color_fit_oracle as CO
import pose_align_cases as CS
import pose_align_oracle as PAO
import pose_family_limits as PL
import pose_grid_oracle as PGO
import pose_grid_scene as SC
import pose_search_cases as PC
import pose_search_oracle as PSO
import scene_align_oracle as SAO
import scene_search_oracle as SSO
from mapped_memory import Mapped

pytestmark = pytest.mark.gpu

E_ARG = -1
P20 = PL.P20
H, W = PL.SMALL_HW
K = np.array([[100.0, 0, 79.5], [0, 100.0, 59.5], [0, 0, 1.0]])
TOL = 5
BLOCK = (slice(40, 81), slice(55, 106))      # a block of the small frame at 500 mm without holes: what the flat patch is seen against


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, 1)
    yield e
    e.close()


class Clock:
    """prints what a case took (device work included) and the peak device memory since it began"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        print("[limits] %s: %.3f s, peak device memory %.2f GB" % (self.what, time.perf_counter() - self.t,
                                                                    torch.cuda.max_memory_allocated() / 2 ** 30))


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def words(rec):
    """a structured array of 32-bit records as an int32 tensor [n, words] on the device"""
    n = len(rec)
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint32).reshape(n, -1).view(np.int32).copy()).cuda()


def small_frame():
    """120 x 160: a tilted wall around 520 mm with 4 % holes and the validity thresholds sprinkled in, and BLOCK at exactly 500 mm"""
    rng = np.random.default_rng(160)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (520 + 0.5 * (xx - W / 2) + 0.3 * (yy - H / 2) + 9 * np.sin(xx / 6.0)).astype(np.uint16)
    mask = rng.random((H, W)) < 0.08
    d[mask] = rng.choice(np.array([0, 0, 0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    d[BLOCK] = 500
    return np.ascontiguousarray(d)


def ellipsoid(P, seed=0):
    """P points on an ellipsoid of half axes 50 x 35 x 25 mm and their outward unit normals"""
    rng = np.random.default_rng(1000 + P + seed)
    v = rng.normal(size=(P, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ax = np.array([0.05, 0.035, 0.025])
    nrm = v / ax
    return np.ascontiguousarray(v * ax), np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))


def patch(z=0.0, offset=(0.0, 0.0)):
    """2^20 points of a flat 60 x 40 mm patch in the plane z (a 1,024 x 1,024 lattice), normals (0, 0, -1): towards a camera in front"""
    gx, gy = np.meshgrid(np.linspace(-0.03, 0.03, 1024) + offset[0], np.linspace(-0.02, 0.02, 1024) + offset[1], indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), np.full(P20, float(z))], 1)
    return np.ascontiguousarray(pts), np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (P20, 1)))


def rigid(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix()
    T[:3, 3] = t
    return T


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


G0 = rigid((0.3, -0.2, 0.1), (0.004, -0.003, 0.5))


def pose_pool(finite=False):
    """64 distinct poses: 61 around G0 (up to 0.6 rad, 40 mm), one behind the camera, one with a NaN (a finite far one instead where
    the entry point inspects its poses), one off the frame"""
    rng = np.random.default_rng(64)
    out = [G0] + [rigid(unit(rng) * rng.uniform(0, 0.6), G0[:3, 3] + rng.uniform(-0.04, 0.04, 3)) for _ in range(60)]
    behind, nan, off = G0.copy(), G0.copy(), G0.copy()
    behind[2, 3] = -0.5
    if finite:
        nan[:3, 3] = (0.0, 0.0, 1.9)
    else:
        nan[1, 1] = np.nan
    off[0, 3] = 2.0
    out += [behind, nan, off]
    assert len(out) == 64
    return np.ascontiguousarray(np.array(out))


def check_slots(idx, pool):
    assert set(idx.tolist()) == set(range(pool)) and idx[0] != idx[-1]


def host_slots(n, seed):
    rng = np.random.default_rng(seed)
    return sorted({0, n - 1, *rng.integers(0, n, 6).tolist()})


def same_records(got, want, what):
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])


# ---- score ----------------------------------------------------------------------------------------------------------------------------
def test_score_at_2_20_poses(se3, eng):
    """se3tn_score_poses, n = 2^20 (grid.x = 2^20 workgroups; blockIdx.x a pose offset of 16 doubles and a record offset of 8 words),
    P = 65"""
    c = PL.SCORE_CASES[0]
    n, P = c["n"], c["P"]
    pts, _ = ellipsoid(P)
    depth, pool = small_frame(), pose_pool()
    want = PSO.score(pts, pool, depth, K, TOL)
    PSO.check_invariants(want, P, TOL)
    assert list(want["in_frame_pts"][61:]) == [0, 0, 0] and want["inlier_pts"][:61].max() > 0
    assert len({w.tobytes() for w in want}) > 32                               # a slot holding the wrong member's record would show
    idx = PL.slot_assignment(n, 64, seed=1)
    check_slots(idx, 64)
    mp = eng.model_points(pts)
    with Clock("score n = 2^20, P = 65"):
        idx_d = torch.from_numpy(idx).cuda()
        poses_d = torch.from_numpy(pool.reshape(64, 16)).cuda()[idx_d].contiguous()
        fit = eng.score_poses(mp, poses_d, dev16(depth), K, TOL)
        assert tuple(fit.shape) == (n, 8) and torch.equal(fit, words(want)[idx_d])
    for s in host_slots(n, 2):
        same_records(fit[s:s + 1].cpu().numpy().view(PSO.DTYPE).reshape(1), want[idx[s]:idx[s] + 1], s)
    mp.close()


@pytest.fixture(scope="module")
def big_patch_score():
    """the three poses of the P = 2^20 score case and the oracle's records: the patch seen frontally at 500 mm against BLOCK (every
    point an inlier), at 300 mm (the sensor sees 500 through every point: all behind), and tilted over the wall's holes"""
    pts, nrm = patch()
    poses = np.array([rigid((0, 0, 0), (0, 0, 0.5)), rigid((0, 0, 0), (0, 0, 0.3)), rigid((0.5, -0.4, 0.2), (0.12, 0.07, 0.52))])
    depth = small_frame()
    want = PSO.score(pts, poses, depth, K, TOL)
    return dict(pts=pts, nrm=nrm, poses=poses, depth=depth, want=want)


def test_score_at_2_20_points(se3, eng, big_patch_score):
    """se3tn_score_poses, P = 2^20 (4,096 points per thread; the uint32 lane counts reach 2^14, the record's words 2^20), n = 3;
    then se3tn_rank_poses on those records: the key's top field at exactly 2^20"""
    b = big_patch_score
    want = b["want"]
    PSO.check_invariants(want, P20, TOL)
    assert want["inlier_pts"][0] == P20 and want["behind_pts"][1] == P20 and want["seen_pts"][1] == P20
    assert 0 < want["seen_pts"][2] < want["in_frame_pts"][2] and min(want[k][2] for k in ("inlier_pts", "front_pts", "behind_pts")) > 0
    mp = eng.model_points(b["pts"])
    with Clock("score P = 2^20, n = 3 (+ rank)"):
        poses_d = torch.from_numpy(b["poses"].reshape(3, 16)).cuda()
        idx_t, top_t = eng.score_poses(mp, poses_d, dev16(b["depth"]), K, TOL, top=3)
        fit = eng.score_poses(mp, poses_d, dev16(b["depth"]), K, TOL)
    same_records(fit.cpu().numpy().view(PSO.DTYPE).reshape(3), want, "P = 2^20")
    order = PSO.rank(want, 3)
    assert np.array_equal(idx_t.cpu().numpy(), order) and order[0] == 0
    same_records(top_t.cpu().numpy().view(PSO.DTYPE).reshape(3), want[order], "top")
    assert PSO.key(want["inlier_pts"][0], want["behind_pts"][0], 0) == PL.KEY_MAX
    mp.close()


def test_search_poses_host_at_2_20_poses_then_a_small_call(se3, eng):
    """se3tn_search_poses_host, n = 2^20, k = 64: 128 MB of poses staged, 32 MB of records ranked on the device, 64 winners read back;
    then a small call on the same context, on the grown staging"""
    c = PL.SEARCH_HOST_CASE
    n, P, k = c["n"], c["P"], c["k"]
    pts, _ = ellipsoid(P)
    depth, pool = small_frame(), pose_pool(finite=True)
    want = PSO.score(pts, pool, depth, K, TOL)
    idx = PL.slot_assignment(n, 64, seed=3)
    check_slots(idx, 64)
    full = want[idx]
    order = PL.rank_fast(full["inlier_pts"], full["behind_pts"], k)
    assert order.max() > 64                                                     # the winners are not simply the first slots
    mp = eng.model_points(pts)
    with Clock("search_poses_host n = 2^20, k = 64"):
        got_idx, got_fit = eng.score_poses(mp, pool[idx], depth, K, TOL, top=k)
    assert np.array_equal(got_idx, order)
    same_records(got_fit, full[order], "host")
    small_idx, small_fit = eng.score_poses(mp, pool[:37], depth, K, TOL, top=8)
    assert np.array_equal(small_idx, PSO.rank(want[:37], 8))
    same_records(small_fit, want[:37][small_idx], "small call after the large one")
    mp.close()


# ---- rank -----------------------------------------------------------------------------------------------------------------------------
def rank_device(eng, fit, k):
    n = len(fit)
    fit_d = words(fit)
    idx_d = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    rc = eng.lib.se3tn_rank_poses(eng._h, n, C.c_void_p(fit_d.data_ptr()), k, C.c_void_p(idx_d.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.se3tn_last_error()
    return idx_d.cpu().numpy()


def expected_rank(fit, k):
    """the oracle's order; inlier_pts above 2^20 -- which se3tn_score_poses never writes -- count as 2^20 (include/se3tracknet.h)"""
    return PL.rank_fast(np.minimum(fit["inlier_pts"], P20), fit["behind_pts"], k)


def test_rank_at_the_field_limits(se3, eng):
    """se3tn_rank_poses, n = 2^20, k = 64 (index 2^20 - 1, 4,096 strided records per thread, 64 rounds) on synthetic records that carry
    the extremes of both fields.
      * drawn: every record from INLIER_EXTREMES x BEHIND_EXTREMES -- ties down to the index among 2^20 / 25 equal pairs;
      * low: the all-zero key (no inliers, behind >= 2^20 - 1, index 2^20 - 1) is in the call.  It is the LAST of the 2^20 records
        of any call, so with k <= 64 it can be no winner (the issue asks for it as the k-th winner; no admitted call has one).  What
        is run instead is the nearest reachable case: every record but 63 has a key whose two upper fields are zero, so the 64th
        winner is the one of them with the lowest index, and the rounds pass over the zero key 64 times without taking it;
      * last: the 64 winners lie among the last 256 records."""
    n, k = PL.RANK_CASE["n"], PL.RANK_CASE["k"]
    rng = np.random.default_rng(20)
    drawn = np.zeros(n, PSO.DTYPE)
    drawn["points"] = P20
    drawn["inlier_pts"] = rng.choice(PL.INLIER_EXTREMES, n)
    drawn["behind_pts"] = rng.choice(PL.BEHIND_EXTREMES, n)
    low = np.zeros(n, PSO.DTYPE)
    low["behind_pts"] = rng.choice(PL.BEHIND_EXTREMES[2:], n)
    winners = rng.choice(np.arange(1, n - 1), 63, replace=False)
    low["inlier_pts"][winners] = rng.choice(np.array([1, P20 - 1, P20], np.uint32), 63)
    low["behind_pts"][winners] = rng.choice(PL.BEHIND_EXTREMES, 63)
    assert PSO.key(low["inlier_pts"][n - 1], low["behind_pts"][n - 1], n - 1) == 0
    last = np.zeros(n, PSO.DTYPE)
    last["inlier_pts"] = rng.integers(0, 2, n)
    last["behind_pts"] = rng.choice(PL.BEHIND_EXTREMES, n)
    tail = n - 256 + rng.choice(256, 80, replace=False)
    last["inlier_pts"][tail] = rng.choice(PL.INLIER_EXTREMES[2:], 80)
    for name, fit in (("drawn", drawn), ("low", low), ("last", last)):
        want = expected_rank(fit, k)
        with Clock("rank n = 2^20, k = 64 (%s)" % name):
            got = rank_device(eng, fit, k)
        assert np.array_equal(got, want), (name, got, want)
        if name == "low":
            assert set(want[:63].tolist()) == set(winners.tolist()) and want[63] == 0 and n - 1 not in want
        if name == "last":
            assert want.min() >= n - 256
    # a small call holds PSO.rank itself on the same kind of records (inliers up to 2^20: no clamp at work)
    small = drawn[:1000].copy()
    small["inlier_pts"] = np.minimum(small["inlier_pts"], P20)
    assert np.array_equal(rank_device(eng, small, 64), PSO.rank(small, 64))


# ---- grid -----------------------------------------------------------------------------------------------------------------------------
def factor_pools():
    """16 rotations (the identity first) and 16 translations around 0.5 m (one behind the camera, one far off the frame)"""
    rng = np.random.default_rng(16)
    rots = np.concatenate([np.eye(3)[None], Rotation.from_rotvec(rng.normal(size=(15, 3))).as_matrix()])
    trans = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, (16, 3))
    trans[5] = (0.0, 0.0, -0.5)
    trans[9] = (2.0, 0.0, 0.5)
    return np.ascontiguousarray(rots), np.ascontiguousarray(trans)


@pytest.fixture(scope="module")
def grid_pool():
    """the oracle's records of the 16 x 16 product, facing 0 and 1, P = 1,025"""
    pts, nrm = ellipsoid(PL.GRID_P)
    rots, trans = factor_pools()
    depth = small_frame()
    want = {f: PGO.score(pts, nrm, rots, trans, depth, K, TOL, f) for f in (0, 1)}
    for f in (0, 1):
        PGO.check_invariants(want[f], PL.GRID_P, TOL, f)
        assert len({w.tobytes() for w in want[f]}) > 128
    return dict(pts=pts, nrm=nrm, rots=rots, trans=trans, depth=depth, want=want)


def factor_slots(n_rot, n_trans):
    ridx, tidx = PL.slot_assignment(n_rot, 16, seed=n_rot), PL.slot_assignment(n_trans, 16, seed=n_trans + 1)
    for idx in (ridx, tidx):
        if len(idx) >= 16:
            check_slots(idx, 16)
    return ridx, tidx


@pytest.mark.parametrize("n_rot,n_trans", PL.GRID_FACTORS)
def test_grid_factorisations_of_2_20(se3, eng, grid_pool, n_rot, n_trans):
    """se3tn_score_pose_grid with n_rot * n_trans at (or 47 below) 2^20, facing 0 and 1: the one-dimensional block index divided by
    pg_tiles(n_trans) from 1 to 65,536 tiles.  Slot (r, t) holds pool members (ridx[r], tidx[t]): its record must be the oracle's of
    that pair of the 16 x 16 product."""
    g = grid_pool
    ridx, tidx = factor_slots(n_rot, n_trans)
    mp = eng.model_points(g["pts"], g["nrm"])
    r_d, t_d = torch.from_numpy(ridx).cuda(), torch.from_numpy(tidx).cuda()
    rots_d = torch.from_numpy(g["rots"].reshape(16, 9)).cuda()[r_d].contiguous()
    trans_d = torch.from_numpy(g["trans"]).cuda()[t_d].contiguous()
    member = (r_d[:, None] * 16 + t_d[None, :]).reshape(-1)
    for facing in (0, 1):
        with Clock("grid %d x %d, facing %d" % (n_rot, n_trans, facing)):
            fit = eng.score_pose_grid(mp, rots_d, trans_d, dev16(g["depth"]), K, TOL, facing=bool(facing))
            assert tuple(fit.shape) == (n_rot * n_trans, 8) and torch.equal(fit, words(g["want"][facing])[member])
        for s in host_slots(n_rot * n_trans, n_rot):
            m = ridx[s // n_trans] * 16 + tidx[s % n_trans]
            same_records(fit[s:s + 1].cpu().numpy().view(PSO.DTYPE).reshape(1), g["want"][facing][m:m + 1], (facing, s))
    mp.close()


def test_grid_refuses_a_product_above_2_20(se3, eng, grid_pool):
    """65,537 x 16 = 2^20 + 16 candidates: refused with the limit's name, nothing launched"""
    n_rot, n_trans = PL.GRID_REFUSED
    g = grid_pool
    mp = eng.model_points(g["pts"], g["nrm"])
    rots_d = torch.from_numpy(np.tile(np.eye(3).reshape(1, 9), (n_rot, 1))).cuda()
    trans_d = torch.from_numpy(g["trans"][:n_trans].copy()).cuda()
    with pytest.raises(se3._lib.Se3tnError, match="SE3TN_POSE_SEARCH_MAX_POSES"):
        eng.score_pose_grid(mp, rots_d, trans_d, dev16(g["depth"]), K, TOL)
    mp.close()


def test_grid_scene_at_2_20_candidates_on_2_21_pixels(se3, eng):
    """se3tn_score_pose_grid_scene, 1,024 x 1,024 candidates on a 1,024 x 2,048 frame (2^21 pixels).  The scene values are written
    directly: a tracked surface in front of part of the object (hidden), one behind another part (not hidden), the validity
    thresholds sprinkled over the rest."""
    c = PL.GRID_SCENE_CASE
    Hs, Ws, n_rot, n_trans = c["H"], c["W"], c["n_rot"], c["n_trans"]
    Ks = np.array([[1000.0, 0, 1023.5], [0, 1000.0, 511.5], [0, 0, 1.0]])
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    depth = (500 + 30 * np.sin(xx / 37.0) + 20 * np.cos(yy / 29.0)).astype(np.uint16)
    mask = rng.random((Hs, Ws)) < 0.04
    depth[mask] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    scene = np.zeros((Hs, Ws), np.uint16)
    scene[:, 930:1000] = 455
    scene[:, 1040:1100] = 560
    mask = rng.random((Hs, Ws)) < 0.02
    scene[mask] = rng.choice(np.array([100, 101, 480, 1999, 2000], np.uint16), int(mask.sum()))
    pts, nrm = ellipsoid(c["P"])
    rots, trans = factor_pools()
    ridx, tidx = factor_slots(n_rot, n_trans)
    mp = eng.model_points(pts, nrm)
    r_d, t_d = torch.from_numpy(ridx).cuda(), torch.from_numpy(tidx).cuda()
    rots_d = torch.from_numpy(rots.reshape(16, 9)).cuda()[r_d].contiguous()
    trans_d = torch.from_numpy(trans).cuda()[t_d].contiguous()
    member = (r_d[:, None] * 16 + t_d[None, :]).reshape(-1)
    for facing in (0, 1):
        want = SSO.score(pts, nrm, rots, trans, depth, scene, Ks, TOL, facing)
        SSO.check_invariants(want, c["P"], TOL, facing)
        assert want["hidden_pts"].max() > 0 and want["inlier_pts"].max() > 0 and len({w.tobytes() for w in want}) > 128
        with Clock("grid scene 1,024 x 1,024 on 1,024 x 2,048, facing %d" % facing):
            fit = eng.score_pose_grid(mp, rots_d, trans_d, dev16(depth), Ks, TOL, facing=bool(facing), scene=dev16(scene))
            assert torch.equal(fit, words(want)[member])
    mp.close()


def test_grid_at_2_20_points(se3, eng):
    """se3tn_score_pose_grid, P = 2^20 on a 2 x 17 grid, facing 1: 1,024 LDS point tiles per workgroup, the LDS rows accumulated once
    per tile up to 2^20; under the identity every point of the patch faces, points == 2^20"""
    c = PL.GRID_BIG_P_CASE
    pts, _ = patch()
    nrm = np.stack([20.0 * pts[:, 0], 20.0 * pts[:, 1], np.full(P20, -1.0)], 1)          # a fan of normals, up to 36 degrees off the patch's
    nrm = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    rng = np.random.default_rng(17)
    rots = np.stack([np.eye(3), Rotation.from_rotvec((1.5, -0.4, 0.2)).as_matrix()])
    trans = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.04, 0.04, (c["n_trans"], 3))
    trans[0] = (0.0, 0.0, 0.5)
    trans[3] = (0.0, 0.0, -0.5)
    depth = small_frame()
    want = PGO.score(pts, nrm, rots, trans, depth, K, TOL, 1, chunk=4)
    PGO.check_invariants(want, P20, TOL, 1)
    assert (np.delete(want["points"][:17], 3) == P20).all() and want["points"][3] == 0          # (translation 3 is behind the camera)
    assert want["inlier_pts"][0] == P20 and 0 < want["points"][17:].max() < P20
    mp = eng.model_points(pts, nrm)
    with Clock("grid P = 2^20, 2 x 17, facing 1"):
        got = eng.score_pose_grid(mp, rots, trans, depth, K, TOL, facing=True)
    same_records(got, want, "P = 2^20")
    mp.close()


def test_search_pose_grid_host_at_2_20_candidates(se3, eng, grid_pool):
    """se3tn_search_pose_grid_host, 1,024 x 1,024, k = 64, facing 1"""
    c = PL.GRID_HOST_CASE
    g = grid_pool
    n_rot, n_trans, k = c["n_rot"], c["n_trans"], c["k"]
    ridx, tidx = factor_slots(n_rot, n_trans)
    full = g["want"][1][(ridx[:, None] * 16 + tidx[None, :]).reshape(-1)]
    order = PL.rank_fast(full["inlier_pts"], full["behind_pts"], k)
    mp = eng.model_points(g["pts"], g["nrm"])
    with Clock("search_pose_grid_host 1,024 x 1,024, k = 64"):
        idx, fit = eng.score_pose_grid(mp, g["rots"][ridx], g["trans"][tidx], g["depth"], K, TOL, facing=True, top=k)
    assert np.array_equal(idx, order)
    same_records(fit, full[order], "host")
    mp.close()


# ---- align ----------------------------------------------------------------------------------------------------------------------------
def align_device(eng, mp, poses_d, depth, Kc, scene=None, **prm):
    kw = dict(scene=dev16(scene)) if scene is not None else {}
    return eng.align_poses(mp, poses_d, dev16(depth), Kc, sums=True, **prm, **kw)


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("with_scene", [False, True])
def test_align_at_4096_poses_and_64_iterations(se3, eng, with_scene):
    """se3tn_align_poses / se3tn_align_poses_scene, n = 4,096, iters = 64, stop = 0 (no pose converges early: those that pair walk all
    64 iterations), P = 257, slots from the 65 poses of tests/test_gpu_pose_align.py.  Poses (as bits: one carries a NaN), records and
    sums of every slot equal the oracle's of its pool member."""
    from test_gpu_pose_align import cloud
    c = PL.ALIGN_CASE
    n = c["n_align"]
    pts, nrm = cloud(c["P"])
    depth = CS.l_scene()[2]
    pool = np.ascontiguousarray(np.array([*CS.perturbed(61, seed=3), *CS.bad_poses(), SC.true_pose()]))
    prm = dict(gate_mm=20, iters=c["iters"], min_pairs=6, damping=1e-6, stop=0.0)
    if with_scene:
        scene = np.zeros_like(depth)
        scene[:, 80:] = depth[:, 80:]                    # a tracked surface where the right half of the frame is: points there are hidden
        want = SAO.align(pts, nrm, pool, depth, scene, SC.K, scene_tol_mm=10, **prm)
        assert want[1]["hidden_pts"].max() > 0
    else:
        scene = None
        want = PAO.align(pts, nrm, pool, depth, SC.K, **prm)
    assert len(pool) == 65 and (want[1]["iterations"][:61] == 64).sum() > 30 and list(want[1]["status"][61:64]) == [PAO.FEW] * 3
    idx = PL.slot_assignment(n, 65, seed=65)
    check_slots(idx, 65)
    mp = eng.model_points(pts, nrm)
    with Clock("align%s n = 4,096, iters = 64, P = 257" % (" scene" if with_scene else "")):
        idx_d = torch.from_numpy(idx).cuda()
        poses_d = torch.from_numpy(pool.reshape(65, 16)).cuda()[idx_d].contiguous()
        out, rec, sums = align_device(eng, mp, poses_d, depth, SC.K, scene=scene, **prm, **(dict(scene_tol_mm=10) if with_scene else {}))
        assert torch.equal(bits(out.reshape(n, 16)), bits(torch.from_numpy(want[0].reshape(65, 16)).cuda())[idx_d])
        assert torch.equal(rec, torch.from_numpy(want[1].view(np.uint8).reshape(65, 40).copy()).cuda()[idx_d])
        assert torch.equal(sums, torch.from_numpy(want[2]).cuda()[idx_d])
    for s in host_slots(n, 4096):
        assert out[s].cpu().numpy().tobytes() == want[0][idx[s]].tobytes() and rec[s].cpu().numpy().tobytes() == want[1][idx[s]].tobytes(), s
    mp.close()


def test_align_at_2_20_points(se3, eng):
    """se3tn_align_poses, P = 2^20, n = 2, iters = 3, sums requested: the patch against BLOCK from two tilted poses a few millimetres
    off; every point pairs, the 28 int64 sums run over 2^20 terms each"""
    c = PL.ALIGN_BIG_P_CASE
    pts, nrm = patch()
    depth = small_frame()
    poses = np.array([rigid((0.035, 0, 0), (0.001, 0, 0.503)), rigid((0, -0.026, 0.01), (0, -0.001, 0.497))])
    prm = dict(gate_mm=20, iters=c["iters"], min_pairs=6, damping=1e-6, stop=0.0)
    want = PAO.align(pts, nrm, poses, depth, K, **prm)
    assert (want[1]["pairs0"] == P20).all() and (want[1]["iterations"] == 3).all() and (want[1]["status"] == PAO.ITERS).all()
    mp = eng.model_points(pts, nrm)
    with Clock("align P = 2^20, n = 2, iters = 3"):
        out, rec, sums = align_device(eng, mp, torch.from_numpy(poses.reshape(2, 16)).cuda(), depth, K, **prm)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and rec.cpu().numpy().tobytes() == want[1].tobytes()
    assert np.array_equal(sums.cpu().numpy(), want[2])
    mp.close()


def test_align_sums_at_the_clamp(se3, eng):
    """Every one of the 28 terms of every one of 2^20 paired points cut at +-256: the sums reach +-2^60, in both signs, through
    wave_sum and the LDS rows.  Model coordinates of tens of metres (q = (30, 40, 50) + the patch), normals (17, 17, -17) -- 17 * 17 >
    256, so the products of the normal's components clamp too, which normals of length 20 could not all do -- the pose brings the
    patch to 60 m on the optical axis, gate_mm = 65,535 pairs it with the 500 mm of BLOCK (r = 1,011 m).  damping = 1,000 lifts the
    rank-one system so that the solve proceeds; with iters = 1 the oracle ends in SE3TN_ALIGN_ITERS."""
    pts, _ = patch(z=50.0, offset=(30.0, 40.0))
    nrm = np.ascontiguousarray(np.tile([17.0, 17.0, -17.0], (P20, 1)))
    pose = rigid((0, 0, 0), (-30.0, -40.0, 10.0))[None]
    depth = small_frame()
    prm = dict(gate_mm=65535, iters=1, min_pairs=6, damping=1000.0, stop=0.0)
    want = PAO.align(pts, nrm, pose, depth, K, **prm)
    assert want[1]["pairs"][0] == P20 and want[1]["status"][0] == PAO.ITERS and want[1]["sum_r2"][0] == 2 ** 60
    assert (np.abs(want[2][0]) == P20 << 40).all() and (want[2][0] > 0).sum() >= 8 and (want[2][0] < 0).sum() >= 8
    mp = eng.model_points(pts, nrm)
    with Clock("align clamp P = 2^20"):
        out, rec, sums = align_device(eng, mp, torch.from_numpy(pose.reshape(1, 16)).cuda(), depth, K, **prm)
    assert np.array_equal(sums.cpu().numpy(), want[2])
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and rec.cpu().numpy().tobytes() == want[1].tobytes()
    mp.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
ERR_RADIUS = 0.1
ERR_CHAIN = 4 + 6 + 4 + 1024      # additions on the kernel's longest chain: a thread's 4 slots, 6 shuffle steps, 4 waves, 1,024 tiles in order


def err_pair(rng, d):
    """tests/test_gpu_pose_errors.py's pair: no model point moves by more than 0.95 d"""
    gt = rigid(unit(rng) * rng.uniform(0.5, 3.0), [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.5, 2.5)])
    return gt @ rigid(unit(rng) * min(3.0, 0.25 * d / ERR_RADIUS), unit(rng) * 0.7 * d), gt


def err_cloud(P):
    rng = np.random.default_rng(1000 + P)
    v = rng.normal(size=(P, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * ERR_RADIUS * rng.uniform(0.2, 1.0, (P, 1))


def test_pose_errors_at_2_20_points(se3, eng):
    """se3tn_pose_errors, P = 2^20: 1,024 query tiles x 1,024 reference tiles, ADD and ADD-S of two pairs (displacements 5 mm and 0.3 m)
    and of an equal pair, which must give exactly 0.0 twice.

    The yardstick is metrics.add / metrics.adi: the same per-point distances (metrics._transform, the KD-tree), their mean formed with
    math.fsum so that it is the correctly rounded mean and only the kernel's rounding enters.  Bound, derived for these shapes
    (coordinates <= 4 m, distances <= S = 1 m, asserted): the kernel adds non-negative terms along a tree whose longest chain has
    ERR_CHAIN = 4 + 6 + 4 + 1,024 = 1,038 additions, each rounding by at most 2^-53 of a partial sum <= P S, so the sum is off by at
    most 1,038 * 2^-53 * P S and the mean by 1,038 * 2^-53 * S = 1.15e-13; the division adds 2^-53 S; the transform and distance
    roundings of a term, about 1.3e-14 m as in tests/test_gpu_pose_errors.py, pass into the mean unamplified.  1.3e-13 m in all."""
    P = PL.ERRORS_BIG_P_CASE["P"]
    S = 1.0
    bound = (ERR_CHAIN + 1) * 2.0 ** -53 * S + 1.3e-14
    pts = err_cloud(P)
    rng = np.random.default_rng(P)
    pairs = [err_pair(rng, 5e-3), err_pair(rng, 0.3)]
    pairs.append((pairs[0][1], pairs[0][1].copy()))
    preds, gts = np.array([p for p, _ in pairs]), np.array([g for _, g in pairs])
    want_add, want_adds = [], []
    for pred, gt in pairs[:2]:
        a, b = se3.metrics._transform(pts, pred), se3.metrics._transform(pts, gt)
        assert max(np.abs(a).max(), np.abs(b).max()) <= 4.0
        d_add = np.linalg.norm(a - b, axis=1)
        d_adds, _ = spatial.cKDTree(a).query(b, k=1, workers=16)
        assert d_add.max() <= S and d_adds.max() <= S
        want_add.append(math.fsum(d_add.tolist()) / P)
        want_adds.append(math.fsum(d_adds.tolist()) / P)
        assert abs(want_add[-1] - se3.metrics.add(pred, gt, pts)) <= 1e-12            # the evaluators themselves, with numpy's mean
    mp = eng.model_points(pts)
    with Clock("pose_errors ADD + ADD-S P = 2^20, 3 pairs"):
        add_t, adds_t = eng.pose_errors(mp, torch.from_numpy(preds.reshape(3, 16)).cuda(), torch.from_numpy(gts.reshape(3, 16)).cuda())
        add, adds = add_t.cpu().numpy(), adds_t.cpu().numpy()
    d1, d2 = np.abs(add[:2] - want_add).max(), np.abs(adds[:2] - want_adds).max()
    print("[limits] P = 2^20: max |d add| = %.3e, max |d adds| = %.3e, bound %.3e" % (d1, d2, bound))
    assert d1 <= bound and d2 <= bound
    assert add[2] == 0.0 and adds[2] == 0.0 and not np.signbit(add[2]) and not np.signbit(adds[2])
    add_only, none = eng.pose_errors(mp, torch.from_numpy(preds.reshape(3, 16)).cuda(), torch.from_numpy(gts.reshape(3, 16)).cuda(), adds=False)
    assert none is None and np.array_equal(add_only.cpu().numpy(), add)
    mp.close()


def test_pose_errors_at_257_chunks(se3, eng):
    """se3tn_pose_errors, n = 65,537 pairs (257 chunks of 256, the last of one pair) at P = 64, slots from a pool of 8 pairs: every
    slot has the bits its pool member has when computed alone"""
    c = PL.ERRORS_N_CASE
    n, P = c["n_err"], c["P"]
    pts = err_cloud(P)
    rng = np.random.default_rng(8)
    pairs = [err_pair(rng, d) for d in (1e-6, 5e-3, 0.3, 1.0) * 2]
    preds, gts = np.array([p for p, _ in pairs]).reshape(8, 16), np.array([g for _, g in pairs]).reshape(8, 16)
    mp = eng.model_points(pts)
    alone = [eng.pose_errors(mp, preds[i:i + 1], gts[i:i + 1]) for i in range(8)]
    alone_add, alone_adds = np.array([a[0][0] for a in alone]), np.array([a[1][0] for a in alone])
    cpu = se3.metrics.pose_errors(preds, gts, pts, workers=1)
    assert np.abs(alone_add - cpu[0]).max() <= 1e-12 and np.abs(alone_adds - cpu[1]).max() <= 1e-12 and len(set(alone_adds.tolist())) == 8
    idx = PL.slot_assignment(n, 8, seed=257)
    check_slots(idx, 8)
    with Clock("pose_errors n = 65,537, P = 64"):
        idx_d = torch.from_numpy(idx).cuda()
        add_t, adds_t = eng.pose_errors(mp, torch.from_numpy(preds).cuda()[idx_d].contiguous(), torch.from_numpy(gts).cuda()[idx_d].contiguous())
        assert torch.equal(add_t, torch.from_numpy(alone_add).cuda()[idx_d]) and torch.equal(adds_t, torch.from_numpy(alone_adds).cuda()[idx_d])
    for s in host_slots(n, 257):
        assert float(add_t[s]) == alone_add[idx[s]] and float(adds_t[s]) == alone_adds[idx[s]], s
    mp.close()


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
FRAME_VALUES = np.array([1000, 1003, 900, 1100, 0, 2000, 995, 1006], np.uint16)      # m = 1000, tol 5: inlier x2, front, behind, unseen x2, inlier, behind


def frame_points(hw, elements):
    """the exact-boundary construction of test_exact_boundaries (identity rotation, z = 1, K = BOUNDARY_K: u = x + 0.5, v = y + 1.5
    exactly): the four frame edges +- 0.5 pixel and two points far beyond any integer (PC.boundary_points), then one point ON each of
    `elements` (flat indices into the frame)"""
    Hh, Ww = hw
    extra = [((e % Ww) - 0.5, (e // Ww) - 1.5, 1.0) for e in elements]
    return np.ascontiguousarray(np.concatenate([PC.boundary_points(hw), np.array(extra)]))


def hit_pixels(pts, hw):
    """(rows, cols) of the pixels the in-frame points land on under the identity"""
    Hh, Ww = hw
    uf, vf = np.rint(pts[:, 0] + 0.5), np.rint(pts[:, 1] + 1.5)
    ok = (uf >= 0) & (uf < Ww) & (vf >= 0) & (vf < Hh)
    q = np.unique(vf[ok].astype(np.int64) * Ww + uf[ok].astype(np.int64))          # (several boundary points share a pixel)
    return q // Ww, q % Ww


def run_frame_case(se3, eng, hw, elements, host):
    Hh, Ww = hw
    Kc = PC.BOUNDARY_K
    pts = frame_points(hw, elements)
    nrm = np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (len(pts), 1)))
    poses = PC.boundary_poses()
    rows, cols = hit_pixels(pts, hw)
    assert set((rows * Ww + cols).tolist()) >= set(elements)
    depth = np.zeros(hw, np.uint16)                      # untouched pages are never backed; the oracles read the projected pixels only
    depth_d = torch.zeros(hw, dtype=torch.int16, device="cuda")
    rows_d, cols_d = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
    mp = eng.model_points(pts, nrm)
    poses_d = torch.from_numpy(poses.reshape(3, 16)).cuda()
    rots, trans = np.eye(3)[None], np.ascontiguousarray(poses[:, :3, 3])
    prm = dict(gate_mm=20, iters=2, min_pairs=6, damping=1e-3, stop=0.0)
    seen_total, most_pairs = 0, 0
    for shift in range(len(FRAME_VALUES)):               # every hit pixel takes every value; its neighbours stay 0
        vals = FRAME_VALUES[(np.arange(len(rows)) + shift) % len(FRAME_VALUES)]
        depth[rows, cols] = vals
        depth_d[rows_d, cols_d] = torch.from_numpy(vals.view(np.int16)).cuda()
        want = PSO.score(pts, poses, depth, Kc, TOL)
        seen_total += int(want["seen_pts"][0])
        same_records(eng.score_poses(mp, poses_d, depth_d, Kc, TOL).cpu().numpy().view(PSO.DTYPE).reshape(3), want, ("score", hw, shift))
        want_g = PGO.score(pts, nrm, rots, trans, depth, Kc, TOL, 1)
        got_g = eng.score_pose_grid(mp, torch.from_numpy(rots.reshape(1, 9)).cuda(), torch.from_numpy(trans).cuda(), depth_d, Kc, TOL, facing=True)
        same_records(got_g.cpu().numpy().view(PSO.DTYPE).reshape(3), want_g, ("grid", hw, shift))
        want_a = PAO.align(pts, nrm, poses, depth, Kc, **prm)
        out, rec, sums = eng.align_poses(mp, poses_d, depth_d, Kc, sums=True, **prm)
        assert out.cpu().numpy().tobytes() == want_a[0].tobytes() and rec.cpu().numpy().tobytes() == want_a[1].tobytes(), ("align", hw, shift)
        assert np.array_equal(sums.cpu().numpy(), want_a[2])
        most_pairs = max(most_pairs, int(want_a[1]["pairs0"].max()))
        if host and shift == 0:
            idx, fit = eng.score_poses(mp, poses, depth, Kc, TOL, top=3)
            assert np.array_equal(idx, PSO.rank(want, 3))
            same_records(fit, want[idx], ("host", hw))
    n_valid = int(((FRAME_VALUES > 100) & (FRAME_VALUES < 2000)).sum())
    assert seen_total >= len(rows) * n_valid and most_pairs >= 6      # every hit pixel was seen under every valid value; the alignment solved
    mp.close()


def test_frame_of_2_25_pixels(se3, eng):
    """4,096 x 8,192 through se3tn_score_poses, se3tn_score_pose_grid, se3tn_align_poses and (once: it stages 64 MB)
    se3tn_search_poses_host: points on pixel (0, 0), on the last pixel, on elements 2^24 - 1, 2^24 and 2^24 + 1 and on the four frame
    edges +- 0.5 pixel"""
    hw = PL.FRAME_25
    n = hw[0] * hw[1]
    with Clock("frame 4,096 x 8,192"):
        run_frame_case(se3, eng, hw, [0, n - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 5 * 8192 + 77], host=True)


def test_frame_beyond_2_31_elements(se3, eng):
    """32,769 x 65,536 = 2^31 + 2^16 pixels, 4.3 GB, through the device-pointer entry points only (the _host entry points copy the
    frame into pinned staging and are not run at this size): points on elements 2^31 - 1, 2^31, 2^31 + 1 and on the last element --
    byte offsets around 2^32 -- each carrying its own depth.  The frame is zeros on the device with the hit pixels written in
    place; the oracle's frame is np.zeros, whose untouched pages are never backed.  tests/test_pose_family_limits_plan.py shows every
    index of the family in range at this size, which is the condition for running it."""
    hw = PL.FRAME_31
    n = hw[0] * hw[1]
    assert n > 2 ** 31 + 1
    with Clock("frame 32,769 x 65,536"):
        run_frame_case(se3, eng, hw, [0, n - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 24], host=False)
    torch.cuda.empty_cache()


# ---- outputs in mapped pinned host memory -------------------------------------------------------------------------------------------------
PAD = 64                                             # bytes behind every output that must keep the 0xEE they were filled with


def mapped_equals(m, want_bytes):
    torch.cuda.synchronize()
    got = m.read()
    n = len(want_bytes)
    assert got[:n].tobytes() == want_bytes, "mapped bytes differ from the device-memory result"
    assert (got[n:] == 0xEE).all() and len(got) == n + PAD


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_pose_outputs_in_mapped_pinned_memory(se3, eng, grid_pool):
    """se3tn_score_poses records, se3tn_rank_poses idx, se3tn_score_pose_grid records, se3tn_pose_errors add / adds: one call each
    into a block pre-filled with 0xEE; after a synchronise its bytes equal the device-memory result (held to the oracle here) and
    every byte past the output is still 0xEE"""
    g = grid_pool
    lib = eng.lib
    pts, nrm, depth = g["pts"][:257].copy(), g["nrm"][:257].copy(), g["depth"]
    pool = pose_pool()[:37]
    want = PSO.score(pts, pool, depth, K, TOL)
    mp = eng.model_points(pts, nrm)
    Kp = np.ascontiguousarray(K.reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
    poses_d, depth_d = torch.from_numpy(pool.reshape(37, 16)).cuda(), dev16(depth)
    fit = eng.score_poses(mp, poses_d, depth_d, K, TOL)
    same_records(fit.cpu().numpy().view(PSO.DTYPE).reshape(37), want, "device")
    m = Mapped(37 * 32 + PAD)
    try:
        assert lib.se3tn_score_poses(eng._h, mp._h, 37, C.c_void_p(poses_d.data_ptr()), C.c_void_p(depth_d.data_ptr()), H, W, Kp, TOL, m.d, stream()) == 0
        mapped_equals(m, fit.cpu().numpy().tobytes())
    finally:
        m.close()
    k = 8
    idx = rank_device(eng, want, k)
    assert np.array_equal(idx, PSO.rank(want, k))
    m = Mapped(4 * k + PAD)
    try:
        assert lib.se3tn_rank_poses(eng._h, 37, C.c_void_p(fit.data_ptr()), k, m.d, stream()) == 0
        mapped_equals(m, idx.tobytes())
    finally:
        m.close()
    rots, trans = g["rots"][:3], g["trans"][:13]                 # a ragged tile of 13 translations
    want_g = PGO.score(pts, nrm, rots, trans, depth, K, TOL, 1)
    rots_d, trans_d = torch.from_numpy(rots.reshape(3, 9).copy()).cuda(), torch.from_numpy(trans.copy()).cuda()
    fit_g = eng.score_pose_grid(mp, rots_d, trans_d, depth_d, K, TOL, facing=True)
    same_records(fit_g.cpu().numpy().view(PSO.DTYPE).reshape(39), want_g, "grid device")
    m = Mapped(39 * 32 + PAD)
    try:
        assert lib.se3tn_score_pose_grid(eng._h, mp._h, 3, C.c_void_p(rots_d.data_ptr()), 13, C.c_void_p(trans_d.data_ptr()),
                                         C.c_void_p(depth_d.data_ptr()), H, W, Kp, TOL, 1, m.d, stream()) == 0
        mapped_equals(m, fit_g.cpu().numpy().tobytes())
    finally:
        m.close()
    rng = np.random.default_rng(5)
    pairs = [err_pair(rng, d) for d in (1e-6, 5e-3, 0.3, 1.0, 0.3)]
    preds, gts = np.array([p for p, _ in pairs]).reshape(5, 16), np.array([q for _, q in pairs]).reshape(5, 16)
    ep = err_cloud(257)
    mpe = eng.model_points(ep)
    pred_d, gt_d = torch.from_numpy(preds).cuda(), torch.from_numpy(gts).cuda()
    add_t, adds_t = eng.pose_errors(mpe, pred_d, gt_d)
    cpu = se3.metrics.pose_errors(preds, gts, ep, workers=1)
    assert np.abs(add_t.cpu().numpy() - cpu[0]).max() <= 1e-12 and np.abs(adds_t.cpu().numpy() - cpu[1]).max() <= 1e-12
    ma, ms = Mapped(5 * 8 + PAD), Mapped(5 * 8 + PAD)
    try:
        assert lib.se3tn_pose_errors(eng._h, mpe._h, 5, C.c_void_p(pred_d.data_ptr()), C.c_void_p(gt_d.data_ptr()), ma.d, ms.d, stream()) == 0
        mapped_equals(ma, add_t.cpu().numpy().tobytes())
        mapped_equals(ms, adds_t.cpu().numpy().tobytes())
    finally:
        ma.close(); ms.close()
    mp.close(); mpe.close()


def crops(se3, group, rgb):
    arr = (se3._lib.Crop * len(group))()
    for i, c in enumerate(group):
        arr[i].rgb = c["rgb"].data_ptr() if rgb else None
        arr[i].depth = c["depth"].data_ptr()
        arr[i].H, arr[i].W = int(c["depth"].shape[0]), int(c["depth"].shape[1])
        arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = c["window"]
    return arr


def test_crop_records_in_mapped_pinned_memory(se3, eng):
    """se3tn_fit_stats records and both records of se3tn_color_stats, on the `identity` case of tests/color_fit_oracle.py"""
    case = CO.cases()["identity"]
    side = [dict(depth=dev16(c["depth"]), rgb=torch.from_numpy(np.array(c["rgb"])).cuda(), window=c["window"]) for c in case]
    want_fit, want_col = CO.as_arrays(se3, [CO.record(case[0], case[1], CO.TOL)])
    fit, col = eng.color_stats([side[0]], [side[1]], CO.TOL)
    assert np.array_equal(fit, want_fit) and np.array_equal(col, want_col)
    fit_only = eng.fit_stats([side[0]], [side[1]], CO.TOL)
    assert fit_only.tobytes() == fit.tobytes()
    m = Mapped(32 + PAD)
    try:
        assert eng.lib.se3tn_fit_stats(eng._h, crops(se3, [side[0]], False), crops(se3, [side[1]], False), 1, CO.TOL, m.d, stream()) == 0
        mapped_equals(m, fit.tobytes())
    finally:
        m.close()
    mf, mc = Mapped(32 + PAD), Mapped(80 + PAD)
    try:
        assert eng.lib.se3tn_color_stats(eng._h, crops(se3, [side[0]], True), crops(se3, [side[1]], True), 1, CO.TOL, mf.d, mc.d, stream()) == 0
        mapped_equals(mf, fit.tobytes())
        mapped_equals(mc, col.tobytes())
    finally:
        mf.close(); mc.close()
