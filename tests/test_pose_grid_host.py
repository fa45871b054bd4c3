"""CPU: the host side of the product-lattice pose search (se3tn_points_set_normals, se3tn_score_pose_grid,
se3tn_search_pose_grid_host; recover.lattice_factors / rotation_grid / depth_seeds; utils.voxel_down_sample_normals): the numpy
oracle the GPU tests hold the library to agrees with a plain per-point loop and, without the facing rule, with the oracle of
se3tn_score_poses on the composed poses; the factored lattice composes to pose_lattice bit for bit; the C ABI refuses bad arguments on
a host-only context, each with its own message; the tiling and staging (csrc/pose_grid_plan.h) hold in a stand-alone host program
under AddressSanitizer + UBSan; and on a synthetic scene the facing rule finds the object where the plain count does not -- the
reason the rule exists.  The device results are held to the oracle in tests/test_gpu_pose_grid.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pose_grid_oracle as PGO
import pose_grid_scene as SC
import pose_search_oracle as PSO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def small_case():
    """3 rotations x 5 translations x 40 points with normals on a 24 x 32 frame of valid, invalid and borderline depths; translation 3
    lies behind the camera, translation 4 carries a NaN, rotation 2 carries one"""
    rng = np.random.default_rng(0)
    H, W = 24, 32
    K = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1.0]])
    depth = rng.integers(480, 520, (H, W)).astype(np.uint16)
    mask = rng.random((H, W)) < 0.2
    depth[mask] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    pts = rng.uniform(-0.05, 0.05, (40, 3))
    nrm = pts / np.linalg.norm(pts, axis=1)[:, None]          # a convex blob: the normal of a point is its direction from the centre
    nrm[5] = 0.0                                              # a zero normal never faces
    rots = np.array([Rotation.from_rotvec(v).as_matrix() for v in ((0.2, -0.1, 0.3), (1.0, 2.0, -0.5), (0.0, 0.4, 0.0))])
    rots[2, 1, 1] = np.nan
    trans = np.array([(0.0, 0.0, 0.5), (0.01, -0.02, 0.45), (0.26, 0.0, 0.5), (0.0, 0.0, -0.5), (0.0, np.nan, 0.5)])
    return pts, nrm, rots, trans, depth, K


def test_vectorised_oracle_equals_the_loop_and_the_pose_search_oracle():
    pts, nrm, rots, trans, depth, K = small_case()
    for tol in (1, 5, 30):
        for facing in (0, 1):
            vec = PGO.score(pts, nrm, rots, trans, depth, K, tol, facing, chunk=2)
            assert np.array_equal(vec, PGO.score(pts, nrm, rots, trans, depth, K, tol, facing))            # any chunking
            assert np.array_equal(vec, PGO.score_loop(pts, nrm, rots, trans, depth, K, tol, facing)), (tol, facing)
            PGO.check_invariants(vec, 40, tol, facing)
        plain = PGO.score(pts, None, rots, trans, depth, K, tol, 0)
        assert np.array_equal(plain, PSO.score(pts, PGO.compose(rots, trans), depth, K, tol)), tol
    f1, f0 = (PGO.score(pts, nrm, rots, trans, depth, K, 30, fc) for fc in (1, 0))
    # the cases show what they are meant to show: a convex blob in front of the camera shows about half its points, none of them hidden
    assert 10 <= f1["points"][0] <= 30 and f1["inlier_pts"][0] > 0 and f0["points"][0] == 40
    assert f1["front_pts"][0] < f0["front_pts"][0]
    assert (f1["in_frame_pts"][3::5] == 0).all() and (f1["in_frame_pts"][4::5] == 0).all() and (f1["in_frame_pts"][10:] == 0).all()
    assert (f1["points"][4::5] == 0).all() and (f1["points"][10:] == 0).all()       # f is NaN: nothing faces


def test_symbols_follow_the_header(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("se3tn_points_set_normals", "se3tn_points_has_normals", "se3tn_score_pose_grid", "se3tn_search_pose_grid_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.exported_symbols(), name
    assert "f < 0" in hdr and "r * n_trans + t" in hdr


def test_lattice_factors_compose_to_pose_lattice_bit_for_bit(se3):
    base = np.eye(4)
    base[:3, :3] = Rotation.from_rotvec([0.3, -0.2, 0.5]).as_matrix()
    base[:3, 3] = [0.02, -0.01, 0.6]
    for steps in (0, 1, 5):
        for rot in ((15.0,), (10.0, 25.0)):
            rots, trans = se3.recover.lattice_factors(base, steps * 0.01, 0.01, rot)
            assert rots.shape == (1 + 6 * len(rot), 3, 3) and trans.shape == ((2 * steps + 1) ** 3, 3)
            want = se3.pose_lattice(base, steps * 0.01, 0.01, rot)
            assert np.array_equal(PGO.compose(rots, trans), want), (steps, rot)
            assert np.array_equal(want, PSO.lattice(base, steps, 0.01, rot))
    assert [len(x) for x in se3.recover.lattice_factors(base)] == [7, 1331]
    with pytest.raises(ValueError):
        se3.recover.lattice_factors(base, 0.05, 0.0)


def test_rotation_grid_count_orthogonality_determinism_and_spacing(se3):
    for views, inplane in ((40, 6), (40, 12), (1, 1), (7, 3)):
        G = se3.recover.rotation_grid(views, inplane)
        assert G.shape == (views * inplane, 3, 3) and G.dtype == np.float64
        assert np.abs(G @ G.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-15
        assert np.abs(np.linalg.det(G) - 1.0).max() <= 1e-15
        assert np.array_equal(G, se3.recover.rotation_grid(views, inplane))
        # the stated order: in-plane turns innermost, each a turn about the optical axis of the view's first rotation
        for p in range(inplane):
            a = 2 * np.pi * p / inplane
            Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
            assert np.allclose(G[p::inplane], Rz @ G[0::inplane], atol=1e-15)
        # the view direction of view v points at the camera
        z = 1.0 - (2.0 * np.arange(views) + 1.0) / views
        assert np.allclose(-G[0::inplane, 2, 2], z, atol=1e-15)
        if len(G) > 1:
            cos = (np.einsum("aij,bij->ab", G, G) - 1.0) / 2.0                    # trace(Ra^T Rb)
            ang = np.arccos(np.clip(cos, -1.0, 1.0))
            ang[np.eye(len(G), dtype=bool)] = np.inf
            nominal = min(np.sqrt(4 * np.pi / views), 2 * np.pi / inplane) if inplane > 1 else np.sqrt(4 * np.pi / views)
            assert ang.min() >= 0.5 * nominal, (views, inplane, ang.min(), nominal)
    with pytest.raises(ValueError):
        se3.recover.rotation_grid(0, 4)


def test_depth_seeds_equal_a_per_pixel_loop(se3):
    rng = np.random.default_rng(3)
    H, W = 37, 53
    K = np.array([[61.5, 0, 25.25], [0, 60.75, 18.5], [0, 0, 1.0]])
    depth = rng.integers(90, 2100, (H, W)).astype(np.uint16)
    depth[::3, ::4] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), depth[::3, ::4].shape)

    def loop(stride, behind, roi):
        left, top, right, bottom = (0, 0, W, H) if roi is None else roi
        out = []
        for v in range(max(top, 0), min(bottom, H), stride):
            for u in range(max(left, 0), min(right, W), stride):
                d = np.float64(depth[v, u])
                if d > 100 and d < 2000:
                    z = d / 1000.0 + behind
                    out.append(((u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z))
        return np.array(out, np.float64).reshape(-1, 3)

    for stride, behind, roi in ((1, 0.0, None), (3, 0.03, None), (4, 0.05, (5, 7, 40, 30)), (8, 0.03, (-4, -2, 99, 99)), (5, 0.01, (10, 10, 11, 11))):
        got = se3.recover.depth_seeds(depth, K, stride, behind, roi)
        assert got.dtype == np.float64 and np.array_equal(got, loop(stride, behind, roi)), (stride, roi)
    assert 0 < len(se3.recover.depth_seeds(depth, K, 1, 0.0)) < H * W                # the validity rule dropped some
    assert se3.recover.depth_seeds(depth, K, 4, 0.0, (20, 20, 20, 30)).shape == (0, 3)   # an empty region
    assert se3.recover.depth_seeds(np.zeros((H, W), np.uint16), K, 4, 0.0).shape == (0, 3)


def test_voxel_down_sample_normals_keeps_the_points(se3):
    U = se3.utils
    rng = np.random.default_rng(4)
    pts = rng.uniform(-0.04, 0.04, (3000, 3))
    nrm = rng.normal(size=(3000, 3))
    for voxel in (0.005, 0.013):
        p, n = U.voxel_down_sample_normals(pts, nrm, voxel)
        want = U.voxel_down_sample(pts, voxel)
        assert p.dtype == np.float64 and p.tobytes() == want.tobytes() and n.shape == p.shape
        # the mean normal of each voxel, by a loop over the voxels
        origin = pts.min(0) - voxel * 0.5
        idx = np.floor((pts - origin) / voxel).astype(np.int64)
        uniq, inv = np.unique(idx, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for j in (0, 1, len(uniq) // 2, len(uniq) - 1):
            assert np.allclose(n[j], nrm[inv == j].mean(0), atol=1e-15)
    one = U.voxel_down_sample_normals(pts[:1], nrm[:1], 0.005)
    assert np.array_equal(one[0], pts[:1]) and np.array_equal(one[1], nrm[:1])
    with pytest.raises(ValueError):
        U.voxel_down_sample_normals(pts, nrm[:10], 0.005)


def test_refusals_on_a_host_only_context_each_with_its_message(se3):
    """Every NULL pointer, the counts, the tolerance, the frame size and the facing switch are refused with SE3TN_E_ARG and a message of
    their own BEFORE the context is found to have no device -- and the points handle is not read before that (a fake one stands in)."""
    L = se3._lib
    lib = L.load()
    eng = se3.Engine(-1, 1)
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    Kp = buf.ctypes.data_as(C.POINTER(C.c_double))
    fake = p
    good = dict(n_rot=3, n_trans=5, H=4, W=4, tol=5, facing=0, k=2)

    def score(ctx=eng._h, pts=fake, rots=p, trans=p, depth=p, Kq=Kp, fit=p, **kw):
        g = dict(good, **kw)
        return lib.se3tn_score_pose_grid(ctx, pts, g["n_rot"], rots, g["n_trans"], trans, depth, g["H"], g["W"], Kq, g["tol"], g["facing"], fit, None)

    def search(ctx=eng._h, pts=fake, rots=p, trans=p, depth=p, Kq=Kp, idx=p, fit=p, **kw):
        g = dict(good, **kw)
        return lib.se3tn_search_pose_grid_host(ctx, pts, g["n_rot"], rots, g["n_trans"], trans, depth, g["H"], g["W"], Kq, g["tol"],
                                               g["facing"], g["k"], idx, fit, None)

    for call in (score, search):
        assert call() == -1 and b"host-only" in lib.se3tn_last_error()           # good numbers: the context is what is wrong
        ptrs = ("ctx", "pts", "rots", "trans", "depth", "Kq", "fit") + (("idx",) if call is search else ())
        for name in ptrs:
            assert call(**{name: None}) == -1 and b"NULL" in lib.se3tn_last_error(), name
        for kw in (dict(n_rot=0), dict(n_trans=0), dict(n_rot=-2), dict(n_trans=-1), dict(n_rot=1025, n_trans=1024),
                   dict(n_rot=2 ** 20, n_trans=2), dict(n_rot=2 ** 30, n_trans=2 ** 30)):
            assert call(**kw) == -1 and b"SE3TN_POSE_SEARCH_MAX_POSES" in lib.se3tn_last_error(), kw
        assert call(n_rot=1024, n_trans=1024) == -1 and b"host-only" in lib.se3tn_last_error()   # 2^20 itself is allowed
        for tol in (0, -5, 65536):
            assert call(tol=tol) == -1 and b"tol_mm" in lib.se3tn_last_error(), tol
        for kw in (dict(H=0), dict(W=-1)):
            assert call(**kw) == -1 and b"empty frame" in lib.se3tn_last_error(), kw
        for fc in (2, -1):
            assert call(facing=fc) == -1 and b"facing" in lib.se3tn_last_error(), fc
    # the normals: a NULL handle (a real one needs a device: non-finite components are refused in tests/test_gpu_pose_grid.py)
    assert lib.se3tn_points_set_normals(None, p) == -1 and b"NULL" in lib.se3tn_last_error()
    assert lib.se3tn_points_set_normals(None, None) == -1 and lib.se3tn_points_has_normals(None) == -1
    with pytest.raises(L.Se3tnError):
        eng.score_pose_grid(np.zeros((4, 3)), np.eye(3)[None], np.zeros((1, 3)), np.zeros((4, 4), np.uint16), np.eye(3), 5)   # no handle
    eng.close()


def test_pose_grid_plan_tiling_and_staging_under_sanitizers(tmp_path):
    """csrc/pose_grid_plan.h in a stand-alone host program built with AddressSanitizer + UBSan: over P in {1, 63, 64, 65, 1023, 1024,
    1025, 2049} x n_trans in {1, TT - 1, TT, TT + 1, 3 TT + 5} x n_rot in {1, 3} every (rotation, translation, point) triple is visited
    exactly once through LDS buffers of exactly the planned bytes, and the staging regions are ordered, aligned and walked."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pose_grid_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pose_grid_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "pose_grid_plan_check: ok" in out.stdout


def test_the_facing_rule_finds_the_object_where_the_plain_count_does_not(se3):
    """pose_grid_scene: the 30 mm thick L (304 points with analytic normals) flat on the tilted table beside the clutter box, 120 x 160,
    5 % holes, tolerance 10 mm.  Stage 1 of the search on the ORACLE alone: rotation_grid(40, 6) x depth_seeds(stride 8, 30 mm behind)
    = 240 x 281 = 67,440 candidates.  The bound is one seed spacing at the winning seed's depth (8 px * z / fx, about 16 mm) plus
    10 mm.  Measured here:
      facing:  the best candidate (97 inliers of 152 facing points) lies 12.1 mm from the true translation, the four best within 25.0 mm;
      plain:   the best candidate (130 inliers of 304) lies 74.7 mm away, half a turn from the truth, sunk into the table with 136 points
               seen through; the candidate the facing rule prefers comes third.
    The plain count rewards the hidden lower face for lying near ANY surface; counting only what the camera could see does not."""
    pts, nrm = SC.l_model()
    depth = SC.frame(0)
    G = SC.true_pose()
    assert 280 <= len(pts) <= 320 and depth.shape == SC.HW
    rots = se3.recover.rotation_grid(40, 6)
    seeds = se3.recover.depth_seeds(depth, SC.K, 8, 0.03)
    assert len(rots) == 240 and 250 <= len(seeds) <= 300
    at_truth = PGO.score(pts, nrm, G[None, :3, :3], G[None, :3, 3], depth, SC.K, SC.TOL, 1)[0]
    assert at_truth["inlier_pts"] >= 0.9 * at_truth["points"] and at_truth["points"] == len(pts) // 2     # the visible half, confirmed
    dist = {}
    for facing in (1, 0):
        fit = PGO.score(pts, nrm, rots, seeds, depth, SC.K, SC.TOL, facing)
        PGO.check_invariants(fit, len(pts), SC.TOL, facing)
        best = int(PSO.rank(fit, 1)[0])
        seed = seeds[best % len(seeds)]
        dist[facing] = (np.linalg.norm(seed - G[:3, 3]), 8 * seed[2] / SC.K[0, 0] + 0.010)
        print("facing = %d: best candidate %d %s, %.1f mm from the truth (bound %.1f mm)" % (facing, best, fit[best], 1000 * dist[facing][0],
                                                                                            1000 * dist[facing][1]))
    assert dist[1][0] <= dist[1][1]
    assert not dist[0][0] <= dist[0][1]
