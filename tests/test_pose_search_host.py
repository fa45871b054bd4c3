"""CPU: the host side of the pose search (se3tn_score_poses, se3tn_rank_poses, se3tn_search_poses_host; recover.pose_lattice): the
numpy oracle the GPU tests hold the library to agrees with a plain per-point loop of the rule, the C ABI exports the new symbols with
the header's constants and refuses a host-only context and NULL pointers before it looks at anything else, the candidate lattice has
the stated count and order, and the rank key and staging layout (csrc/pose_search_plan.h) hold in a stand-alone host program under
AddressSanitizer + UBSan.  The device results are held to the oracle in tests/test_gpu_pose_search.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pose_search_oracle as PSO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def test_vectorised_oracle_equals_the_per_point_loop():
    """5 poses x 40 points on a 24 x 32 frame whose depth holds valid, invalid and borderline values: a pose in front of the surface, one
    on it, one off the frame edge, one behind the camera, one with a NaN entry."""
    rng = np.random.default_rng(0)
    H, W = 24, 32
    K = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1.0]])
    depth = rng.integers(480, 520, (H, W)).astype(np.uint16)
    mask = rng.random((H, W)) < 0.2
    depth[mask] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    depth[::5, ::3] = 0
    depth[1::7, 2::4] = 2000
    pts = rng.uniform(-0.05, 0.05, (40, 3))
    poses = np.tile(np.eye(4), (5, 1, 1))
    for i, (rv, t) in enumerate((((0.2, -0.1, 0.3), (0.0, 0.0, 0.5)), ((1.0, 2.0, -0.5), (0.01, -0.02, 0.45)),
                                 ((0, 0, 0), (0.26, 0.0, 0.5)), ((0.3, 0, 0), (0, 0, -0.5)), ((0, 0, 0), (0, 0, 0.5)))):
        poses[i, :3, :3] = Rotation.from_rotvec(rv).as_matrix()
        poses[i, :3, 3] = t
    poses[4, 0, 1] = np.nan
    for tol in (1, 5, 30):
        vec, loop = PSO.score(pts, poses, depth, K, tol), PSO.score_loop(pts, poses, depth, K, tol)
        assert np.array_equal(vec, loop), (tol, vec, loop)
        PSO.check_invariants(vec, 40, tol)
    f = PSO.score(pts, poses, depth, K, 30)
    # the cases show what they are meant to show
    assert f["inlier_pts"][0] > 0 and f["seen_pts"][0] < f["in_frame_pts"][0] == 40
    assert 0 < f["in_frame_pts"][2] < 40 and f["in_frame_pts"][3] == 0 and f["in_frame_pts"][4] == 0
    # the rank oracle sorts by the tuple; the key orders the same way
    ks = PSO.keys(f)
    assert list(PSO.rank(f, 5)) == sorted(range(5), key=lambda i: -ks[i])


def test_symbols_constants_and_the_record_follow_the_header(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("se3tn_score_poses", "se3tn_rank_poses", "se3tn_search_poses_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.exported_symbols(), name
    assert int(re.search(r"#define SE3TN_POSE_SEARCH_MAX_POSES (\d+)", hdr).group(1)) == L.POSE_SEARCH_MAX_POSES == 2 ** 20
    assert int(re.search(r"#define SE3TN_POSE_RANK_MAX (\d+)", hdr).group(1)) == L.POSE_RANK_MAX == 64
    body = re.search(r"typedef struct se3tn_point_fit \{(.*?)\} se3tn_point_fit;", hdr, re.S).group(1)
    assert tuple(re.findall(r"uint32_t (\w+);", body)) == L.POINT_FIT_FIELDS + ("_reserved",) == PSO.FIELDS
    assert L.POINT_FIT_DTYPE == PSO.DTYPE and L.POINT_FIT_DTYPE.itemsize == C.sizeof(L.PointFit) == 32
    assert "predict.py:539-541" in hdr   # the reference's counterpart
    # the Python key is the oracle's
    rec = np.zeros(4, L.POINT_FIT_DTYPE)
    rec["inlier_pts"] = [0, 107, 107, 2 ** 20]
    rec["behind_pts"] = [0, 5, 2 ** 21, 0]
    assert list(se3.recover.pose_key(rec)) == PSO.keys(rec)
    assert list(se3.recover.pose_key(rec, [2 ** 20 - 1, 0, 7, 1])) == [PSO.key(r["inlier_pts"], r["behind_pts"], i)
                                                                      for r, i in zip(rec, [2 ** 20 - 1, 0, 7, 1])]


def test_host_only_context_and_null_arguments_are_refused_first(se3):
    """A host-only context and every NULL pointer: SE3TN_E_ARG before n, k, tol or the frame size are looked at (they are nonsense here)."""
    L = se3._lib
    lib = L.load()
    eng = se3.Engine(-1, 1)
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    K = buf.ctypes.data_as(C.POINTER(C.c_double))
    fake = p          # stands for a points handle: never dereferenced, the context is refused first
    bad = dict(n=-7, H=0, W=-1, tol=0, k=999)
    assert lib.se3tn_score_poses(eng._h, fake, bad["n"], p, p, bad["H"], bad["W"], K, bad["tol"], p, None) == -1
    assert b"host-only" in lib.se3tn_last_error()
    assert lib.se3tn_rank_poses(eng._h, bad["n"], p, bad["k"], p, None) == -1
    assert b"host-only" in lib.se3tn_last_error()
    assert lib.se3tn_search_poses_host(eng._h, fake, bad["n"], p, p, bad["H"], bad["W"], K, bad["tol"], bad["k"], p, p, None) == -1
    assert b"host-only" in lib.se3tn_last_error()
    # every pointer in turn (a NULL context included)
    score = [eng._h, fake, bad["n"], p, p, bad["H"], bad["W"], K, bad["tol"], p, None]
    for i in (0, 1, 3, 4, 7, 9):
        a = list(score)
        a[i] = None
        assert lib.se3tn_score_poses(*a) == -1 and b"NULL" in lib.se3tn_last_error(), i
    rank = [eng._h, bad["n"], p, bad["k"], p, None]
    for i in (0, 2, 4):
        a = list(rank)
        a[i] = None
        assert lib.se3tn_rank_poses(*a) == -1 and b"NULL" in lib.se3tn_last_error(), i
    search = [eng._h, fake, bad["n"], p, p, bad["H"], bad["W"], K, bad["tol"], bad["k"], p, p, None]
    for i in (0, 1, 3, 4, 7, 10, 11):
        a = list(search)
        a[i] = None
        assert lib.se3tn_search_poses_host(*a) == -1 and b"NULL" in lib.se3tn_last_error(), i
    with pytest.raises(L.Se3tnError):
        eng.score_poses(np.zeros((4, 3)), np.eye(4)[None], np.zeros((4, 4), np.uint16), np.eye(3), 5)   # an array is not a handle
    eng.close()


def test_pose_lattice_count_order_and_determinism(se3):
    base = np.eye(4)
    base[:3, :3] = Rotation.from_rotvec([0.3, -0.2, 0.5]).as_matrix()
    base[:3, 3] = [0.02, -0.01, 0.6]
    for radius, step, rot in ((0.05, 0.01, (15.0,)), (0.02, 0.01, (10.0, 25.0)), (0.03, 0.015, ()), (0.0, 0.01, (5.0,))):
        L = se3.pose_lattice(base, radius, step, rot)
        r = int(round(radius / step))
        m = (2 * r + 1) ** 3
        assert L.shape == (m * (1 + 6 * len(rot)), 4, 4) and L.dtype == np.float64
        assert np.array_equal(L, PSO.lattice(base, r, step, rot))                                  # the order, bit for bit
        assert np.array_equal(L, se3.pose_lattice(base, radius, step, rot))                        # two calls: equal bits
        assert np.array_equal(L[(r * (2 * r + 1) + r) * (2 * r + 1) + r], base)                    # the base pose, where the order puts it
        assert np.array_equal(L[:, 3, :], np.tile([0, 0, 0, 1.0], (len(L), 1)))
        # identity block first: the rotation of the first m candidates is the base's; translations x outermost, z innermost, ascending
        assert (L[:m, :3, :3] == base[:3, :3]).all()
        d = L[:m, :3, 3] - base[:3, 3]
        if r:
            assert np.allclose(d[0], [-r * step] * 3) and np.allclose(d[1] - d[0], [0, 0, step]) and np.allclose(d[2 * r + 1] - d[0], [0, step, 0])
            assert np.allclose(d[(2 * r + 1) ** 2] - d[0], [step, 0, 0])
        # then +a, -a about camera x, y, z for each angle
        for q in range(6 * len(rot)):
            a, axis, sign = rot[q // 6], (q % 6) // 2, 1 - 2 * (q % 2)
            rv = np.zeros(3)
            rv[axis] = np.deg2rad(sign * a)
            blk = L[(1 + q) * m:(2 + q) * m]
            assert np.allclose(blk[0, :3, :3], Rotation.from_rotvec(rv).as_matrix() @ base[:3, :3], atol=1e-15)
            assert np.array_equal(blk[:, :3, 3], L[:m, :3, 3])
    assert len(se3.pose_lattice(base)) == 9317   # the defaults: +-50 mm in 10 mm steps, identity and +-15 degrees about each axis


def test_pose_search_plan_key_and_staging_under_sanitizers(tmp_path):
    """csrc/pose_search_plan.h (the rank key and its inverse, the staging layout of se3tn_search_poses_host) in a stand-alone host
    program built with AddressSanitizer + UBSan: key order against tuple order over the edge values, and every staging region walked
    over buffers malloc'ed with exactly the planned bytes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pose_search_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pose_search_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "pose_search_plan_check: ok" in out.stdout
