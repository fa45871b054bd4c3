"""CPU: the host side of the scene-aware lattice search (se3tn_score_pose_grid_scene, se3tn_search_pose_grid_scene_host): the numpy
oracle the GPU tests hold the library to (tests/scene_search_oracle.py) agrees with a plain per-point loop and, with an all-zero scene,
with the oracle of se3tn_score_pose_grid word for word; the header states the rule and the symbols are exported and bound; the C ABI
refuses bad arguments on a host-only context, each with its own message; count_point_scene (csrc/pose_point_rule.h) and the LDS and
staging arithmetic (csrc/pose_grid_plan.h) hold in a stand-alone host program under AddressSanitizer + UBSan; and on the scene of
tests/scene_search_scene.py the plain facing search lays the lost slab onto its tracked neighbour where the scene-aware rule finds
it -- the reason the rule exists.  The device results are held to the oracle in tests/test_gpu_scene_search.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pose_grid_oracle as PGO
import pose_search_oracle as PSO
import scene_search_oracle as SSO
import scene_search_scene as SS
from test_pose_grid_host import small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = SS.BOUNDARY


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def small_scene(tol):
    """the boundary scene frame of small_case() for tolerance `tol` (scene_search_scene.boundary_scene)"""
    return SS.boundary_scene(small_case(), tol)


def test_vectorised_oracle_equals_the_loop_and_the_plain_oracle():
    pts, nrm, rots, trans, depth, K = small_case()
    zero = np.zeros_like(depth)
    for tol in (1, 5, 30):
        scene, marks = small_scene(tol)
        assert set(BOUNDARY) <= set(np.unique(scene).tolist())
        for facing in (0, 1):
            vec = SSO.score(pts, nrm, rots, trans, depth, scene, K, tol, facing, chunk=2)
            assert np.array_equal(vec, SSO.score(pts, nrm, rots, trans, depth, scene, K, tol, facing))       # any chunking
            assert np.array_equal(vec, SSO.score_loop(pts, nrm, rots, trans, depth, scene, K, tol, facing)), (tol, facing)
            SSO.check_invariants(vec, 40, tol, facing)
            # an all-zero scene: every word is the plain rule's (hidden_pts = 0 = _reserved)
            plain = PGO.score(pts, nrm, rots, trans, depth, K, tol, facing)
            none = SSO.score(pts, nrm, rots, trans, depth, zero, K, tol, facing)
            assert none.tobytes() == plain.tobytes(), (tol, facing)
            assert np.array_equal(SSO.rank(vec, 5), PSO.rank(vec.view(PSO.DTYPE), 5))
        # the edge of `hidden`, on candidate 0 without the facing rule: s == m + tol hides the point, s == m + tol + 1 does not
        (p_eq, m_eq), (p_gt, m_gt) = marks
        assert scene[p_eq] == m_eq + tol and scene[p_gt] == m_gt + tol + 1
        base = SSO.score(pts, None, rots[:1], trans[:1], depth, scene, K, tol, 0)[0]
        for at, moved in ((p_eq, -1), (p_gt, +1)):
            other = scene.copy()
            other[at] = int(scene[at]) + (1 if at == p_eq else -1)                # across the edge: the point changes sides
            rec = SSO.score(pts, None, rots[:1], trans[:1], depth, other, K, tol, 0)[0]
            assert int(rec["hidden_pts"]) == int(base["hidden_pts"]) + moved, (tol, at)
    vec = SSO.score(pts, nrm, rots, trans, depth, small_scene(5)[0], K, 5, 0)
    assert vec["hidden_pts"].max() > 0 and (vec["seen_pts"] > 0).any()            # the case shows both verdicts
    assert (vec["hidden_pts"][3::5] == 0).all() and (vec["hidden_pts"][10:] == 0).all()   # behind the camera / NaN: nothing is in frame


def test_the_header_states_the_rule_and_the_symbols_are_bound(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    rule = open(os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc", "pose_point_rule.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("se3tn_score_pose_grid_scene", "se3tn_search_pose_grid_scene_host", "se3tn_last_search_scene"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.exported_symbols(), name
    flat = " ".join(hdr.split())
    for text in ("s = scene[vf, uf]", "100 < s < 2000 && s <= m + tol_mm", "hidden + seen <= in_frame <= points",
                 "seen = inlier + front + behind", "(const se3tn_point_fit*)fit_dev", "NOTHING else past in_frame_pts"):
        assert text in flat, text
    assert re.search(r"typedef struct se3tn_scene_point_fit \{.{0,800}?uint32_t hidden_pts;.{0,200}?\} se3tn_scene_point_fit;", hdr, re.S)
    assert "count_point_scene" in rule and "s <= m + tol" in rule
    assert L.SCENE_POINT_FIT_DTYPE.names == L.POINT_FIT_DTYPE.names[:7] + ("hidden_pts",) and L.SCENE_POINT_FIT_DTYPE.itemsize == 32
    # recover.pose_key reads both record types alike
    a = np.zeros(3, L.SCENE_POINT_FIT_DTYPE)
    a["inlier_pts"], a["behind_pts"], a["hidden_pts"] = (5, 7, 7), (1, 2, 0), (9, 9, 9)
    assert list(se3.recover.pose_key(a)) == list(se3.recover.pose_key(a.view(L.POINT_FIT_DTYPE)))
    assert int(np.argmax(se3.recover.pose_key(a))) == 2


def test_refusals_on_a_host_only_context_each_with_its_message(se3):
    """Every NULL pointer, the counts, the tolerance, the frame, the facing switch, k, and for the one-call entry the occluders (their
    number, meshes, widths, poses, the camera, the frame limits of the scene stage) are refused with SE3TN_E_ARG and a message of
    their own BEFORE the context is found to have no device; fake handles stand in and are never read."""
    L = se3._lib
    lib = L.load()
    eng = se3.Engine(-1, 4)
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    Kh = np.ascontiguousarray(SS.K.reshape(9))
    Kp = Kh.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(n_rot=3, n_trans=5, H=120, W=160, tol=5, facing=0, k=2, n_occ=2)

    def objects(n, mesh=buf.ctypes.data, width=150.0):
        return (L.Object * max(n, 1))(*[L.Object(None, mesh, width) for _ in range(max(n, 1))])

    poses = np.tile(np.eye(4), (4, 1, 1))
    poses[:, 2, 3] = 0.5
    posep = C.c_void_p(poses.ctypes.data)

    def score(ctx=eng._h, pts=p, rots=p, trans=p, depth=p, scene=p, Kq=Kp, fit=p, **kw):
        g = dict(good, **kw)
        return lib.se3tn_score_pose_grid_scene(ctx, pts, g["n_rot"], rots, g["n_trans"], trans, depth, scene, g["H"], g["W"], Kq, g["tol"],
                                               g["facing"], fit, None)

    def search(ctx=eng._h, pts=p, rots=p, trans=p, depth=p, Kq=Kp, idx=p, fit=p, occ=None, occ_poses=posep, occ_fit=p, **kw):
        g = dict(good, **kw)
        occ = objects(g["n_occ"]) if occ is None else occ
        return lib.se3tn_search_pose_grid_scene_host(ctx, pts, g["n_rot"], rots, g["n_trans"], trans, depth, g["H"], g["W"], Kq, g["tol"],
                                                     g["facing"], g["k"], g["n_occ"], occ, occ_poses, idx, fit, occ_fit, None)

    for call in (score, search):
        assert call() == -1 and b"host-only" in lib.se3tn_last_error()           # good numbers: the context is what is wrong
        ptrs = ("ctx", "pts", "rots", "trans", "depth", "Kq", "fit") + (("scene",) if call is score else ("idx", "occ_poses"))
        for name in ptrs:
            assert call(**{name: None}) == -1 and b"NULL" in lib.se3tn_last_error(), name
        for kw in (dict(n_rot=0), dict(n_trans=0), dict(n_rot=-2), dict(n_rot=1025, n_trans=1024), dict(n_rot=2 ** 30, n_trans=2 ** 30)):
            assert call(**kw) == -1 and b"SE3TN_POSE_SEARCH_MAX_POSES" in lib.se3tn_last_error(), kw
        for tol in (0, -5, 65536):
            assert call(tol=tol) == -1 and b"tol_mm" in lib.se3tn_last_error(), tol
        for kw in (dict(H=0), dict(W=-1)):
            assert call(**kw) == -1 and b"empty frame" in lib.se3tn_last_error(), kw
        for fc in (2, -1):
            assert call(facing=fc) == -1 and b"facing" in lib.se3tn_last_error(), fc
    # the one-call entry alone: the ranking and the occluders
    null_occ = C.cast(None, C.POINTER(L.Object))
    assert search(occ=null_occ) == -1 and b"NULL" in lib.se3tn_last_error()
    assert search(occ_fit=None) == -1 and b"host-only" in lib.se3tn_last_error()  # the occluders' records are optional
    for k in (0, 16, 65):
        assert search(k=k) == -1 and b"k = " in lib.se3tn_last_error(), k
    for n_occ in (0, -1, 5, 33):                                                  # the context holds 4
        assert search(n_occ=n_occ) == -1 and b"SE3TN_SCENE_MAX_OBJECTS" in lib.se3tn_last_error(), n_occ
    assert search(n_occ=4) == -1 and b"host-only" in lib.se3tn_last_error()
    assert search(H=2049, W=8) == -1 and b"2048 rows" in lib.se3tn_last_error()
    assert search(H=2048, W=1025) == -1 and b"2^21" in lib.se3tn_last_error()
    assert search(occ=objects(2, mesh=None)) == -1 and b"has no mesh" in lib.se3tn_last_error()
    assert search(occ=objects(2, width=0.0)) == -1 and b"object_width_mm" in lib.se3tn_last_error()
    for bad, word in ((-0.5, b"not in front"), (np.nan, b"not finite")):
        q = poses.copy()
        q[1, 2, 3] = bad
        assert search(occ_poses=C.c_void_p(q.ctypes.data)) == -1 and word in lib.se3tn_last_error(), bad
    Kbad = Kh.copy()
    Kbad[4] = np.inf
    assert search(Kq=Kbad.ctypes.data_as(C.POINTER(C.c_double))) == -1 and b"K entry 4" in lib.se3tn_last_error()
    # no scene has been composed on this context
    ptr, h, w = C.c_void_p(), C.c_int(), C.c_int()
    assert lib.se3tn_last_search_scene(eng._h, C.byref(ptr), C.byref(h), C.byref(w)) == -2 and b"no scene frame" in lib.se3tn_last_error()
    assert lib.se3tn_last_search_scene(None, C.byref(ptr), C.byref(h), C.byref(w)) == -1 and b"NULL" in lib.se3tn_last_error()
    with pytest.raises(L.Se3tnError):
        eng.search_pose_grid_scene(np.zeros((4, 3)), np.eye(3)[None], np.zeros((1, 3)), np.zeros((4, 4), np.uint16), np.eye(3), [], [])
    eng.close()


def test_the_rule_and_the_plan_under_sanitizers(tmp_path):
    """tests/c_abi/scene_search_check.cpp built with AddressSanitizer + UBSan and run as a program: the seven-word rows lie behind the
    planes in an LDS buffer of exactly the planned bytes, six / three workgroups still share a CU, the staging of the one-call entry
    is ordered, aligned and walked for every grid, frame and number of occluders tried -- and count_point_scene, run through such
    rows, gives the records of the numpy oracle word for word on small_case() with its boundary scene, for both facing values and
    three tolerances."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "scene_search_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "scene_search_check.cpp"), "-o", exe])
    pts, nrm, rots, trans, depth, K = small_case()
    ran = 0
    for tol in (1, 5, 30):
        scene = small_scene(tol)[0]
        for facing in (0, 1):
            src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                f.write(np.array([0x5343, len(pts), len(rots), len(trans), depth.shape[0], depth.shape[1], tol, facing], np.int32).tobytes())
                for a in (K, pts, nrm, rots, trans):
                    f.write(np.ascontiguousarray(a, np.float64).tobytes())
                f.write(np.ascontiguousarray(depth, np.uint16).tobytes())
                f.write(np.ascontiguousarray(scene, np.uint16).tobytes())
            out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "plan ok" in out.stdout and "case done" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
            got = np.fromfile(dst, SSO.DTYPE)
            want = SSO.score(pts, nrm, rots, trans, depth, scene, K, tol, facing)
            assert got.tobytes() == want.tobytes(), (tol, facing)
            ran += 1
    assert ran == 6


def test_the_scene_rule_finds_the_lost_slab_where_the_plain_search_takes_its_neighbour(se3):
    """scene_search_scene: two 90 x 90 x 20 mm slabs 92 mm apart on a 186 x 94 mm table top, T tracked and L lost, a third tracked
    slab O in front of L covering 66.6 % of its pixels; 120 x 160, +- 2 mm noise, 5 % holes, tolerance 10 mm; the default lattice
    (7 rotations x 1,331 translations = 9,317 candidates) around the place L was last seen, on the ORACLE alone.  Measured here:
      plain facing search:  the best candidate (118 inliers of 140 facing points) lies 6.0 mm from T and 90.6 mm from the true place
                            of L (half the spacing: 46 mm); under the scene rule 129 of its 140 points are hidden (claimed by T)
                            and 7 inliers are left;
      scene-aware search:   the best candidate is the true place of L, 0.0 mm off (bound: one lattice step, 17.3 mm): 46 inliers, 94
                            points hidden behind O, nothing in front, nothing seen through; the runner-up (43 inliers) lies one node
                            (10 mm) away.
    The plain count rewards the neighbour's visible face; a surface the tracked objects already explain offers nothing."""
    P = SS.poses()
    pts, nrm = SS.slab_model()
    depth, scene = SS.frame(), SS.scene()
    assert depth.shape == SS.HW and len(pts) == 280
    assert SS.covered_share() > 0.6                                                # O covers well over half of L
    rots, trans = se3.recover.lattice_factors(P["last"], 0.05, SS.TRANS_STEP, (15.0,))
    assert len(rots) == 7 and len(trans) == 1331
    truth, neighbour = P["L"][:3, 3], P["T"][:3, 3]
    spacing = float(np.linalg.norm(truth - neighbour))
    assert abs(spacing - SS.SPACING) < 1e-12
    assert np.abs(trans - truth).max(1).min() < 1e-9                               # the lattice holds the true place exactly ...
    assert np.abs(trans - neighbour).max(1).min() <= SS.TRANS_STEP / 2 + 1e-9      # ... and the neighbour's within half a step per axis
    plain = PGO.score(pts, nrm, rots, trans, depth, SS.K, SS.TOL, 1)
    aware = SSO.score(pts, nrm, rots, trans, depth, scene, SS.K, SS.TOL, 1)
    SSO.check_invariants(aware, len(pts), SS.TOL, 1)
    b_plain, b_aware = int(PSO.rank(plain, 1)[0]), int(SSO.rank(aware, 1)[0])
    d_plain = float(np.linalg.norm(trans[b_plain % len(trans)] - truth))
    d_aware = float(np.linalg.norm(trans[b_aware % len(trans)] - truth))
    print("plain: best %d %s, %.1f mm from the truth, %.1f mm from the neighbour; under the scene rule %s" %
          (b_plain, plain[b_plain], 1000 * d_plain, 1000 * np.linalg.norm(trans[b_plain % len(trans)] - neighbour), aware[b_plain]))
    print("scene-aware: best %d %s, %.1f mm from the truth" % (b_aware, aware[b_aware], 1000 * d_aware))
    assert d_plain > spacing / 2                                                   # the plain winner lies on the tracked slab
    assert np.linalg.norm(trans[b_plain % len(trans)] - neighbour) < spacing / 2
    assert aware[b_plain]["hidden_pts"] > 0                                        # which the scene rule sees as claimed
    assert d_aware <= SS.TRANS_STEP * np.sqrt(3)
    assert aware[b_aware]["hidden_pts"] > aware[b_aware]["inlier_pts"] > 0         # more than half hidden, the rest confirmed
