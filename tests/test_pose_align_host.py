"""CPU: the host side of the pose alignment (se3tn_align_poses, se3tn_align_poses_host, Engine.align_poses): the numpy oracle the GPU
tests hold the library to (tests/pose_align_oracle.py) agrees with a plain per-point loop on Python floats; the statements the kernel
runs (csrc/pose_align_math.h, csrc/pose_align_plan.h), compiled for the host with -ffp-contract=off under AddressSanitizer + UBSan,
give the oracle's poses, records and sums BYTE FOR BYTE; on the scene of tests/pose_grid_scene.py the alignment takes perturbed
poses and the hypotheses of the search to the truth; the C ABI refuses bad arguments on a host-only context, each with its own
message.  The device results are held to the oracle in tests/test_gpu_pose_align.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pose_align_cases as CS
import pose_align_oracle as PAO
import pose_grid_scene as SC
import pose_search_oracle as PSO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_vectorised_oracle_equals_the_loop_all_words():
    pts, nrm, poses, depth, K = CS.l_case()
    vec = PAO.align(pts, nrm, poses, depth, K, iters=6)
    assert same(vec, PAO.align_loop(pts, nrm, poses, depth, K, iters=6))
    out, rec, sums = PAO.align(pts, nrm, poses, depth, K, **CS.DEFAULTS)
    limits = PAO.align_limits(pts, nrm, poses, depth, K, (1, 2, 6, 20))                # one walk for several iteration limits: the same words
    assert same(limits[6], vec) and same(limits[20], (out, rec, sums))
    assert all(same(limits[k], PAO.align(pts, nrm, poses, depth, K, iters=k)) for k in (1, 2))
    # the cases show what they are meant to show
    assert list(rec["status"]) == [PAO.CONVERGED, PAO.FEW, PAO.FEW, PAO.FEW, PAO.CONVERGED]
    assert list(rec["iterations"][1:4]) == [1, 1, 1] and list(rec["pairs"][1:4]) == [0, 0, 0] and rec["facing_pts"][2] == 0
    assert rec["facing_pts"][1] > 0 and rec["facing_pts"][3] > 0                 # behind / off the frame: facing, but nothing in frame
    assert out[1:4, :3].tobytes() == poses[1:4, :3].tobytes()                    # the bits they came in with, the NaN included
    assert (out[:, 3] == (0.0, 0.0, 0.0, 1.0)).all() and (rec["_reserved"] == 0).all()
    for i in (0, 4):
        err = PAO.pose_error(out[i], SC.true_pose())
        assert err[0] <= CS.BOUND_M and err[1] <= CS.BOUND_DEG, (i, err)
        assert rec["sum_r2"][i] < rec["sum_r2_0"][i] and rec["pairs"][i] >= rec["pairs0"][i] and 1 < rec["iterations"][i] < 20
        assert sums[i, 27] == rec["sum_r2"][i] and sums[i, 0] > 0
    # the zero normals: with them restored the same pose sees two more facing points
    full = SC.l_model()[1]
    assert PAO.align(pts, full, poses[:1], depth, K, iters=1)[1]["facing_pts"][0] == PAO.align(pts, nrm, poses[:1], depth, K, iters=1)[1]["facing_pts"][0] + 2


def test_the_frontal_plane_is_singular_without_damping_and_stays_put_with_it():
    pts, nrm, poses, depth, K = CS.plane_case()
    out0, rec0, sums0 = PAO.align(pts, nrm, poses, depth, K, damping=0.0)
    assert same((out0, rec0, sums0), PAO.align_loop(pts, nrm, poses, depth, K, damping=0.0))
    assert rec0["status"][0] == PAO.SINGULAR and rec0["iterations"][0] == 1 and rec0["pairs"][0] == len(pts)
    assert out0[0, :3].tobytes() == poses[0, :3].tobytes()
    assert sums0[0, 2] == 0 and sums0[0, 11] == 0                                # S_A[0][2] and S_A[2][2]: exactly nothing turns about z
    out, rec, sums = PAO.align(pts, nrm, poses, depth, K, damping=1e-6)
    assert same((out, rec, sums), PAO.align_loop(pts, nrm, poses, depth, K, damping=1e-6))
    for i in (0, 1):
        assert rec["status"][i] in (PAO.CONVERGED, PAO.ITERS), rec[i]
        moved = np.linalg.norm(out[i, :2, 3] - poses[i, :2, 3])
        print("plane pose %d: %s, in-plane translation moved %.3f mm, z = %.6f" % (i, rec[i], 1000 * moved, out[i, 2, 3]))
        assert moved < 0.001                                                     # the directions depth cannot observe stay put
        assert abs(out[i, 2, 3] - 0.5) < 1e-4 and abs(out[i, 2, 2] - 1.0) < 1e-6   # on the surface, frontal
        assert rec["sum_r2"][i] < rec["sum_r2_0"][i]


def build_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pose_align_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pose_align_check.cpp"), "-o", exe])
    return exe


def test_the_shared_header_on_the_host_equals_the_oracle_byte_for_byte(tmp_path):
    """csrc/pose_align_math.h and pose_align_plan.h in a stand-alone host program under AddressSanitizer + UBSan: the plan's walk
    visits every point once for P in {1, 63, 64, 65, T - 1, T, T + 1, 2 T + 1}; the L case, the plane case (damping 0 and 1e-6), a
    one-iteration run with another gate and min_pairs, and a point count above the thread count come out as the oracle has them."""
    exe = build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pose_align_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    pts, nrm, poses, depth, K = CS.l_case()
    tiled = (np.concatenate([pts, pts[:209] + 1e-4]), np.concatenate([nrm, nrm[:209]]))      # 513 points: past 2 x 256 threads
    runs = [(CS.l_case(), CS.DEFAULTS), (CS.l_case(), dict(CS.DEFAULTS, gate_mm=5, iters=1, min_pairs=150, stop=0.0)),
            (CS.plane_case(), dict(CS.DEFAULTS, damping=0.0)), (CS.plane_case(), CS.DEFAULTS),
            ((tiled[0], tiled[1], poses, depth, K), dict(CS.DEFAULTS, iters=3, stop=0.0))]
    for k, (case, prm) in enumerate(runs):
        want = PAO.align(*case, **prm)
        src, dst = str(tmp_path / ("case%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        CS.write_case(src, *case, **prm)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (k, out.returncode, out.stdout[-2000:], out.stderr[-4000:])
        got = CS.read_result(dst, len(case[2]))
        for name, g, w in zip(("poses", "records", "sums"), got, want):
            assert g.tobytes() == w.tobytes(), (k, name, g, w)


def test_forty_seeded_perturbations_end_at_the_truth():
    """Perturbations of up to 12 degrees and 12 mm per axis of the true pose of the L (304 points, 120 x 160 frame, 5 % holes), the
    defaults (gate 20 mm, damping 1e-6, stop 1e-6, 20 iterations).  The bound: one pixel's footprint at 0.5 m, 0.5 / 266.7 m, plus
    the 1 mm depth quantum = 2.9 mm, and that length over the L's 120 mm = 1.4 degrees; at least 38 of 40 within it.  Measured on the
    oracle: 40 of 40 end 1.37 mm / 0.016 degrees from the truth in 5 to 12 iterations, all CONVERGED."""
    pts, nrm, depth = CS.l_scene()
    G = SC.true_pose()
    out, rec, _ = PAO.align(pts, nrm, CS.perturbed(40), depth, SC.K, **CS.DEFAULTS)
    errs = np.array([PAO.pose_error(o, G) for o in out])
    good = (errs[:, 0] <= CS.BOUND_M) & (errs[:, 1] <= CS.BOUND_DEG)
    print("within the bound: %d of 40; worst %.2f mm / %.3f deg; iterations %d to %d" % (
        good.sum(), 1000 * errs[:, 0].max(), errs[:, 1].max(), rec["iterations"].min(), rec["iterations"].max()))
    assert good.sum() >= 38
    fit = CS.facing_fit(pts, nrm, out[good][:1], depth, SC.K, SC.TOL)[0]
    assert fit["inlier_pts"] >= 0.9 * fit["points"]


def test_the_acquire_chain_ends_at_the_truth_and_widens_the_margin():
    """rotation_grid(40, 6) x depth_seeds(stride 8), top 8, the local lattice, then alignment, all on the oracle.  Measured: the 10 mm
    facing inliers are [97, 119, 112, 98, 102, 99, 102, 106] after the local lattice and [111, 146, 135, 107, 59, 69, 51, 135] after
    alignment; the winner (146 of 152) lies 1.37 mm / 0.016 degrees from the truth, its half-turn twin stops at 135."""
    ch = CS.acquire_chain(8)
    G = SC.true_pose()
    keys = PSO.keys(ch["aligned_fit"])
    best = int(np.argmax(keys))
    err = PAO.pose_error(ch["aligned"][best], G)
    print("local %s -> aligned %s; winner %d at %.2f mm / %.3f deg" % (ch["local_fit"]["inlier_pts"], ch["aligned_fit"]["inlier_pts"], best,
                                                                      1000 * err[0], err[1]))
    assert err[0] <= CS.BOUND_M and err[1] <= CS.BOUND_DEG
    assert ch["aligned_fit"]["inlier_pts"][best] >= 0.9 * ch["aligned_fit"]["points"][best]
    assert keys[best] > max(PSO.keys(ch["local_fit"]))
    assert ch["aligned_fit"]["inlier_pts"][best] > ch["local_fit"]["inlier_pts"].max()


def test_symbols_and_the_ctypes_mirror_follow_the_header(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("se3tn_align_poses", "se3tn_align_poses_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.exported_symbols(), name

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))

    assert define("SE3TN_POSE_ALIGN_MAX_POSES") == L.POSE_ALIGN_MAX_POSES == 4096
    assert define("SE3TN_POSE_ALIGN_MAX_ITERS") == L.POSE_ALIGN_MAX_ITERS == 64
    assert define("SE3TN_POSE_ALIGN_SUMS") == L.POSE_ALIGN_SUMS == PAO.SUMS == 28
    for k, name in enumerate(("ITERS", "CONVERGED", "FEW", "SINGULAR")):
        assert define("SE3TN_ALIGN_" + name) == getattr(L, "ALIGN_" + name) == getattr(PAO, name) == k
    assert L.ALIGN_REC_DTYPE.itemsize == 40 == C.sizeof(L.AlignRec) and L.ALIGN_REC_DTYPE == PAO.REC_DTYPE
    assert [f[0] for f in L.AlignRec._fields_] == list(L.ALIGN_REC_DTYPE.names)
    assert [L.ALIGN_REC_DTYPE.fields[k][1] for k in L.ALIGN_REC_DTYPE.names] == [getattr(L.AlignRec, k).offset for k in L.ALIGN_REC_DTYPE.names]
    body = re.search(r"typedef struct se3tn_align_rec \{(.*?)\} se3tn_align_rec;", hdr, re.S).group(1)
    assert re.findall(r"(?:uint32_t|int64_t)\s+(\w+);", body) == list(L.ALIGN_REC_DTYPE.names)
    body = re.search(r"typedef struct se3tn_align_params \{(.*?)\} se3tn_align_params;", hdr, re.S).group(1)
    assert re.findall(r"(?:int32_t|double)\s+(\w+);", body) == [f[0] for f in L.AlignParams._fields_] and C.sizeof(L.AlignParams) == 32
    assert "rotation is taken about the object's origin" in hdr and "fx(v)" in hdr


def test_refusals_on_a_host_only_context_each_with_its_message(se3):
    """Every NULL pointer and every number out of range is refused with SE3TN_E_ARG and a message of its own BEFORE the context is found
    to have no device -- and the points handle is not read before that (a fake one stands in)."""
    L = se3._lib
    lib = L.load()
    eng = se3.Engine(-1, 1)
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    Kp = buf.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(gate_mm=20, iters=20, min_pairs=12, _reserved=0, damping=1e-6, stop=1e-6)

    def call(fn, ctx=eng._h, pts=p, n=3, poses=p, depth=p, H=4, W=4, Kq=Kp, prm=True, out=p, rec=p, sums=p, **kw):
        g = dict(good, **kw)
        q = L.AlignParams(g["gate_mm"], g["iters"], g["min_pairs"], g["_reserved"], g["damping"], g["stop"])
        return fn(ctx, pts, n, poses, depth, H, W, Kq, C.byref(q) if prm else None, out, rec, sums, None)

    for fn in (lib.se3tn_align_poses, lib.se3tn_align_poses_host):
        assert call(fn) == -1 and b"host-only" in lib.se3tn_last_error()            # good numbers: the context is what is wrong
        assert call(fn, sums=None) == -1 and b"host-only" in lib.se3tn_last_error()   # the sums are optional
        for name in ("ctx", "pts", "poses", "depth", "Kq", "out", "rec"):
            assert call(fn, **{name: None}) == -1 and b"NULL" in lib.se3tn_last_error(), name
        assert call(fn, prm=False) == -1 and b"NULL" in lib.se3tn_last_error()
        for n in (0, -1, 4097, 2 ** 30):
            assert call(fn, n=n) == -1 and b"SE3TN_POSE_ALIGN_MAX_POSES" in lib.se3tn_last_error(), n
        assert call(fn, n=4096) == -1 and b"host-only" in lib.se3tn_last_error()
        for kw, word in ((dict(gate_mm=0), b"gate_mm"), (dict(gate_mm=65536), b"gate_mm"), (dict(iters=0), b"SE3TN_POSE_ALIGN_MAX_ITERS"),
                         (dict(iters=65), b"SE3TN_POSE_ALIGN_MAX_ITERS"), (dict(min_pairs=5), b"min_pairs"),
                         (dict(min_pairs=2 ** 20 + 1), b"min_pairs"), (dict(_reserved=1), b"_reserved"), (dict(damping=-1e-9), b"damping"),
                         (dict(damping=np.nan), b"damping"), (dict(damping=np.inf), b"damping"), (dict(stop=-1.0), b"stop is"),
                         (dict(stop=np.nan), b"stop is"), (dict(stop=np.inf), b"stop is"), (dict(H=0), b"empty frame"), (dict(W=-1), b"empty frame")):
            assert call(fn, **kw) == -1 and word in lib.se3tn_last_error(), (kw, lib.se3tn_last_error())
        for kw in (dict(iters=64), dict(iters=1), dict(min_pairs=6), dict(min_pairs=2 ** 20), dict(gate_mm=1), dict(gate_mm=65535),
                   dict(damping=0.0), dict(stop=0.0)):
            assert call(fn, **kw) == -1 and b"host-only" in lib.se3tn_last_error(), kw          # the ends of the ranges are allowed
    with pytest.raises(L.Se3tnError):
        eng.align_poses(np.zeros((4, 3)), np.eye(4)[None], np.zeros((4, 4), np.uint16), np.eye(3))   # no handle
    eng.close()
