"""CPU: the host side of the scene-aware pose alignment (se3tn_align_poses_scene, se3tn_align_poses_scene_host,
Engine.align_poses(scene=...)): the numpy oracle the GPU tests hold the library to (tests/scene_align_oracle.py) agrees with a plain
per-point loop on Python floats and, with an all-zero scene, with the plain oracle byte for byte; the hidden verdict sits exactly on
its edges; the statements the kernel runs (csrc/pose_point_rule.h, pose_align_math.h, pose_align_plan.h), compiled for the host with
-ffp-contract=off under AddressSanitizer + UBSan in a stand-alone program, give the oracle's poses, records and sums BYTE FOR BYTE; on
the stacked scene and on the scene of tests/scene_search_scene.py the rule does what it is for; the C ABI refuses bad arguments on a
host-only context, each with its own message.  The device results are held to the oracle in tests/test_gpu_scene_align.py.  No
sanitizer runs on code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pose_align_oracle as PAO
import scene_align_oracle as SAO
import scene_align_scene as AS
import scene_search_scene as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def boundary_case(tol):
    """SS.device_case() as an alignment case: (pts, nrm, poses [12,4,4], depth, scene, K, marks)"""
    case = SS.device_case()
    pts, nrm, _, _, depth, K = case
    scene, marks = SS.boundary_scene(case, tol)
    return pts, nrm, AS.device_poses(case), depth, scene, K, marks


def test_vectorised_oracle_equals_the_loop_all_words():
    for tol, prm in ((10, dict(AS.DEFAULTS, iters=3)), (1, dict(AS.DEFAULTS, iters=2, gate_mm=40, min_pairs=6, stop=0.0))):
        pts, nrm, poses, depth, scene, K, _ = boundary_case(tol)
        vec = SAO.align(pts, nrm, poses, depth, scene, K, tol, **prm)
        assert same(vec, SAO.align_loop(pts, nrm, poses, depth, scene, K, tol, **prm)), tol
        rec = vec[1]
        assert rec.dtype == SAO.REC_DTYPE and rec["hidden_pts"].max() > 0 and rec["pairs"].max() > 0
        assert (rec["pairs"] + rec["hidden_pts"] <= rec["facing_pts"]).all()
    # the stacked scene's first perturbations, all 20 iterations
    pts, nrm = SS.slab_model()
    depth, scene, poses = AS.stacked_frame(0), AS.stacked_scene(), AS.perturbed(3)
    assert same(SAO.align(pts, nrm, poses, depth, scene, AS.K, AS.TOL, **AS.DEFAULTS),
                SAO.align_loop(pts, nrm, poses, depth, scene, AS.K, AS.TOL, **AS.DEFAULTS))


def test_an_all_zero_scene_is_the_plain_oracle_byte_for_byte():
    pts, nrm, poses, depth, scene, K, _ = boundary_case(10)
    for prm in (AS.DEFAULTS, dict(AS.DEFAULTS, iters=1, gate_mm=5)):
        got = SAO.align(pts, nrm, poses, depth, np.zeros_like(scene), K, 10, **prm)
        want = PAO.align(pts, nrm, poses, depth, K, **prm)
        assert same(got, want) and (got[1]["hidden_pts"] == 0).all()
        assert not same(SAO.align(pts, nrm, poses, depth, scene, K, 10, **prm), want)      # (and the scene of the case does matter)
    pts, nrm = SS.slab_model()
    depth = AS.stacked_frame(0)
    assert same(SAO.align(pts, nrm, AS.perturbed(5), depth, np.zeros_like(depth), AS.K, AS.TOL, **AS.DEFAULTS),
                PAO.align(pts, nrm, AS.perturbed(5), depth, AS.K, **AS.DEFAULTS))


def test_the_hidden_verdict_sits_on_its_edges():
    """On SS.boundary_scene(SS.device_case(), tol): under pose 0 the point whose pixel holds m + tol is hidden, the one at m + tol + 1 is
    not; scene values 0, 100 and 2000 never hide, 101 and 1999 hide exactly when they are <= m + tol; the NaN rotation and the
    translation behind the camera hide and pair nothing; pairs + hidden <= facing."""
    for tol in (1, 10, 30):
        pts, nrm, poses, depth, scene, K, marks = boundary_case(tol)
        R, t = poses[0, :3, :3], poses[0, :3, 3]
        uf, vf, m = SS.pixels_of(pts, R, t, K)
        for (pix, mm), hidden_there in zip(marks, (True, False)):
            j = int(np.flatnonzero((vf == pix[0]) & (uf == pix[1]))[0])                  # the point that owns the pixel
            assert m[j] == mm and scene[pix] == mm + tol + (0 if hidden_there else 1)
            one = (pts[j:j + 1], np.ascontiguousarray((-(R @ pts[j] + t) @ R)[None]))    # a normal that points at the camera: facing
            for val, want in ((scene[pix], hidden_there), (0, False), (100, False), (101, True), (1999, False), (2000, False),
                              (mm + tol, True), (mm + tol + 1, False)):
                sc = scene.copy()
                sc[pix] = val
                for fn in (SAO.sums_of_scene, SAO.sums_of_scene_loop):
                    _, pairs, facing, hidden = fn(one[0], one[1], R, t, depth, sc, K, 65535, tol)
                    assert facing == 1 and hidden == int(want), (tol, pix, val, fn.__name__)
                    assert pairs == int(not want and 100 < depth[pix] < 2000), (tol, pix, val)
            # a surface at 1999 hides a point at 1999 mm; one at 2000 is no surface
            far = np.eye(4)
            far[:3, 3] = (0.0, 0.0, 1.999)
            sc = np.full_like(scene, 1999)
            _, pairs, facing, hidden = SAO.sums_of_scene(np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]]), far[:3, :3], far[:3, 3], depth, sc, K, 20, tol)
            assert (facing, hidden, pairs) == (1, 1, 0)
            sc[:] = 2000
            assert SAO.sums_of_scene(np.zeros((1, 3)), np.array([[0.0, 0.0, -1.0]]), far[:3, :3], far[:3, 3], depth, sc, K, 20, tol)[3] == 0
        out, rec, sums = SAO.align(pts, nrm, poses, depth, scene, K, tol, **dict(AS.DEFAULTS, iters=1))
        assert (rec["pairs"] + rec["hidden_pts"] <= rec["facing_pts"]).all() and rec["hidden_pts"][:3].min() > 0
        assert (rec["hidden_pts"][3::4] == 0).all() and (rec["pairs"][3::4] == 0).all()      # behind the camera
        assert (rec["hidden_pts"][8:] == 0).all() and (rec["status"][8:] == SAO.FEW).all()  # the rotation with the NaN
        assert out[8:, :3].tobytes() == poses[8:, :3].tobytes()


def test_stacked_scene_plain_alignment_fails_and_the_scene_rule_ends_at_the_truth():
    """A tracked slab S lies on the lost slab L, its near face 20 mm in front of L's (inside the gate), covering 43 % of it; 40 seeded
    perturbations of up to 8 degrees and 8 mm per axis.  The bound: 2.9 mm / 1.85 degrees (scene_align_scene).  Plain alignment: 0 of
    40 within it (median 13.8 mm / 22.4 degrees: L's covered points pair with S's face and tilt L up); the scene rule: at least 38 of
    40.  Measured on the oracle: 39 of 40, median 1.37 mm / 0.42 degrees."""
    assert 0.40 < AS.stacked_covered_share() < 0.46
    truth = AS.stacked_poses()["L"]
    res = AS.stacked_aligned(0)
    plain, plain_errs = AS.within(res["plain"][0], truth)
    good, errs = AS.within(res["scene"][0], truth)
    print("plain: %d of 40, median %.1f mm / %.1f deg; scene rule: %d of 40, median %.2f mm / %.2f deg" % (
        plain.sum(), 1000 * np.median(plain_errs[:, 0]), np.median(plain_errs[:, 1]), good.sum(), 1000 * np.median(errs[:, 0]),
        np.median(errs[:, 1])))
    assert plain.sum() == 0
    assert good.sum() >= 38
    rec = res["scene"][1]
    assert (rec["pairs"] + rec["hidden_pts"] <= rec["facing_pts"]).all() and (rec["hidden_pts"][good] > 0).all()


def test_existing_scene_the_pool_choice_reaches_the_truth_only_with_the_scene_rule():
    """MultiTracker.recover(align=20, refine=0) on the oracles around a `last` pose off the lattice, with and without a further turn
    of 5 degrees: plain alignment drags all 8 top nodes onto the tracked neighbour T (over 30 mm from the truth), so the pool's choice
    stays at the lattice node, 15.17 mm away; under the scene rule the choice ends within 2.9 mm / 1.85 degrees.  Measured: 1.12 mm /
    1.23 degrees with the turn, 1.39 mm / 1.14 degrees without."""
    truth = SS.poses()["L"]
    for turn in (True, False):
        plain, scene = AS.pool(turn, False), AS.pool(turn, True)
        e_plain, e_scene = PAO.pose_error(plain["pose"], truth), PAO.pose_error(scene["pose"], truth)
        drag = [PAO.pose_error(a, truth)[0] for a in plain["aligned"]]
        print("turn %s: plain choice %d at %.2f mm / %.2f deg, aligned %.1f to %.1f mm off; scene rule choice %d at %.2f mm / %.2f deg" % (
            turn, plain["chosen"], 1000 * e_plain[0], e_plain[1], 1000 * min(drag), 1000 * max(drag), scene["chosen"], 1000 * e_scene[0],
            e_scene[1]))
        assert np.array_equal(plain["top_idx"], scene["top_idx"])                            # the search is the same: only step (3) differs
        assert min(drag) > 0.030 and plain["chosen"] >= 8                                    # every aligned pose is worse than its node
        assert round(1000 * e_plain[0], 2) == 15.17                                          # the lattice node, a step and a half away
        assert e_scene[0] <= AS.BOUND_M and e_scene[1] <= AS.BOUND_DEG and scene["chosen"] < 8
        assert scene["align_rec"].dtype == SAO.REC_DTYPE and scene["align_rec"]["hidden_pts"].min() > 0


def build_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pose_align_scene_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pose_align_scene_check.cpp"), "-o", exe])
    return exe


def test_the_shared_header_on_the_host_equals_the_oracle_byte_for_byte(tmp_path):
    """csrc/pose_point_rule.h, pose_align_math.h and pose_align_plan.h in a stand-alone host program under AddressSanitizer + UBSan:
    hidden() on its edges, the 31-word row walk, pa_stage_scene; then the boundary case (1,100 points: past four strides of 256
    threads, tol 10 and 1), an all-zero scene, and perturbations of the stacked scene come out as the oracle has them."""
    exe = build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pose_align_scene_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    b10, b1 = boundary_case(10), boundary_case(1)
    pts, nrm = SS.slab_model()
    runs = [(b10[:6], 10, dict(AS.DEFAULTS, iters=3)), (b1[:6], 1, dict(AS.DEFAULTS, iters=2, gate_mm=40, min_pairs=6, stop=0.0)),
            ((*b10[:4], np.zeros_like(b10[4]), b10[5]), 10, AS.DEFAULTS),
            ((pts, nrm, AS.perturbed(4), AS.stacked_frame(0), AS.stacked_scene(), AS.K), AS.TOL, AS.DEFAULTS)]
    for k, (case, tol, prm) in enumerate(runs):
        want = SAO.align(*case, tol, **prm)
        src, dst = str(tmp_path / ("case%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        AS.write_case(src, *case, tol, **prm)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (k, out.returncode, out.stdout[-2000:], out.stderr[-4000:])
        got = AS.read_result(dst, len(case[2]))
        for name, g, w in zip(("poses", "records", "sums"), got, want):
            assert g.tobytes() == w.tobytes(), (k, name, g, w)
    assert want[1]["hidden_pts"].min() > 0


def test_symbols_and_the_ctypes_mirror_follow_the_header(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ("se3tn_align_poses_scene", "se3tn_align_poses_scene_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.exported_symbols(), name
    D = L.SCENE_ALIGN_REC_DTYPE
    assert D.itemsize == 40 == C.sizeof(L.SceneAlignRec) and D == SAO.REC_DTYPE
    assert [n if n != "hidden_pts" else "_reserved" for n in D.names] == list(L.ALIGN_REC_DTYPE.names)
    assert [D.fields[k][1] for k in D.names] == [L.ALIGN_REC_DTYPE.fields[k][1] for k in L.ALIGN_REC_DTYPE.names] and D.fields["hidden_pts"][1] == 28
    assert [f[0] for f in L.SceneAlignRec._fields_] == list(D.names)
    assert [D.fields[k][1] for k in D.names] == [getattr(L.SceneAlignRec, k).offset for k in D.names]
    body = re.search(r"typedef struct se3tn_scene_align_rec \{(.*?)\} se3tn_scene_align_rec;", hdr, re.S).group(1)
    assert re.findall(r"(?:uint32_t|int64_t)\s+(\w+);", body) == list(D.names)
    # the plain record and the parameters are untouched
    body = re.search(r"typedef struct se3tn_align_rec \{(.*?)\} se3tn_align_rec;", hdr, re.S).group(1)
    assert re.findall(r"(?:uint32_t|int64_t)\s+(\w+);", body) == list(L.ALIGN_REC_DTYPE.names) and "_reserved" in L.ALIGN_REC_DTYPE.names
    assert C.sizeof(L.AlignParams) == 32 and C.sizeof(L.AlignRec) == 40
    assert "pairs + hidden_pts <= facing_pts" in hdr and "all-zero scene" in hdr and "scene_tol_mm" in hdr


def test_refusals_on_a_host_only_context_each_with_its_message(se3):
    """Every refusal of se3tn_align_poses / _host, in its order and with its message, a NULL scene among the NULL pointers and
    scene_tol_mm outside [1, 65535] -- all BEFORE the context is found to have no device, and the points handle is not read before
    that (a fake one stands in).  The ends of the ranges are allowed."""
    L = se3._lib
    lib = L.load()
    eng = se3.Engine(-1, 1)
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    Kp = buf.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(gate_mm=20, iters=20, min_pairs=12, _reserved=0, damping=1e-6, stop=1e-6)

    def call(fn, ctx=eng._h, pts=p, n=3, poses=p, depth=p, scene=p, H=4, W=4, Kq=Kp, prm=True, tol=10, out=p, rec=p, sums=p, **kw):
        g = dict(good, **kw)
        q = L.AlignParams(g["gate_mm"], g["iters"], g["min_pairs"], g["_reserved"], g["damping"], g["stop"])
        return fn(ctx, pts, n, poses, depth, scene, H, W, Kq, C.byref(q) if prm else None, tol, out, rec, sums, None)

    for fn in (lib.se3tn_align_poses_scene, lib.se3tn_align_poses_scene_host):
        assert call(fn) == -1 and b"host-only" in lib.se3tn_last_error()            # good numbers: the context is what is wrong
        assert call(fn, sums=None) == -1 and b"host-only" in lib.se3tn_last_error()   # the sums are optional
        for name in ("ctx", "pts", "poses", "depth", "scene", "Kq", "out", "rec"):
            assert call(fn, **{name: None}) == -1 and b"NULL" in lib.se3tn_last_error(), name
        assert call(fn, prm=False) == -1 and b"NULL" in lib.se3tn_last_error()
        for n in (0, -1, 4097, 2 ** 30):
            assert call(fn, n=n) == -1 and b"SE3TN_POSE_ALIGN_MAX_POSES" in lib.se3tn_last_error(), n
        assert call(fn, n=4096) == -1 and b"host-only" in lib.se3tn_last_error()
        for kw, word in ((dict(gate_mm=0), b" gate_mm"), (dict(gate_mm=65536), b" gate_mm"), (dict(iters=0), b"SE3TN_POSE_ALIGN_MAX_ITERS"),
                         (dict(iters=65), b"SE3TN_POSE_ALIGN_MAX_ITERS"), (dict(min_pairs=5), b"min_pairs"),
                         (dict(min_pairs=2 ** 20 + 1), b"min_pairs"), (dict(_reserved=1), b"_reserved"), (dict(damping=-1e-9), b"damping"),
                         (dict(damping=np.nan), b"damping"), (dict(damping=np.inf), b"damping"), (dict(stop=-1.0), b"stop is"),
                         (dict(stop=np.nan), b"stop is"), (dict(stop=np.inf), b"stop is"), (dict(tol=0), b"scene_tol_mm"),
                         (dict(tol=-3), b"scene_tol_mm"), (dict(tol=65536), b"scene_tol_mm"), (dict(H=0), b"empty frame"),
                         (dict(W=-1), b"empty frame")):
            assert call(fn, **kw) == -1 and word in lib.se3tn_last_error(), (kw, lib.se3tn_last_error())
        # the order of se3tn_align_poses: n before gate_mm before iters; the gate before the scene tolerance; that before the frame
        assert call(fn, n=0, gate_mm=0) == -1 and b"SE3TN_POSE_ALIGN_MAX_POSES" in lib.se3tn_last_error()
        assert call(fn, gate_mm=0, tol=0) == -1 and b" gate_mm" in lib.se3tn_last_error() and b"scene_tol_mm" not in lib.se3tn_last_error()
        assert call(fn, tol=0, H=0) == -1 and b"scene_tol_mm" in lib.se3tn_last_error()
        for kw in (dict(iters=64), dict(iters=1), dict(min_pairs=6), dict(min_pairs=2 ** 20), dict(gate_mm=1), dict(gate_mm=65535),
                   dict(damping=0.0), dict(stop=0.0), dict(tol=1), dict(tol=65535)):
            assert call(fn, **kw) == -1 and b"host-only" in lib.se3tn_last_error(), kw          # the ends of the ranges are allowed
    with pytest.raises(L.Se3tnError):
        eng.align_poses(np.zeros((4, 3)), np.eye(4)[None], np.zeros((4, 4), np.uint16), np.eye(3), scene=np.zeros((4, 4), np.uint16))   # no handle
    eng.close()
