"""CPU: the host side of the scene-aware colour verification -- the depth record's dtype mirror and the exported symbols, the refusals
that need no device, the per-pixel loop of tests/scene_verify_oracle.py held to color_fit_oracle.record under an all-zero scene,
utils.fit_stats(scene=) / utils.color_stats(scene=) (the NumPy statement of se3tn_color_stats_scene) against that loop, csrc/fit_rule.h's
scene-aware classifier in a stand-alone host program under sanitizers, and the slab-and-plate scene of tests/scene_verify_scene.py
evaluated with the oracle renderer and the loops alone: the plain rule confirms the half-turned pose, the scene rule the true one.
Every comparison of records is an equality.  Without the feature every test fails: the names do not exist."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import color_fit_oracle as CO
import color_fit_scene as CS
import scene_verify_oracle as VO
import scene_verify_scene as VS
from oracle import se3_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
TOL = VS.TOL


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def crop(desc):
    """O.crop_bbox of a descriptor (depth alone for a scene descriptor); a window that misses the image is all zeros"""
    l, t, r, b = desc["window"]
    h, w = desc["depth"].shape
    if r <= 0 or b <= 0 or l >= w or t >= h:
        return np.zeros((176, 176, 3), np.uint8), np.zeros((176, 176), np.uint16)
    rgb = desc["rgb"] if "rgb" in desc else np.zeros((h, w, 3), np.uint8)
    return O.crop_bbox(rgb, desc["depth"], np.array([[t, l], [b, r]]))


def test_record_layout_symbols_and_refusals_without_a_device(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    # the depth record keeps se3tn_fit's 32 bytes; the mirror names the last word hidden_px
    assert L.SCENE_CROP_FIT_DTYPE.itemsize == L.FIT_DTYPE.itemsize == 32
    assert list(L.SCENE_CROP_FIT_DTYPE.names) == list(L.FIT_DTYPE.names[:-1]) + ["hidden_px"] and L.FIT_DTYPE.names[-1] == "_reserved"
    assert [L.SCENE_CROP_FIT_DTYPE.fields[k][1] for k in L.SCENE_CROP_FIT_DTYPE.names] == list(range(0, 32, 4))
    assert int(re.search(r"#define SE3TN_FIT_SCENE_MAX_PAIRS (\d+)", hdr).group(1)) == L.FIT_SCENE_MAX_PAIRS == 16
    internal = open(os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc", "se3tn_internal.h")).read()
    assert "MAX = SE3TN_FIT_SCENE_MAX_PAIRS" in internal and 3 * 16 * C.sizeof(L.Crop) + 64 <= 4096 < 3 * 32 * C.sizeof(L.Crop)
    for name in ("se3tn_color_stats_scene", "se3tn_verify_poses_scene_host"):
        assert name in L.exported_symbols() and hasattr(C.CDLL(L.LIB_PATH), name)
    lib = L.load()
    crops = (L.Crop * 1)()
    crops[0].rgb = crops[0].depth = 8                                           # never read: every refusal below comes first
    crops[0].H = crops[0].W = crops[0].right = crops[0].bottom = 176
    fit = np.zeros(2, L.SCENE_CROP_FIT_DTYPE)
    col = np.zeros(2, L.COLOR_FIT_DTYPE)
    f, p = C.c_void_p(fit.ctypes.data), C.c_void_p(col.ctypes.data)
    eng = se3.Engine(device=-1, max_batch=2)                                    # host-only context
    assert lib.se3tn_color_stats_scene(None, crops, crops, crops, 1, 5, f, p, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, crops, crops, None, 1, 5, f, p, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, None, crops, crops, 1, 5, f, p, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, crops, crops, crops, 1, 5, f, None, None) == E_ARG
    assert lib.se3tn_color_stats_scene(eng._h, crops, crops, crops, 1, 5, f, p, None) == E_ARG and b"se3tn_color_stats_scene" in lib.se3tn_last_error()
    poses = np.tile(np.eye(4).reshape(1, 16), (2, 1)); poses[:, 11] = 0.5
    Kc = np.ascontiguousarray(CS.K)
    rgb, dep = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint16)

    def verify(h, mesh, n, tol, width=100.0, H=8, W=8, cp=p, scene=C.c_void_p(8)):
        return lib.se3tn_verify_poses_scene_host(h, mesh, C.c_void_p(poses.ctypes.data), n, Kc.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(width),
                                                 C.c_void_p(rgb.ctypes.data), C.c_void_p(dep.ctypes.data), scene, H, W, tol, f, cp, None)
    mesh = C.c_void_p(8)                                                        # never read either
    assert verify(None, mesh, 1, 5) == E_ARG and verify(eng._h, None, 1, 5) == E_ARG and verify(eng._h, mesh, 1, 5, cp=None) == E_ARG
    assert verify(eng._h, mesh, 1, 5, scene=None) == E_ARG and b"NULL" in lib.se3tn_last_error()
    assert verify(eng._h, mesh, 1, 0) == E_ARG and verify(eng._h, mesh, 1, 65536) == E_ARG and verify(eng._h, mesh, 1, 5, H=0) == E_ARG
    assert verify(eng._h, mesh, 1, 5, width=0.0) == E_ARG
    assert verify(eng._h, mesh, 1, 5) == E_ARG and b"host-only" in lib.se3tn_last_error() and b"se3tn_verify_poses_scene_host" in lib.se3tn_last_error()
    assert not fit.view(np.uint8).any() and not col.view(np.uint8).any()
    eng.close()


def test_the_loop_equals_the_colour_oracle_under_an_all_zero_scene():
    """word for word, on every case of color_fit_oracle: hidden_px stands where the plain record keeps its reserved 0"""
    want = CO.expected()
    for k, (m, o) in CO.cases().items():
        for scene in (dict(depth=np.zeros_like(o["depth"]), window=o["window"]), dict(depth=np.zeros((3, 5), np.uint16), window=(0, 0, 5, 3))):
            fit, col = VO.record(m, o, scene, CO.TOL)
            assert [fit[a] for a in VO.FIT_KEYS] == [want[k][0][b] for b in CO.FIT_KEYS], (k, fit, want[k][0])
            assert col == want[k][1], (k, col, want[k][1])


def test_the_shared_cases_reach_what_they_are_for():
    """every boundary value of the scene meets every branch of the observed depth; the scene hides something wherever it should, and
    nothing where its window misses its image"""
    cover = VS.boundary_coverage()
    for value in VS.BOUNDARY_VALUES:
        for branch in VS.BRANCHES:
            assert cover.get((value, branch), 0) > 0, (value, branch)
    want = VS.expected()
    for k, (fit, col) in want.items():
        assert fit["seen_px"] == fit["inlier_px"] + fit["front_px"] + fit["behind_px"] and col["px"] == fit["inlier_px"], k
        if k not in ("same_miss", "scene_miss"):
            assert 0 < fit["hidden_px"] < fit["model_px"] and fit["inlier_px"] > 0 and fit["front_px"] > 0 and fit["behind_px"] > 0, (k, fit)
    assert want["scene_miss"][0]["hidden_px"] == 0 and want["scene_miss"][1] == CO.expected()["identity"][1]
    assert want["same_miss"][0]["model_px"] == 0
    m, o, s = VS.cases()["other_identity"]
    assert s["depth"].shape != o["depth"].shape and s["window"] != o["window"]


def test_numpy_statements_equal_the_loop(se3):
    want = VS.expected()
    for k, (m, o, s) in VS.cases().items():
        (mr, md), (orr, od), (_, sd) = crop(m), crop(o), crop(s)
        fit = se3.utils.fit_stats(md, od, TOL, scene=sd)
        col = se3.utils.color_stats(mr, md, orr, od, TOL, scene=sd)
        fit_w, col_w = VO.as_arrays(se3, [want[k]])
        assert fit.dtype == se3._lib.SCENE_CROP_FIT_DTYPE and fit.shape == () and np.array_equal(fit, fit_w[0]), (k, fit, fit_w[0])
        assert col.dtype == se3._lib.COLOR_FIT_DTYPE and np.array_equal(col, col_w[0]), (k, col, col_w[0])
        # scene=None is the function as it was; an all-zero scene gives its words
        plain = se3.utils.fit_stats(md, od, TOL)
        assert plain.dtype == se3._lib.FIT_DTYPE and se3.utils.fit_stats(md, od, TOL, scene=np.zeros_like(sd)).tobytes() == plain.tobytes()
        assert np.array_equal(se3.utils.color_stats(mr, md, orr, od, TOL, scene=np.zeros_like(sd)), se3.utils.color_stats(mr, md, orr, od, TOL))
    # stacked crops: one record per leading index
    names = ["same_identity", "boundaries"]
    parts = [[crop(c) for c in VS.cases()[k]] for k in names]
    md, od, sd = (np.stack([p[i][1] for p in parts]) for i in range(3))
    both = se3.utils.fit_stats(md, od, TOL, scene=sd)
    assert both.shape == (2,) and np.array_equal(both, VO.as_arrays(se3, [want[k] for k in names])[0])


def _around(m, tol, with_below):
    v = [0, 100, 101, 1999, 2000, 65535, m, m + tol, m + tol + 1] + ([m - tol, m - tol - 1] if with_below else [])
    return [d for d in v if 0 <= d <= 65535]


def test_scene_classifier_under_sanitizers(tmp_path):
    """csrc/fit_rule.h in a stand-alone host program built with AddressSanitizer + UBSan (tests/c_abi/scene_verify_check.cpp): every
    (m, o, s) over the boundary set at tol 1 and 10; its counts against the loop's verdicts.  Host code only."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "scene_verify_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "scene_verify_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "scene_verify_check: ok" in out.stdout
    M = (0, 100, 101, 102, 111, 600, 1988, 1989, 1998, 1999, 2000, 65535)
    for tol in (1, 10):
        want = dict.fromkeys(("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "hidden_px"), 0)
        for m in M:
            for key, v in VO.counts([m], _around(m, tol, True), _around(m, tol, False), tol).items():
                want[key] += v
        line = re.search(r"^tol=%d (.*)$" % tol, out.stdout, re.M).group(1)
        got = {k: int(v) for k, v in (item.split("=") for item in line.split())}
        assert got == want and want["hidden_px"] > 0 and want["inlier_px"] > 0 and want["front_px"] > 0 and want["behind_px"] > 0, (tol, got, want)


def test_slab_and_plate_plain_rule_confirms_the_wrong_pose_scene_rule_the_true_one(se3):
    """The oracle renderer, the frames and the two loops, nothing recorded: a tracked plate on the slab, its colours swapped.  Under the
    plain rule the plate's pixels are depth inliers of the slab and vote for the half-turned pose; the scene rule hides them."""
    rec = VS.slab_records()
    plain = {k: VS.score(se3, rec[k]["plain"][1]) for k in rec}
    scene = {k: VS.score(se3, rec[k]["scene"][1]) for k in rec}
    print("slab and plate: plain rule true %.3f flipped %.3f (px %d); scene rule true %.3f flipped %.3f (px %d, hidden %d of %d model px)"
          % (plain["true"], plain["flipped"], rec["true"]["plain"][1]["px"], scene["true"], scene["flipped"], rec["true"]["scene"][1]["px"],
             rec["true"]["scene"][0]["hidden_px"], rec["true"]["scene"][0]["model_px"]))
    assert plain["true"] < 0 < plain["flipped"]
    assert scene["flipped"] < 0 < scene["true"]
    assert rec["true"]["scene"][0]["hidden_px"] > 0 and rec["true"]["scene"][0]["hidden_px"] == rec["flipped"]["scene"][0]["hidden_px"]
    for k in rec:
        for rule in ("plain", "scene"):
            assert rec[k][rule][1]["px"] >= VS.MIN_PX, (k, rule)
        f = rec[k]["scene"][0]
        assert f["model_px"] == rec[k]["plain"][0]["model_px"] and f["hidden_px"] + f["seen_px"] <= f["model_px"]
        assert f["seen_px"] == f["inlier_px"] + f["front_px"] + f["behind_px"]
