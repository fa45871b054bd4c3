"""CPU: the host side of the scene fit -- the record and its mirrors, the refusals that need no device, utils.scene_stats (the NumPy
statement of se3tn_scene_stats) against the per-pixel loop of tests/scene_fit_oracle.py, the identities of the rule over seeded random
layers, the occlusion scene of tests/scene_fit_scene.py evaluated with the oracle renderer and the NumPy rule alone, and
csrc/scene_fit_rule.h + scene_fit_plan.h in a stand-alone host program under sanitizers.  Every comparison is an equality.  Without the
feature every test fails: the names do not exist."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_fit_oracle as SO
import scene_fit_scene as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def test_record_layout_symbols_and_refusals_without_a_device(se3):
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    body = re.search(r"\nstruct se3tn_scene_fit \{(.*?)\n\};", hdr, re.S).group(1)
    names = re.findall(r"uint32_t\s+(\w+);", body)
    assert len(names) == 12 and L.SCENE_FIT_DTYPE.itemsize == C.sizeof(L.SceneFit) == 48
    assert names == [n for n, _ in L.SceneFit._fields_] == list(L.SCENE_FIT_DTYPE.names) == list(L.SCENE_FIT_FIELDS) + ["_reserved"]
    assert [L.SCENE_FIT_DTYPE.fields[k][1] for k in names] == [getattr(L.SceneFit, k).offset for k in names] == list(range(0, 48, 4))
    layer = re.search(r"typedef struct se3tn_scene_layer \{(.*?)\} se3tn_scene_layer;", hdr, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[4\])?;", layer) == [n for n, _ in L.SceneLayer._fields_] and C.sizeof(L.SceneLayer) == 24
    assert L.SceneLayer.rect.offset == 8
    # the overflow bound is stated, and true
    assert "2^21 x 1,898 = 3,980,394,496 < 2^32" in hdr and 2 ** 21 * (1999 - 101) == 3980394496 < 2 ** 32
    assert int(re.search(r"#define SE3TN_SCENE_MAX_OBJECTS (\d+)", hdr).group(1)) == L.SCENE_MAX_OBJECTS == 32
    assert int(re.search(r"#define SE3TN_SCENE_MAX_PIXELS (\d+)", hdr).group(1)) == L.SCENE_MAX_PIXELS == 2 ** 21
    for name in ("se3tn_scene_stats", "se3tn_scene_fit", "se3tn_scene_fit_host"):
        assert name in L.exported_symbols() and hasattr(C.CDLL(L.LIB_PATH), name)
    lib = L.load()
    eng = se3.Engine(device=-1, max_batch=40)                                   # host-only context
    rec = np.zeros(2, L.SCENE_FIT_DTYPE)
    ids, scene = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint16)
    rp, ip, sp = C.c_void_p(rec.ctypes.data), C.c_void_p(ids.ctypes.data), C.c_void_p(scene.ctypes.data)
    obs = C.c_void_p(8)                                                         # never read: every refusal below comes first

    def stats(h=eng._h, n=1, rect=(0, 0, 8, 8), depth=8, o=obs, H=8, W=8, tol=5, out=rp):
        layers = (L.SceneLayer * 40)()
        for l in layers:
            l.depth, l.rect[:] = depth, rect
        return lib.se3tn_scene_stats(h, n, layers, o, H, W, tol, out, ip, sp, None)
    assert stats(h=None) == E_ARG and stats(o=None) == E_ARG and stats(out=None) == E_ARG and stats(depth=None) == E_ARG
    assert stats(n=0) == E_ARG and stats(n=33) == E_ARG and stats(tol=0) == E_ARG and stats(tol=65536) == E_ARG
    assert stats(H=0) == E_ARG and stats(H=2049, W=1024) == E_ARG and stats(H=1 << 20, W=1 << 20) == E_ARG
    assert stats(rect=(0, 0, 9, 8)) == E_ARG and stats(rect=(-1, 0, 4, 4)) == E_ARG and stats(rect=(0, 2, 8, 9)) == E_ARG
    assert stats() == E_ARG and b"host-only" in lib.se3tn_last_error() and b"se3tn_scene_stats" in lib.se3tn_last_error()
    small = se3.Engine(device=-1, max_batch=2)                                  # n is bounded by se3tn_max_batch as well
    assert stats(h=small._h, n=3) == E_ARG and b"n = 3" in lib.se3tn_last_error()
    small.close()

    poses = np.tile(np.eye(4).reshape(1, 16), (40, 1)); poses[:, 11] = 0.5
    Kc = np.ascontiguousarray(SS.K)
    dep = np.zeros((8, 8), np.uint16)
    for fn in (lib.se3tn_scene_fit, lib.se3tn_scene_fit_host):
        def fit(h=eng._h, n=1, mesh=8, width=100.0, p=poses, K=Kc, d=C.c_void_p(dep.ctypes.data), H=8, W=8, tol=5, out=rp):
            objs = (L.Object * 40)()
            for o_ in objs:
                o_.mesh, o_.object_width_mm = mesh, width                       # (a mesh handle is never read: the refusals come first)
            return fn(h, n, objs, C.c_void_p(p.ctypes.data) if p is not None else None,
                      K.ctypes.data_as(C.POINTER(C.c_double)) if K is not None else None, d, H, W, tol, out, ip, sp, None)
        assert fit(h=None) == E_ARG and fit(p=None) == E_ARG and fit(K=None) == E_ARG and fit(d=None) == E_ARG and fit(out=None) == E_ARG
        assert fit(n=0) == E_ARG and fit(n=33) == E_ARG and fit(tol=0) == E_ARG and fit(tol=65536) == E_ARG and fit(H=0) == E_ARG
        assert fit(H=2049, W=8) == E_ARG and fit(H=2048, W=1025) == E_ARG
        behind, nan = poses.copy(), poses.copy()
        behind[0, 11], nan[0, 3] = -0.5, np.nan
        assert fit(p=behind) == E_ARG and fit(p=nan) == E_ARG and fit(mesh=None) == E_ARG and fit(width=0.0) == E_ARG
        assert fit() == E_ARG and b"host-only" in lib.se3tn_last_error()
    assert not rec.view(np.uint8).any() and not ids.any() and not scene.any()
    eng.close()


@pytest.fixture(scope="module")
def oracle_results():
    """name -> (records as a list of dicts, ids, scene) of the per-pixel loop, computed once"""
    return {k: SO.scene_stats(c["layers"], c["rects"], c["observed"], c["tol"]) for k, c in SS.cases().items()}


def test_scene_stats_numpy_equals_the_per_pixel_oracle(se3, oracle_results):
    cases = SS.cases()
    assert set(cases) >= {"single", "thresholds", "ties", "one_px", "edges", "gap", "empty_among", "all_empty", "n32", "zeros_observed"}
    got = {}
    for k, c in cases.items():
        rec, ids, scene = se3.utils.scene_stats(c["layers"], c["rects"], c["observed"], c["tol"])
        want, ids_w, scene_w = oracle_results[k]
        assert rec.dtype == se3._lib.SCENE_FIT_DTYPE and np.array_equal(rec, SO.as_array(se3, want)), (k, rec, want)
        assert ids.dtype == np.uint8 and scene.dtype == np.uint16 and ids.shape == scene.shape == (SS.H, SS.W)
        assert np.array_equal(ids, np.array(ids_w)) and np.array_equal(scene, np.array(scene_w)), k
        got[k] = rec
    # the cases are not vacuous
    r = got["single"][0]
    assert len(got["single"]) == 1 and all(int(r[k]) > 20 for k in ("inlier_px", "front_px", "behind_px")) and int(r["visible_px"]) > int(r["seen_px"])
    # depths 100 / 101 / 1999 / 2000: two of every eight columns are not valid; |o - m| at tol is an inlier, at tol + 1 it is not
    t = got["thresholds"][0]
    rows, reps = SS.H // 4, SS.W // 8
    assert int(t["model_px"]) == int(t["visible_px"]) == 6 * reps * SS.H and int(t["seen_px"]) == 6 * reps * rows
    assert int(t["inlier_px"]) == 4 * reps * rows and int(t["front_px"]) == int(t["behind_px"]) == reps * rows
    assert int(t["sum_abs_mm"]) == 4 * reps * rows * SS.TOL
    # two identical layers: layer 0 owns everything, layer 1 is all hidden behind it
    a, b = got["ties"]
    assert int(a["hidden_px"]) == 0 and int(a["visible_px"]) == int(a["model_px"]) > 1000 and int(a["hidden_by"]) == 0
    assert int(b["visible_px"]) == 0 and int(b["hidden_px"]) == int(b["model_px"]) == int(a["model_px"]) and int(b["hidden_by"]) == 1
    assert int(b["seen_px"]) == 0 and int(b["sum_abs_mm"]) == 0
    assert int(got["one_px"][0]["model_px"]) == 1
    assert all(int(r["model_px"]) > 0 for r in got["edges"]) and int(got["gap"][0]["hidden_px"]) == int(got["gap"][1]["hidden_px"]) == 0
    e = got["empty_among"]
    assert not any(int(e[i][k]) for i in (1, 3) for k in SO.FIELDS[:9]) and int(e[0]["hidden_px"]) + int(e[2]["hidden_px"]) > 50
    assert all(not any(int(r[k]) for k in SO.FIELDS[:9]) and int(r["n_objects"]) == 3 for r in got["all_empty"])
    assert not np.array(oracle_results["all_empty"][1]).any()
    n32 = got["n32"]
    assert len(n32) == 32 and int(n32["n_objects"][0]) == 32 and (n32["hidden_px"] > 0).all() and int(n32["hidden_by"].max()) >= 1 << 31
    z = got["zeros_observed"]
    assert (z["seen_px"] == 0).all() and (z["visible_px"] > 100).all()
    with pytest.raises(ValueError):
        se3.utils.scene_stats([np.zeros((4, 4), np.uint16)], [(0, 0, 4, 41)], np.zeros((SS.H, SS.W), np.uint16), 5)


def test_identities_over_seeded_random_layers(se3):
    U = se3.utils
    for seed in range(6):
        n = (2, 3, 5, 9, 17, 32)[seed]
        c = SS.random_layers(100 + seed, n, ties=seed % 2 == 0)
        rec, ids, scene = U.scene_stats(c["layers"], c["rects"], c["observed"], c["tol"])
        assert np.array_equal(rec["model_px"], rec["visible_px"] + rec["hidden_px"])
        assert np.array_equal(rec["seen_px"], rec["inlier_px"] + rec["front_px"] + rec["behind_px"])
        assert int(rec["visible_px"].sum()) == int((ids != 0).sum()) > 0
        # a bit of hidden_by agrees with the ids: object j hides object i exactly where i's layer is valid and the pixel is j's
        for i, (d, (x0, y0, x1, y1)) in enumerate(zip(c["layers"], c["rects"])):
            v = (d > 100) & (d < 2000)
            owners = set(np.unique(ids[y0:y1, x0:x1][v]).tolist()) - {i + 1}
            assert int(rec["hidden_by"][i]) == sum(1 << (j - 1) for j in owners), (seed, i)
        if seed % 2:   # without ties a permutation of the layers permutes the records and relabels the ids
            perm = np.random.default_rng(seed).permutation(n)
            rec_p, ids_p, scene_p = U.scene_stats([c["layers"][j] for j in perm], [c["rects"][j] for j in perm], c["observed"], c["tol"])
            assert np.array_equal(scene_p, scene)
            relabel = np.zeros(n + 1, np.uint8)
            relabel[perm + 1] = np.arange(n) + 1                                  # old id perm[k] + 1 -> new id k + 1
            assert np.array_equal(ids_p, relabel[ids])
            for k, j in enumerate(perm):
                for f in SO.FIELDS:
                    if f != "hidden_by":
                        assert int(rec_p[f][k]) == int(rec[f][j]), (seed, f)
                old_bits = [b for b in range(n) if int(rec["hidden_by"][j]) >> b & 1]
                assert int(rec_p["hidden_by"][k]) == sum(1 << int(np.nonzero(perm == b)[0][0]) for b in old_bits)


def test_scene_a_tracked_object_behind_another_is_hidden_not_lost(se3):
    U = se3.utils
    sc = SS.occlusion(se3)
    rec, ids, scene = U.scene_stats(sc["layers"], sc["rects"], sc["observed"], SS.TOL)
    A, B, Cc = rec
    print("scene: A %s\n       B %s\n       C %s" % (A, B, Cc))
    print("B: inlier/model %.3f  inlier/visible %.3f  hidden/model %.3f" % (B["inlier_px"] / B["model_px"], B["inlier_px"] / B["visible_px"],
                                                                              B["hidden_px"] / B["model_px"]))
    # alone B would read as lost; over the pixels where it is the nearest tracked surface it is confirmed
    assert B["inlier_px"] / B["model_px"] < 0.5
    assert B["inlier_px"] / B["visible_px"] >= 0.9
    assert 0.3 <= B["hidden_px"] / B["model_px"] <= 0.8
    assert int(B["hidden_by"]) == 1
    assert U.scene_status(rec, lost_below=0.5, min_visible=0.2)[1] == "tracked"
    assert U.scene_status(rec, lost_below=0.5, min_visible=0.5)[1] == "occluded"
    assert int(A["visible_px"]) == int(A["model_px"]) > 1000
    # C's window leaves the frame on the left: a clipped rectangle, a handful of pixels
    x0, y0, x1, y1 = sc["rects"][2]
    bb = se3.compute_bbox(sc["poses"][2], SS.K, SS.OBJECT_WIDTH_MM)
    assert 0 < int(Cc["model_px"]) < 50 and x0 == 0 and int(bb[:, 1].min()) < 0 and x1 == int(bb[:, 1].max()) < SS.HW[1]
    assert np.isclose(U.scene_ratio(rec)[1], B["inlier_px"] / B["visible_px"]) and np.isclose(U.visible_share(rec)[0], 1.0)
    # A gone from the observed frame (the wall, or B, where A was) but still in the call: A is lost, B's status does not change
    rec2 = U.scene_stats(sc["layers"], sc["rects"], sc["observed_without_A"], SS.TOL)[0]
    s1, s2 = U.scene_status(rec, 0.5, 0.2), U.scene_status(rec2, 0.5, 0.2)
    assert s1[0] == "tracked" and s2[0] == "lost" and s2[1] == s1[1] == "tracked"
    assert int(rec2["behind_px"][0]) > 0.9 * int(rec2["seen_px"][0])
    # the rule of scene_status at its edges
    one = np.zeros(4, se3._lib.SCENE_FIT_DTYPE)
    one["model_px"], one["visible_px"], one["inlier_px"] = (0, 100, 100, 100), (0, 20, 19, 50), (0, 10, 19, 24)
    assert U.scene_status(one, 0.5, 0.2) == ["occluded", "tracked", "occluded", "lost"]


def test_scene_plan_and_rule_under_sanitizers(tmp_path):
    """csrc/scene_fit_rule.h and csrc/scene_fit_plan.h in a stand-alone host program built with AddressSanitizer + UBSan: the kernel's
    tiles and threads replayed on exact-size mallocs, the records of synthetic cases against numbers written into the program, the
    cover of the union of the rectangles, the multiply-and-shift tile index and the staging layout of the host entry."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "scene_fit_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "scene_fit_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "scene_fit_check: ok" in out.stdout
