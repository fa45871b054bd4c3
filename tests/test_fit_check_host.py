"""CPU: the host side of the fit check -- utils.fit_stats (the NumPy statement of se3tn_fit_stats) against counts written out by
hand, the refusals of the five C entry points that need no device, and the fit-driven re-initialisation of
sequence.predict_sequence_ycb on the synthetic YCB tree with a replaying stand-in whose last_fit_ratio follows a script.
Every case fails without the feature: the function, the symbols and the keyword do not exist."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ycbv_fixtures as YF

E_ARG, E_STATE = -1, -2
TOL = 7


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def literal_pair():
    """176 x 176 pair, every class of pixel present.  Row by row (176 pixels each unless a slice is given):
      0      model 0 (no model)                     observed 500
      1      model 100, 2000 (88 each: invalid)     observed 500
      2      model 65535 (invalid)                  observed 500
      3      model 500, observed 0 | 100 | 2000 | 65535 (44 each: invalid observed)      -> model only
      4      model 500, observed 500 + TOL                                               -> inlier, |d| = TOL
      5      model 500, observed 500 - TOL                                               -> inlier, |d| = TOL
      6      model 500, observed 500 (first 100 pixels), 499 (the other 76)              -> inlier, |d| = 0 | 1
      7      model 500, observed 500 - TOL - 1                                           -> front
      8      model 500, observed 500 + TOL + 1 (first 50 pixels), 1999 (the other 126)   -> behind
      9      model 101 (just valid), observed 1999 (just valid)                          -> behind
      10     model 1999, observed 101                                                    -> front
    everything else 0 / 0."""
    m = np.zeros((176, 176), np.uint16)
    o = np.zeros((176, 176), np.uint16)
    o[0] = 500
    m[1, :88], m[1, 88:], o[1] = 100, 2000, 500
    m[2], o[2] = 65535, 500
    m[3] = 500
    o[3, :44], o[3, 44:88], o[3, 88:132], o[3, 132:] = 0, 100, 2000, 65535
    m[4], o[4] = 500, 500 + TOL
    m[5], o[5] = 500, 500 - TOL
    m[6], o[6, :100], o[6, 100:] = 500, 500, 499
    m[7], o[7] = 500, 500 - TOL - 1
    m[8], o[8, :50], o[8, 50:] = 500, 500 + TOL + 1, 1999
    m[9], o[9] = 101, 1999
    m[10], o[10] = 1999, 101
    return m, o


LITERAL = dict(model_px=8 * 176, seen_px=7 * 176, inlier_px=3 * 176, front_px=2 * 176, behind_px=2 * 176,
               sum_abs_mm=2 * 176 * TOL + 76, tol_mm=TOL)


def test_fit_stats_numpy_against_literal_counts(se3):
    m, o = literal_pair()
    rec = se3.utils.fit_stats(m, o, TOL)
    assert rec.shape == () and rec.dtype == se3._lib.FIT_DTYPE
    assert {k: int(rec[k]) for k in se3._lib.FIT_FIELDS} == LITERAL
    assert int(rec["seen_px"]) == int(rec["inlier_px"]) + int(rec["front_px"]) + int(rec["behind_px"])
    assert int(rec["_reserved"]) == 0
    assert se3.utils.fit_ratio(rec) == 3 / 8
    # a wider tolerance moves pixels between the classes, never in or out of `seen`: rows 7 and the first 50 of row 8 become inliers
    wide = se3.utils.fit_stats(m, o, TOL + 1)
    assert (int(wide["model_px"]), int(wide["seen_px"])) == (LITERAL["model_px"], LITERAL["seen_px"])
    assert (int(wide["inlier_px"]), int(wide["front_px"]), int(wide["behind_px"])) == (4 * 176 + 50, 176, 126 + 176)
    assert int(wide["sum_abs_mm"]) == LITERAL["sum_abs_mm"] + (176 + 50) * (TOL + 1)
    # a stack of pairs: one record each; an empty model: ratio 0.0, not a division by zero
    both = se3.utils.fit_stats(np.stack([m, np.zeros_like(m)]), np.stack([o, o]), TOL)
    assert both.shape == (2,) and {k: int(both[0][k]) for k in se3._lib.FIT_FIELDS} == LITERAL
    assert [int(both[1][k]) for k in se3._lib.FIT_FIELDS] == [0, 0, 0, 0, 0, 0, TOL]
    assert se3.utils.fit_ratio(both).tolist() == [3 / 8, 0.0]
    # the largest sum the record can hold stays inside uint32: every pixel an inlier at the largest distance two valid depths have
    far = se3.utils.fit_stats(np.full((176, 176), 101, np.uint16), np.full((176, 176), 1999, np.uint16), 65535)
    assert int(far["sum_abs_mm"]) == 176 * 176 * 1898 and int(far["inlier_px"]) == 176 * 176


def test_fit_entry_points_refuse_without_a_device(se3):
    lib = se3._lib.load()
    L = se3._lib
    assert C.sizeof(L.Fit) == 32 and L.FIT_DTYPE.itemsize == 32
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "se3tracknet.h")).read()
    import re
    assert int(re.search(r"#define SE3TN_FIT_MAX_PAIRS (\d+)", hdr).group(1)) == L.FIT_MAX_PAIRS
    crops = (L.Crop * 1)()
    out = (L.Fit * 1)()
    # NULL context
    assert lib.se3tn_fit_stats(None, crops, crops, 1, 5, C.byref(out), None) == E_ARG
    assert lib.se3tn_set_fit_check(None, 5) == E_ARG and lib.se3tn_get_fit_check(None) == -1
    assert lib.se3tn_last_fit(None, 1, C.byref(out)) == E_ARG
    assert lib.se3tn_last_fit_images(None, None, None) == E_ARG
    # a host-only context: the switch is plain state; the compute call refuses; no tracking call has left records
    eng = se3.Engine(device=-1, max_batch=2)
    assert eng.get_fit_check() is None and lib.se3tn_get_fit_check(eng._h) == 0
    for bad in (-1, 65536):
        assert lib.se3tn_set_fit_check(eng._h, bad) == E_ARG
    assert eng.get_fit_check() is None
    eng.set_fit_check(12)
    assert eng.get_fit_check() == 12
    eng.set_fit_check(65535)
    assert eng.get_fit_check() == 65535
    eng.set_fit_check(None)
    assert eng.get_fit_check() is None
    assert lib.se3tn_fit_stats(eng._h, crops, crops, 1, 5, C.byref(out), None) == E_ARG and b"se3tn_fit_stats" in lib.se3tn_last_error()
    assert lib.se3tn_last_fit(eng._h, 1, C.byref(out)) == E_STATE
    assert lib.se3tn_last_fit(eng._h, 0, C.byref(out)) == E_ARG and lib.se3tn_last_fit(eng._h, 1, None) == E_ARG
    p = C.c_void_p()
    assert lib.se3tn_last_fit_images(eng._h, C.byref(p), None) == E_STATE and p.value is None
    with pytest.raises(L.Se3tnError):
        eng.last_fit(1)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return YF.make_tree(str(tmp_path_factory.mktemp("ycbv_fit")))


@pytest.fixture(scope="module")
def seq():
    import importlib
    return importlib.import_module("iros20-6d-pose-tracking_amd.sequence")


class ScriptedTracker:
    """stands where the Tracker stands: answers with scripted poses, reports a scripted fit ratio after every call"""
    object_cloud = None

    def __init__(self, poses_out, ratios, fit_check=20):
        self.out, self.ratios, self.fit_check = poses_out, ratios, fit_check
        self.fed, self.k, self.last_fit_ratio = [], 0, None

    def on_track(self, prev_pose, rgb, depth, **kw):
        self.fed.append(np.array(prev_pose))
        self.last_fit_ratio = self.ratios[self.k]
        self.k += 1
        return self.out[self.k - 1].copy()


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_reinit_below_follows_the_scripted_fit(tree, seq, tmp_path):
    seq_dir = os.path.join(tree, "data_organized", "0048")
    n = 8                                                        # 9 frames: image indices 1 .. 8 are tracked
    rng = np.random.default_rng(3)
    poses = [YF.gt_pose(48, i + 1) + np.pad(rng.normal(0, 1e-3, (3, 4)), ((0, 1), (0, 0))) for i in range(n)]
    #          call for image index:  1     2     3     4     5     6     7     8
    ratios = [0.9, 0.2, 0.8, 0.5, 0.1, 0.05, 0.7, 0.0]           # below 0.5 after the calls for 2, 5, 6 (and 8: nothing follows)
    trk = ScriptedTracker(poses, ratios)
    out = str(tmp_path / "fit")
    res = seq.predict_sequence_ycb(trk, seq_dir, YF.CLASS_ID, out, ycb_dir=tree, reinit_below=0.5)
    assert res["reinit_at"] == [3, 6, 7] and res["frames"] == n
    fed = trk.fed
    assert np.array_equal(fed[0], np.loadtxt(os.path.join(seq_dir, "pose_gt", str(YF.CLASS_ID), "000001.txt")))
    for k in range(1, n):
        i = k + 1                                                # the image index this call tracked
        if i in (3, 6, 7):   # the reference's rule for a listed frame: PoseCNN nearest to frame NUMBER i - 1 (predict.py:538-541)
            assert np.array_equal(fed[k], seq.use_posecnn_res(tree, YF.CLASS_ID, "0048/%06d" % (i - 1))), i
            assert np.abs(fed[k] - poses[k - 1]).max() > 1e-3
        else:
            assert np.array_equal(fed[k], poses[k - 1]), i       # pose feedback (0.5 itself is not below 0.5: index 5)
    # the ratio alone decides: no threshold, no re-initialisation, and then the files are byte for byte those of today's signature;
    # a tracker with the check off is never re-initialised either, whatever the threshold
    runs = {}
    for name, kw, fit_check in (("today", {}, 20), ("none", dict(reinit_below=None), 20), ("check_off", dict(reinit_below=0.5), None)):
        t = ScriptedTracker(poses, ratios, fit_check)
        d = str(tmp_path / name)
        r = seq.predict_sequence_ycb(t, seq_dir, YF.CLASS_ID, d, ycb_dir=tree, **kw)
        runs[name] = (_files(d), r, t)
        for k in range(1, n):
            assert np.array_equal(t.fed[k], poses[k - 1])
    assert runs["today"][0] == runs["none"][0] == runs["check_off"][0] and len(runs["today"][0]) == 2 * (n + 1)
    assert "reinit_at" not in runs["today"][1] and "reinit_at" not in runs["none"][1] and runs["check_off"][1]["reinit_at"] == []
    assert _files(out) == runs["today"][0]                       # (the written poses are the scripted answers either way)
    # the fit-driven list and the reference's list compose: a listed frame is re-initialised whatever its fit
    t = ScriptedTracker(poses, [1.0] * n)
    r = seq.predict_sequence_ycb(t, seq_dir, YF.CLASS_ID, str(tmp_path / "both"), ycb_dir=tree, reinit_frames=YF.REINIT_FRAMES,
                                 reinit_below=0.5)
    assert r["reinit_at"] == []
    assert np.array_equal(t.fed[3], seq.use_posecnn_res(tree, YF.CLASS_ID, "0048/%06d" % 3))     # 0048/000005 = index 4, listed
