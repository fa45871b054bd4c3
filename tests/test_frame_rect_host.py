"""CPU: se3tn_frame_rect -- the rectangle of the camera frame the full-frame (pyrender) route of se3tn_on_track renders -- against
the oracle's compute_bbox clipped to the frame in numpy, and the presence of the route's symbols in header and ctypes table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import se3_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("se3tn_render_frame_rect", "se3tn_mesh_set_route", "se3tn_mesh_get_route", "se3tn_frame_rect")


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def _want(P, K, width, H, W):
    """crop window of predict.py:231-235 (min / max of compute_bbox's corners) intersected with the frame; None: they do not meet"""
    bb = O.compute_bbox(P, K, width, (1000, 1000, 1000))
    left, top, right, bottom = int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())
    x0, y0, x1, y1 = max(left, 0), max(top, 0), min(right, W), min(bottom, H)
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


def test_frame_rect_vs_oracle_bbox_clipped_to_the_frame(se3):
    rng = np.random.default_rng(11)
    H, W = 480, 640
    kinds = dict(inside=0, left=0, right=0, top=0, bottom=0, miss=0, larger=0)
    cases = [(Fx.pose(i, (rng.uniform(-0.6, 0.6), rng.uniform(-0.45, 0.45), rng.uniform(0.25, 2.0))), float(rng.uniform(80, 400)))
             for i in range(400)]
    # one of every kind for certain (YCB camera, 150 mm): inside, over each border, off the frame, larger than the frame
    cases += [(Fx.pose(1, t), 150.0) for t in ((0.0, 0.0, 0.7), (-0.18, 0.0, 0.7), (0.2, 0.0, 0.7), (0.0, -0.13, 0.7), (0.0, 0.14, 0.7),
                                               (0.6, 0.5, 0.9), (0.0, 0.0, 0.3))]
    for i, (P, w) in enumerate(cases):
        got = se3.frame_rect(P, Fx.K_YCB, w, H, W)
        want = _want(P, Fx.K_YCB, w, H, W)
        assert got == want, (i, got, want)
        bb = O.compute_bbox(P, Fx.K_YCB, w, (1000, 1000, 1000))
        left, top, right, bottom = bb[:, 1].min(), bb[:, 0].min(), bb[:, 1].max(), bb[:, 0].max()
        if want is None:
            kinds["miss"] += 1
            continue
        kinds["left"] += left < 0; kinds["right"] += right > W; kinds["top"] += top < 0; kinds["bottom"] += bottom > H
        kinds["inside"] += left >= 0 and top >= 0 and right <= W and bottom <= H
        kinds["larger"] += top < 0 and bottom > H
    assert all(v > 0 for v in kinds.values()), kinds
    # another frame size, and the raw entry point: a miss is the empty rectangle with return value 0
    lib = se3._lib.load()
    K = np.ascontiguousarray(Fx.K_YCB)
    r = (C.c_int32 * 4)(7, 7, 7, 7)
    P = np.ascontiguousarray(Fx.pose(2, (0.6, 0.5, 0.9)))
    rc = lib.se3tn_frame_rect(P.ctypes.data_as(C.POINTER(C.c_double)), K.ctypes.data_as(C.POINTER(C.c_double)), 150.0, 480, 640, r)
    assert rc == 0 and list(r) == [0, 0, 0, 0]
    for i in range(50):
        P = Fx.pose(i, (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.3, 1.0)))
        assert se3.frame_rect(P, Fx.K_YCB, 200.0, 97, 131) == _want(P, Fx.K_YCB, 200.0, 97, 131)


def test_frame_rect_refuses_poses_without_a_window(se3):
    lib = se3._lib.load()
    K = np.ascontiguousarray(Fx.K_YCB)
    pk = K.ctypes.data_as(C.POINTER(C.c_double))
    r = (C.c_int32 * 4)()

    def rc_of(P, width=150.0, H=480, W=640):
        P = np.ascontiguousarray(P, np.float64)
        return lib.se3tn_frame_rect(P.ctypes.data_as(C.POINTER(C.c_double)), pk, width, H, W, r)
    good = Fx.pose(3, (0.0, 0.0, 0.7))
    assert rc_of(good) == 0
    for bad in (0.0, -0.5, np.nan, np.inf, -np.inf):
        P = good.copy(); P[2, 3] = bad
        assert rc_of(P) == -1, bad                        # SE3TN_E_ARG
        assert b"se3tn_frame_rect" in lib.se3tn_last_error()
    for k in (0, 1):
        for bad in (np.nan, np.inf):
            P = good.copy(); P[k, 3] = bad
            assert rc_of(P) == -1, (k, bad)
    assert rc_of(good, width=0.0) == -1 and rc_of(good, H=0) == -1 and rc_of(good, W=0) == -1
    assert lib.se3tn_frame_rect(None, pk, 150.0, 480, 640, r) == -1
    with pytest.raises(se3._lib.Se3tnError):
        se3.frame_rect(np.zeros((4, 4)), Fx.K_YCB, 150.0, 480, 640)
    assert rc_of(good) == 0


def test_frame_route_symbols_in_header_library_and_ctypes(se3):
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    lib = C.CDLL(se3._lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in se3._lib.exported_symbols(), name
    assert (int(re.search(r"#define SE3TN_ROUTE_WINDOW (\d+)", hdr).group(1)), int(re.search(r"#define SE3TN_ROUTE_FRAME (\d+)", hdr).group(1))) == \
        (se3._lib.ROUTE_WINDOW, se3._lib.ROUTE_FRAME) == (0, 1)
    # route selector on no mesh: refused, no crash (a mesh needs a device: tests/test_gpu_frame_route.py)
    L = se3._lib.load()
    assert L.se3tn_mesh_get_route(None) == -1 and L.se3tn_mesh_set_route(None, 1) == -1
