"""CPU: the host side of the live-camera call for several objects -- se3tn_fill_depth_rects and se3tn_on_track_objects_live exist, are in
the ctypes table and refuse a host-only context and NULL arguments without crashing; the staging layout of csrc/track_plan.h
(plan_live, the BGR swap of stage_window, crop_pair on the layout) holds under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def test_entry_points_exist_and_are_in_the_ctypes_table(se3):
    raw = C.CDLL(se3._lib.LIB_PATH)
    for name in ("se3tn_fill_depth_rects", "se3tn_on_track_objects_live"):
        assert hasattr(raw, name), name
        assert name in se3._lib.exported_symbols()
        assert getattr(se3._lib.load(), name).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    assert "int se3tn_fill_depth_rects(" in hdr and "int se3tn_on_track_objects_live(" in hdr
    assert hasattr(se3.Engine, "fill_depth_rects") and hasattr(se3.MultiTracker, "on_track_live")
    assert hasattr(se3, "LiveMultiTracker") and "LiveMultiTracker" in se3.package.__all__


def test_fill_depth_rects_refuses_a_host_only_context_and_null_arguments(se3):
    lib = se3._lib.load()
    eng = se3.Engine(device=-1, max_batch=1)
    rects = (C.c_int32 * 8)(0, 0, 4, 4, 1, 1, 3, 3)
    offs = (C.c_size_t * 2)(0, 16)
    p = C.c_void_p(64)     # (never dereferenced: every call below is refused before any work)
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 1, 2, rects, offs, p, None) == E_ARG      # host-only context
    assert b"se3tn_fill_depth_rects" in lib.se3tn_last_error()
    assert lib.se3tn_fill_depth_rects(None, p, 8, 8, 2.0, 0, 1, 2, rects, offs, p, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, None, 8, 8, 2.0, 0, 1, 2, rects, offs, p, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 1, 2, None, offs, p, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 1, 2, rects, None, p, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 1, 2, rects, offs, None, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 1, 0, rects, offs, p, None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, p, 8, 8, 2.0, 0, 7, 2, rects, offs, p, None) == E_ARG
    eng.close()


def test_on_track_objects_live_refuses_a_host_only_context_and_null_arguments(se3):
    lib = se3._lib.load()
    eng = se3.Engine(device=-1, max_batch=2)
    H, W = 6, 8
    objs = (se3._lib.Object * 1)(se3._lib.Object(eng._h.value, None, 100.0))
    P = np.eye(4)
    P[2, 3] = 0.5
    K = np.ascontiguousarray(np.array([[100.0, 0, 4], [0, 100.0, 3], [0, 0, 1]]))
    color, raw, out = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16), np.zeros(16)
    v = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    Kp = K.ctypes.data_as(C.POINTER(C.c_double))

    def call(ctx=eng._h, n=1, objects=objs, poses=v(P), Kc=Kp, col=v(color), order=1, dep=v(raw), pose_out=v(out), blur=1):
        return lib.se3tn_on_track_objects_live(ctx, n, objects, poses, Kc, col, order, dep, H, W, 2.0, 0, blur, None, None, None,
                                               pose_out, None, None, None, None)

    assert call() == E_ARG                          # host-only context
    assert b"se3tn_on_track_objects_live" in lib.se3tn_last_error()
    assert call(ctx=None) == E_ARG
    assert call(objects=None) == E_ARG
    assert call(poses=None) == E_ARG
    assert call(Kc=None) == E_ARG
    assert call(col=None) == E_ARG
    assert call(dep=None) == E_ARG
    assert call(pose_out=None) == E_ARG
    assert call(n=0) == E_ARG
    assert call(order=2) == E_ARG and call(blur=7) == E_ARG
    eng.close()


def test_live_layout_host_arithmetic_under_sanitizers(tmp_path):
    """csrc/track_plan.h's live layout in a stand-alone host program built with AddressSanitizer + UBSan: regions disjoint, aligned
    and inside the planned size; the BGR swap writes exactly its regions of a buffer of exactly the planned bytes; crop_pair on
    the layout = the non-live descriptors, shifted."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "live_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "live_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "live_plan_check: ok" in out.stdout
