"""GPU: se3tn_fill_depth_rects (the fill chain once per frame, then blur + invert-back + uint16 for a TABLE of rectangles in one launch
per 64) against se3tn_fill_depth on the same device, bit for bit; with blur=None against the CPU oracle too.

Every value depends on the whole frame only, so a rectangle's bytes must not depend on its company: the one call of these tests
holds overlapping rectangles, the same rectangle twice and an empty one, and is repeated in reverse order.  The frames are those a
tiled chain gets wrong (no multiple of the 32 x 16 tile, under two tiles in one direction, smaller than the 11-pixel halo, negative
inverted depth)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import depth_oracle as D
from oracle.fixtures import depth_frame_with_far_wall, depth_frame_with_holes

pytestmark = pytest.mark.gpu

E_ARG = -1
BLURS = [None, "bilateral", "gaussian"]
BLUR_ID = {None: 0, "bilateral": 1, "gaussian": 2}


def _tiny():
    """7 x 9, smaller than the halo: a ramp of 600-900 mm with zeros at (0, 0) and one interior pixel"""
    mm = np.linspace(600, 900, 63).reshape(7, 9).astype(np.uint16)
    mm[0, 0] = 0
    mm[3, 4] = 0
    return mm


FRAMES = {
    "holes_37x53": lambda: depth_frame_with_holes(1, 37, 53),
    "holes_33x95": lambda: depth_frame_with_holes(2, 33, 95),
    "far_wall_240x320": lambda: depth_frame_with_far_wall(7),
    "tiny_7x9": _tiny,
}
_cache = {}


def frame(name):
    if name not in _cache:
        _cache[name] = FRAMES[name]()
    return _cache[name]


def oracle_no_blur(name, extrapolate=False):
    key = (name, "oracle", extrapolate)
    if key not in _cache:
        out = D.grab_depth(frame(name), 2.0, extrapolate, None)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    import se3tracknet_amd as se3
    return se3.Engine(0, 1)


def full(eng, name, extrapolate, blur):
    """Engine.fill_depth of the frame, once per (frame, extrapolate, blur)"""
    key = (name, "full", extrapolate, blur)
    if key not in _cache:
        out = eng.fill_depth(frame(name), 2.0, extrapolate, blur)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def rects(name):
    """(x0, y0, x1, y1) of ONE call: the whole frame, the four corner blocks, a block across the tile seams in both directions, 1 x 1
    at both ends, an EMPTY rectangle, a full-width row, a full-height column, two overlapping rectangles, the same rectangle twice"""
    H, W = frame(name).shape
    bh, bw = min(H, 13), min(W, 21)
    seam = (27, 11, min(70, W - 1), min(37, H - 1)) if W > 29 and H > 13 else (1, 1, W - 1, H - 1)
    return [(0, 0, W, H), (0, 0, bw, bh), (W - bw, 0, W, bh), (0, H - bh, bw, H), (W - bw, H - bh, W, H), seam,
            (0, 0, 1, 1), (W - 1, H - 1, W, H), (0, 0, 0, 0), (0, H // 2, W, H // 2 + 1), (W // 2, 0, W // 2 + 1, H),
            (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2), (W // 3, H // 3, W, H),     # these two overlap
            seam, (0, 0, bw, bh)]                                                         # ... and these repeat earlier ones


def assert_not_degenerate(name):
    """more than half of the frame's filled pixels are valid (an all-empty frame would pass everything below vacuously)"""
    out = oracle_no_blur(name)
    valid = (out > 100) & (out < 2000)
    assert valid.mean() > 0.5, (name, valid.mean())


def check_call(eng, name, rs, extrapolate, blur):
    want = full(eng, name, extrapolate, blur)
    got = eng.fill_depth_rects(frame(name), rs, 2.0, extrapolate, blur)
    assert len(got) == len(rs)
    for (x0, y0, x1, y1), g in zip(rs, got):
        assert g.dtype == np.uint16 and g.shape == (max(y1 - y0, 0), max(x1 - x0, 0))
        assert np.array_equal(g, want[y0:y1, x0:x1]), (name, blur, extrapolate, (x0, y0, x1, y1))
        if blur is None:
            assert np.array_equal(g, oracle_no_blur(name, extrapolate)[y0:y1, x0:x1])
    return got


@pytest.mark.parametrize("extrapolate", [False, True], ids=["plain", "extrapolate"])
@pytest.mark.parametrize("blur", BLURS, ids=[str(b) for b in BLURS])
@pytest.mark.parametrize("name", list(FRAMES))
def test_every_rectangle_of_one_call_equals_the_full_chain(eng, name, blur, extrapolate):
    assert_not_degenerate(name)
    if blur is None:
        assert np.array_equal(full(eng, name, extrapolate, blur), oracle_no_blur(name, extrapolate))
    rs = rects(name)
    got = check_call(eng, name, rs, extrapolate, blur)
    back = check_call(eng, name, rs[::-1], extrapolate, blur)           # the same list reversed: the same bytes per rectangle
    for a, b in zip(got, back[::-1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("blur", BLURS, ids=[str(b) for b in BLURS])
def test_seventy_rows_make_two_chunks_of_kernel_arguments(eng, blur):
    name = "holes_37x53"
    H, W = frame(name).shape
    rs = [(0, i % H, W, i % H + 1) for i in range(70)]
    check_call(eng, name, rs, False, blur)


def raw_call(eng, mm_dev, H, W, blur, rs, offs, out):
    """se3tn_fill_depth_rects as the header declares it (host tables, device base pointer)"""
    r = np.ascontiguousarray(np.asarray(rs, np.int32).reshape(-1, 4))
    o = np.ascontiguousarray(np.asarray(offs, np.uintp))
    return eng.lib.se3tn_fill_depth_rects(eng._h, C.c_void_p(mm_dev.data_ptr()), H, W, 2.0, 0, blur, len(rs),
                                          r.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_size_t)),
                                          C.c_void_p(out.data_ptr()), None)


@pytest.mark.parametrize("name", ["holes_37x53", "far_wall_240x320"])
def test_a_guard_element_between_the_outputs_is_untouched(eng, name):
    """the grid is sized by the largest rectangle of the launch: threads past a small rectangle's area must not write"""
    mm = frame(name)
    H, W = mm.shape
    rs = [r for r in rects(name)]
    offs, total = [], 1
    for x0, y0, x1, y1 in rs:                      # guard | rect 0 | guard | rect 1 | ... | guard
        offs.append(total)
        total += max(x1 - x0, 0) * max(y1 - y0, 0) + 1
    GUARD = 0x5A5A
    src = torch.from_numpy(mm.view(np.int16).copy()).cuda()
    for blur in BLURS:
        want = full(eng, name, False, blur)
        out = torch.full((total,), GUARD, dtype=torch.int16, device="cuda")
        assert raw_call(eng, src, H, W, BLUR_ID[blur], rs, offs, out) == 0
        torch.cuda.synchronize()
        flat = out.cpu().numpy().view(np.uint16)
        assert flat[0] == GUARD
        for (x0, y0, x1, y1), o in zip(rs, offs):
            n = max(x1 - x0, 0) * max(y1 - y0, 0)
            assert np.array_equal(flat[o:o + n].reshape(max(y1 - y0, 0), max(x1 - x0, 0)), want[y0:y1, x0:x1]), (blur, (x0, y0, x1, y1))
            assert flat[o + n] == GUARD, (blur, (x0, y0, x1, y1))


def test_all_rectangles_empty_enqueues_nothing(eng):
    mm = frame("holes_37x53")
    src = torch.from_numpy(mm.view(np.int16).copy()).cuda()
    out = torch.full((8,), 0x5A5A, dtype=torch.int16, device="cuda")
    assert raw_call(eng, src, 37, 53, 1, [(0, 0, 0, 0), (5, 5, 5, 9), (9, 4, 3, 8)], [0, 2, 4], out) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all()
    assert [g.shape for g in eng.fill_depth_rects(mm, [(0, 0, 0, 0), (4, 4, 2, 9)])] == [(0, 0), (0, 0)]


def test_device_tensor_in_and_out(eng):
    name = "holes_33x95"
    t = torch.from_numpy(frame(name).view(np.int16).copy()).cuda()
    for blur in BLURS:
        a, b = eng.fill_depth_rects(t, [(5, 3, 90, 30), (0, 0, 95, 33)], 2.0, False, blur)
        assert a.is_cuda and tuple(a.shape) == (27, 85) and tuple(b.shape) == (33, 95)
        assert np.array_equal(a.cpu().numpy().view(np.uint16), full(eng, name, False, blur)[3:30, 5:90])
        assert np.array_equal(b.cpu().numpy().view(np.uint16), full(eng, name, False, blur))


def test_capturable_after_reserve(eng):
    eng.reserve(240, 320)
    name = "far_wall_240x320"
    rs = [(150, 70, 300, 200), (0, 0, 0, 0), (190, 90, 230, 120)]
    src = torch.from_numpy(frame(name).view(np.int16).copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.fill_depth_rects(src, rs)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        outs = eng.fill_depth_rects(src, rs)
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = full(eng, name, False, "bilateral")
    for (x0, y0, x1, y1), o in zip(rs, outs):
        assert np.array_equal(o.cpu().numpy().view(np.uint16), want[y0:y1, x0:x1])


def test_refusals_leave_the_context_usable(eng):
    import se3tracknet_amd as se3
    name = "holes_37x53"
    mm = frame(name)
    want = full(eng, name, False, "bilateral")
    good = [(3, 2, 50, 35), (0, 0, 0, 0), (10, 10, 20, 30)]
    src = torch.from_numpy(mm.view(np.int16).copy()).cuda()
    out = torch.zeros((4096,), dtype=torch.int16, device="cuda")

    def good_call_is_right():
        for (x0, y0, x1, y1), g in zip(good, eng.fill_depth_rects(mm, good)):
            assert np.array_equal(g, want[y0:y1, x0:x1])

    # a rectangle that is not empty and not inside the frame, first / in the middle / last
    for bad in ((0, 0, 54, 37), (0, 0, 53, 38), (-1, 0, 5, 5), (50, 30, 60, 36)):
        for at in (0, 1, 3):
            rs = list(good)
            rs.insert(at, bad)
            with pytest.raises(se3._lib.Se3tnError, match=r"rc=%d" % E_ARG):
                eng.fill_depth_rects(mm, rs)
        good_call_is_right()
    assert raw_call(eng, src, 37, 53, 1, [], [], out) == E_ARG                       # n = 0
    good_call_is_right()
    with pytest.raises(se3._lib.Se3tnError, match=r"rc=%d" % E_ARG):
        eng.fill_depth_rects(mm, good, 2.0, False, 7)                                # blur 7
    good_call_is_right()
    lib = eng.lib                                                                    # NULL pointers
    r = (C.c_int32 * 4)(0, 0, 5, 5)
    o = (C.c_size_t * 1)(0)
    assert lib.se3tn_fill_depth_rects(eng._h, None, 37, 53, 2.0, 0, 1, 1, r, o, C.c_void_p(out.data_ptr()), None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, C.c_void_p(src.data_ptr()), 37, 53, 2.0, 0, 1, 1, None, o, C.c_void_p(out.data_ptr()), None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, C.c_void_p(src.data_ptr()), 37, 53, 2.0, 0, 1, 1, r, None, C.c_void_p(out.data_ptr()), None) == E_ARG
    assert lib.se3tn_fill_depth_rects(eng._h, C.c_void_p(src.data_ptr()), 37, 53, 2.0, 0, 1, 1, r, o, None, None) == E_ARG
    good_call_is_right()
