"""GPU: se3tn_fill_depth_rect (the fill chain up to the median as one tiled launch, then blur + invert-back + uint16 on a rectangle)
against se3tn_fill_depth on the same device, bit for bit; with blur=None against the CPU oracle too.

The frames are chosen for what a tiled version gets wrong -- positions outside the frame at every stage, not only for the input:
frames that are no multiple of the 32 x 16 tile and under two tiles in one direction, one smaller than the 11-pixel halo, holes
that reach a frame corner (the fixture's empty corner), negative inverted depth (the far wall)."""
import numpy as np
import pytest
import torch

from oracle import depth_oracle as D
from oracle.fixtures import depth_frame_with_far_wall, depth_frame_with_holes

pytestmark = pytest.mark.gpu

E_ARG = -1
BLURS = [None, "bilateral", "gaussian"]


def _tiny():
    """7 x 9, smaller than the halo: a ramp of 600-900 mm with zeros at (0, 0) and one interior pixel"""
    mm = np.linspace(600, 900, 63).reshape(7, 9).astype(np.uint16)
    mm[0, 0] = 0
    mm[3, 4] = 0
    return mm


FRAMES = {
    "holes_120x160": lambda: depth_frame_with_holes(0),
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


def rects(name):
    """(x0, y0, x1, y1): the whole frame, a block at each corner, an interior block across the tile boundaries in both directions,
    1 x 1 at both ends, a full-width row, a full-height column"""
    H, W = frame(name).shape
    bh, bw = min(H, 13), min(W, 21)
    out = [(0, 0, W, H), (0, 0, bw, bh), (W - bw, 0, W, bh), (0, H - bh, bw, H), (W - bw, H - bh, W, H),
           (27, 11, min(70, W - 1), min(37, H - 1)) if W > 29 and H > 13 else (1, 1, W - 1, H - 1),
           (0, 0, 1, 1), (W - 1, H - 1, W, H), (0, H // 2, W, H // 2 + 1), (W // 2, 0, W // 2 + 1, H)]
    if name == "far_wall_240x320":
        out.append((190, 90, 230, 120))   # straddles the rim of the wall at rows 100-140, cols 200-260
    return out


@pytest.fixture(scope="module")
def eng():
    import se3tracknet_amd as se3
    return se3.Engine(0, 1)


def assert_not_degenerate(name):
    """more than half of the frame's filled pixels are valid (an all-empty frame would pass everything below vacuously)"""
    out = oracle_no_blur(name)
    valid = (out > 100) & (out < 2000)
    assert valid.mean() > 0.5, (name, valid.mean())


@pytest.mark.parametrize("blur", BLURS, ids=[str(b) for b in BLURS])
@pytest.mark.parametrize("name", list(FRAMES))
def test_rect_equals_full_chain(eng, name, blur):
    assert_not_degenerate(name)
    mm = frame(name)
    want = eng.fill_depth(mm, 2.0, False, blur)
    if blur is None:
        assert np.array_equal(want, oracle_no_blur(name))
    for x0, y0, x1, y1 in rects(name):
        got = eng.fill_depth_rect(mm, (x0, y0, x1, y1), 2.0, False, blur)
        assert got.shape == (y1 - y0, x1 - x0) and got.dtype == np.uint16
        assert np.array_equal(got, want[y0:y1, x0:x1]), (name, blur, (x0, y0, x1, y1))
        if blur is None:
            assert np.array_equal(got, oracle_no_blur(name)[y0:y1, x0:x1])


@pytest.mark.parametrize("blur", [None, "bilateral"], ids=["None", "bilateral"])
def test_rect_with_extrapolate(eng, blur):
    name = "holes_120x160"
    mm = frame(name)
    want = eng.fill_depth(mm, 2.0, True, blur)
    for x0, y0, x1, y1 in rects(name):
        got = eng.fill_depth_rect(mm, (x0, y0, x1, y1), 2.0, True, blur)
        assert np.array_equal(got, want[y0:y1, x0:x1]), (x0, y0, x1, y1)
        if blur is None:
            assert np.array_equal(got, oracle_no_blur(name, True)[y0:y1, x0:x1])


def test_device_tensor_in_and_out(eng):
    mm = frame("holes_33x95")
    t = torch.from_numpy(mm.view(np.int16).copy()).cuda()
    for blur in BLURS:
        out = eng.fill_depth_rect(t, (5, 3, 90, 30), 2.0, False, blur)
        assert out.is_cuda and tuple(out.shape) == (27, 85)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), eng.fill_depth(mm, 2.0, False, blur)[3:30, 5:90])


def test_second_call_does_not_see_the_first_call_s_range(eng):
    """the far wall's range (negative inverted depth) must not survive in the min / max words into the next frame's table"""
    a, b = frame("far_wall_240x320"), frame("holes_120x160")
    want_a, want_b = eng.fill_depth(a, 2.0, False, "bilateral"), eng.fill_depth(b, 2.0, False, "bilateral")
    assert np.array_equal(eng.fill_depth_rect(a, (180, 80, 280, 160)), want_a[80:160, 180:280])
    assert np.array_equal(eng.fill_depth_rect(b, (10, 20, 150, 100)), want_b[20:100, 10:150])
    assert np.array_equal(eng.fill_depth_rect(b, (100, 5, 160, 47)), want_b[5:47, 100:160])
    assert np.array_equal(eng.fill_depth_rect(a, (0, 0, 320, 240)), want_a)


def test_capturable_after_reserve(eng):
    eng.reserve(240, 320)
    mm = frame("far_wall_240x320")
    rect = (150, 70, 300, 200)
    want = eng.fill_depth(mm, 2.0, False, "bilateral")[70:200, 150:300]
    src = torch.from_numpy(mm.view(np.int16).copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.fill_depth_rect(src, rect)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = eng.fill_depth_rect(src, rect)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)


def test_refusals_leave_the_context_usable(eng):
    import se3tracknet_amd as se3
    mm = frame("holes_37x53")
    want = eng.fill_depth(mm, 2.0, False, "bilateral")
    for rect, blur in (((10, 10, 10, 20), "bilateral"), ((10, 20, 30, 20), "bilateral"), ((30, 10, 20, 20), "bilateral"),
                       ((0, 0, 54, 37), "bilateral"), ((0, 0, 53, 38), "bilateral"), ((-1, 0, 5, 5), "bilateral"), ((0, 0, 5, 5), 7)):
        with pytest.raises(se3._lib.Se3tnError, match=r"rc=%d" % E_ARG):
            eng.fill_depth_rect(mm, rect, 2.0, False, blur)
        assert np.array_equal(eng.fill_depth_rect(mm, (3, 2, 50, 35)), want[2:35, 3:50])
