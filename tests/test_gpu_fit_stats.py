"""GPU: se3tn_fit_stats (csrc/fit_stats.hip) against utils.fit_stats applied to O.crop_bbox of the same arrays.  All the statistics are
integers, so every comparison is np.array_equal: no tolerance anywhere.

Descriptors: windows of 176 px (identity), ~80 px (up-sampling) and ~300 px (down-sampling), none of them square; a window over
each frame edge, over a corner, over the whole frame, off the frame; a 1 x 1 image; model and observed images of different sizes
under different windows.  Batches of 1, 5, 6, the per-launch capacity and capacity + 1 pairs (the chunk boundary) on a context whose
max_batch just allows it.  Launches back to back on one stream, a smaller batch after a larger one and a captured, replayed launch:
where counters that were not re-armed would show.  Without the feature every case fails: the symbol does not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import se3_oracle as O

pytestmark = pytest.mark.gpu

E_ARG = -1
TOL = 6
H, W = 340, 400
WINDOWS = dict(identity=(100, 80, 276, 256), up=(150, 120, 233, 197), down=(40, 20, 345, 318), left=(-30, 100, 120, 260),
               right=(330, 50, 450, 190), top=(100, -40, 230, 100), bottom=(200, 250, 360, 420), corner=(-50, -60, 110, 90),
               whole=(-20, -50, 420, 360), miss=(500, 100, 650, 240), miss_corner=(-300, -300, -100, -120))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    e = se3.Engine(0, se3._lib.FIT_MAX_PAIRS + 1)          # max_batch just allows capacity + 1 pairs
    yield e
    e.close()


def _depth_pair(seed, h, w):
    """model / observed depth frames [h,w] uint16 in which every class of the record occurs: the model a surface around 600 mm with
    background (0) and the validity thresholds (100, 2000, 65535) sprinkled in; the observed one that surface plus -15 .. 15 mm,
    with holes, thresholds, an occluder (300 mm) and a far wall (1500 mm)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = (600 + 80 * np.sin(xx / 23.0) + 60 * np.cos(yy / 17.0) + rng.integers(-3, 4, (h, w))).astype(np.int64)
    o = m + rng.integers(-15, 16, (h, w))
    sel = rng.random((h, w))
    for k, v in enumerate((0, 100, 2000, 65535, 101, 1999)):
        m[(sel > 0.03 * k) & (sel < 0.03 * k + 0.02)] = v
    m[sel > 0.8] = 0
    sel = rng.random((h, w))
    for k, v in enumerate((0, 100, 2000, 65535, 101, 1999, 300, 1500)):
        o[(sel > 0.04 * k) & (sel < 0.04 * k + 0.03)] = v
    return m.astype(np.uint16), o.astype(np.uint16)


def crop_depth(depth, window):
    """O.crop_bbox's depth crop (Utils.py:320-359); a window that misses the image is all zeros (crop_bbox itself raises there, as
    the reference's does: its slices come out empty)"""
    l, t, r, b = window
    h, w = depth.shape
    if r <= 0 or b <= 0 or l >= w or t >= h:
        return np.zeros((176, 176), np.uint16)
    return O.crop_bbox(np.zeros((h, w, 3), np.uint8), depth, np.array([[t, l], [b, r]]))[1]


class Pairs:
    """descriptor cases: (model image, model window, observed image, observed window), device copies and the expected record"""

    def __init__(self, se3):
        self.se3 = se3
        m, o = _depth_pair(1, H, W)
        m2, o2 = _depth_pair(2, 120, 160)
        one_m, one_o = np.array([[640]], np.uint16), np.array([[644]], np.uint16)
        self.cases = [(k, m, w, o, w) for k, w in WINDOWS.items()]
        self.cases.append(("one_pixel_image", one_m, (-3, -2, 5, 6), one_o, (-3, -2, 5, 6)))
        self.cases.append(("one_pixel_observed", m, WINDOWS["up"], one_o, (0, 0, 1, 1)))
        # model and observed under different descriptors: another image size, another window, another scale
        self.cases.append(("different", m, WINDOWS["identity"], o2, (20, -10, 150, 100)))
        self.cases.append(("different_miss", m2, (10, 5, 130, 110), o, WINDOWS["miss"]))
        self._dev = {}
        self.want = {k: se3.utils.fit_stats(crop_depth(mi, mw), crop_depth(oi, ow), TOL) for k, mi, mw, oi, ow in self.cases}
        self.names = [c[0] for c in self.cases]
        self.by_name = {c[0]: c for c in self.cases}

    def dev(self, a):
        if id(a) not in self._dev:
            self._dev[id(a)] = torch.from_numpy(a.view(np.int16)).cuda()
        return self._dev[id(a)]

    def descriptors(self, names):
        model = [dict(depth=self.dev(self.by_name[k][1]), window=self.by_name[k][2]) for k in names]
        observed = [dict(depth=self.dev(self.by_name[k][3]), window=self.by_name[k][4]) for k in names]
        return model, observed

    def expected(self, names):
        out = np.zeros(len(names), self.se3._lib.FIT_DTYPE)
        for i, k in enumerate(names):
            out[i] = self.want[k]
        return out


@pytest.fixture(scope="module")
def pairs(se3):
    return Pairs(se3)


def crop_array(se3, group):
    arr = (se3._lib.Crop * len(group))()
    for i, c in enumerate(group):
        d = c["depth"]
        arr[i].rgb = None; arr[i].depth = d.data_ptr()
        arr[i].H, arr[i].W = int(d.shape[0]), int(d.shape[1])
        arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = c["window"]
    return arr


def enqueue(se3, eng, model, observed, tol, out):
    """se3tn_fit_stats on the current stream, no synchronisation; out: device uint8 [n,32]"""
    rc = eng.lib.se3tn_fit_stats(eng._h, crop_array(se3, model), crop_array(se3, observed), len(model), tol, C.c_void_p(out.data_ptr()),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.se3tn_last_error()


def records(se3, out, n):
    return out.cpu().numpy().reshape(-1).view(se3._lib.FIT_DTYPE)[:n]


def test_expected_records_cover_every_class(se3, pairs):
    """preconditions on the expected values: the cases are not vacuous"""
    w = pairs.want
    for k in ("identity", "up", "down", "left", "corner", "whole", "different"):
        assert min(int(w[k][f]) for f in ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm")) > 0, k
        assert int(w[k]["model_px"]) > int(w[k]["seen_px"])
    for k in ("miss", "miss_corner"):
        assert [int(w[k][f]) for f in se3._lib.FIT_FIELDS] == [0, 0, 0, 0, 0, 0, TOL]
    assert int(w["different_miss"]["model_px"]) > 0 and int(w["different_miss"]["seen_px"]) == 0
    assert [int(w["one_pixel_image"][f]) for f in se3._lib.FIT_FIELDS] == [484, 484, 484, 0, 0, 4 * 484, TOL]     # 1 / 64 of the crop
    assert len({tuple(int(w[k][f]) for f in se3._lib.FIT_FIELDS) for k in w if "miss" not in k}) == len(w) - 3


def test_every_descriptor_case_alone(se3, eng, pairs):
    for k in pairs.names:
        model, observed = pairs.descriptors([k])
        got = eng.fit_stats(model, observed, TOL)
        assert got.dtype == se3._lib.FIT_DTYPE and np.array_equal(got, pairs.expected([k])), (k, got, pairs.want[k])
        assert int(got["seen_px"][0]) == int(got["inlier_px"][0]) + int(got["front_px"][0]) + int(got["behind_px"][0])
    # 176 x 176 device images stand for their own whole-image descriptors; another tolerance re-classifies
    m176, o176 = _depth_pair(5, 176, 176)
    got = eng.fit_stats([torch.from_numpy(m176.view(np.int16)).cuda()], [torch.from_numpy(o176.view(np.int16)).cuda()], 11)
    assert np.array_equal(got[0], se3.utils.fit_stats(m176, o176, 11))


@pytest.mark.parametrize("n", [1, 5, 6, 32, 33])
def test_batches_up_to_the_chunk_boundary(se3, eng, pairs, n):
    assert se3._lib.FIT_MAX_PAIRS == 32 and eng.max_batch == 33
    names = [pairs.names[(3 * i + n) % len(pairs.names)] for i in range(n)]
    model, observed = pairs.descriptors(names)
    got = eng.fit_stats(model, observed, TOL)
    assert np.array_equal(got, pairs.expected(names)), n


def test_back_to_back_launches_and_a_smaller_batch_after_a_larger(se3, eng, pairs):
    """stale counters or a wrong re-arm would show here: no synchronisation between the launches"""
    big = [pairs.names[i % len(pairs.names)] for i in range(33)]
    small = ["down", "corner", "identity"]
    outs = [torch.full((33, 32), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(4)]
    mb, ob = pairs.descriptors(big)
    ms, os_ = pairs.descriptors(small)
    enqueue(se3, eng, mb, ob, TOL, outs[0])
    enqueue(se3, eng, mb, ob, TOL, outs[1])
    enqueue(se3, eng, ms, os_, TOL, outs[2])
    enqueue(se3, eng, list(reversed(mb)), list(reversed(ob)), TOL, outs[3])
    torch.cuda.synchronize()
    assert np.array_equal(records(se3, outs[0], 33), pairs.expected(big))
    assert np.array_equal(records(se3, outs[1], 33), pairs.expected(big))
    assert np.array_equal(records(se3, outs[2], 3), pairs.expected(small))
    assert (outs[2][3:].cpu().numpy() == 0xAB).all()                        # nothing past the n records is written
    assert np.array_equal(records(se3, outs[3], 33), pairs.expected(list(reversed(big))))


def test_same_records_from_a_captured_and_replayed_graph(se3, eng, pairs):
    names = [pairs.names[(5 * i) % len(pairs.names)] for i in range(33)]        # two launches inside the capture
    model, observed = pairs.descriptors(names)
    out = torch.zeros((33, 32), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue(se3, eng, model, observed, TOL, out)                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue(se3, eng, model, observed, TOL, out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(records(se3, out, 33), pairs.expected(names))
    # ... and an eager launch after the replays finds the counters armed
    assert np.array_equal(eng.fit_stats(model[:5], observed[:5], TOL), pairs.expected(names[:5]))


def test_refusals_leave_the_context_usable(se3, eng, pairs):
    lib = eng.lib
    model, observed = pairs.descriptors(["identity"] * 34)
    out = torch.zeros((34, 32), dtype=torch.uint8, device="cuda")
    m, o, p = crop_array(se3, model), crop_array(se3, observed), C.c_void_p(out.data_ptr())
    for n, tol in ((0, TOL), (34, TOL), (-1, TOL), (1, 0), (1, 65536), (1, -3)):
        assert lib.se3tn_fit_stats(eng._h, m, o, n, tol, p, None) == E_ARG, (n, tol)
    assert lib.se3tn_fit_stats(eng._h, None, o, 1, TOL, p, None) == E_ARG and lib.se3tn_fit_stats(eng._h, m, o, 1, TOL, None, None) == E_ARG
    empty = crop_array(se3, [dict(depth=model[0]["depth"], window=(10, 10, 10, 50))])
    assert lib.se3tn_fit_stats(eng._h, empty, o, 1, TOL, p, None) == E_ARG
    null = crop_array(se3, model[:1]); null[0].depth = None
    assert lib.se3tn_fit_stats(eng._h, m, null, 1, TOL, p, None) == E_ARG
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                       # a refused call writes nothing
    assert np.array_equal(eng.fit_stats(model[:1], observed[:1], 65535)[0], se3.utils.fit_stats(
        crop_depth(pairs.by_name["identity"][1], WINDOWS["identity"]), crop_depth(pairs.by_name["identity"][3], WINDOWS["identity"]), 65535))
