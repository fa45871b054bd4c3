"""The depth frames of oracle/fixtures.py that are built to break the fill chain (thresholds on both sides of the inversion, a
max_depth that is no float32, constant / one-millimetre / 65-metre ranges for the bilateral table, every kind of column for the
extrapolation, frames smaller than the kernels and around the 256-thread and 32 x 16 tile sizes, plateaus that put the median
on a step) on the CPU: every family provably reaches the branch it names, the oracle's morphology and median equal scipy.ndimage
bit for bit on them, and its two float32 blurs are held per pixel to float64 evaluations of the same rules.  The per-pixel distances
float32 oracle - float64 found here are what tests/test_gpu_fill_depth_hard_frames.py bounds the HIP kernels with; that file
calls the proofs below before it trusts a frame."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import depth_oracle as D
from oracle import fixtures as Fx

f32, f64 = np.float32, np.float64
T = f32(0.1)                      # the threshold of every comparison of the chain, as float32 (NumPy compares a float32 image so)
EPS = float(np.finfo(f32).eps)
BIL_BINS = 1 << 12
BLURS = [None, "bilateral", "gaussian"]
MAX_DEPTHS = [2.0, 1.7, 0.95, 3.3]
SEAMS = [(h, w) for h in (31, 32, 33) for w in (63, 64, 65)]          # one 32 x 16 tile + 15 | 16 | 17 rows, 31 | 32 | 33 columns
SMALL = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (7, 2), (5, 5), (1, 257), (19, 27)]   # 1 x 257 and 19 x 27: H * W = k * 256 + 1
# float32 operations of a blurred pixel's accumulation chain (csrc/depth_fill.hip), each worth one ulp of the margin that
# the GPU tests allow beyond the oracle's own distance to float64:
#   bilateral  12 additions into `sum` (wsum has as many, in parallel) + the division + the subtraction of fd_finish_kernel = 14
#   gaussian   5 additions per pass, two passes + the subtraction of fd_finish_kernel                                       = 11
MARGIN_ULPS = {None: 0, "bilateral": 14, "gaussian": 11}
# bounds of the float32 ORACLE against float64, in ulps of the largest |tap| of the pixel's 5 x 5 window: one half ulp per rounding.
#   gaussian: 5 products + 5 additions per pass, the second pass carries the first's error once more: (10 + 10) / 2
#   bilateral: per tap the weight (table entry rounded to float32, 5 operations of the interpolation and the space weight), the
#   product and the two additions, 12 taps, and the division: (12 * 9 + 1) / 2, rounded up
ORACLE_ULPS = {"gaussian": 10, "bilateral": 55}

# name -> (frame, max_depth, the extrapolate settings it runs under, bound class of the two blurs)
#   "mid":  the project's 2e-6 m (every value in mid-range);  "wide": the per-pixel bound from float64 (values of tens of metres)
CASES = {}
for md in MAX_DEPTHS:
    CASES["thresholds_%g" % md] = (lambda md=md: Fx.depth_frame_thresholds(md, 0), md, (False,), "wide")
CASES["constant"] = (lambda: Fx.depth_frame_constant(0), 2.0, (False,), "mid")
CASES["near_constant"] = (lambda: Fx.depth_frame_near_constant(0), 2.0, (False,), "mid")
CASES["huge_range"] = (lambda: Fx.depth_frame_huge_range(0), 2.0, (False,), "wide")
CASES["columns_20x257"] = (lambda: Fx.depth_frame_columns(0, 20, 257), 2.0, (False, True), "mid")
CASES["columns_45x24"] = (lambda: Fx.depth_frame_columns(1, 45, 24), 2.0, (False, True), "mid")
for h, w in SMALL:
    CASES["geometry_%dx%d" % (h, w)] = (lambda h=h, w=w: Fx.depth_frame_geometry(h, w, 98 if (h, w) == (5, 5) else 0), 2.0,
                                        (False, True) if (h, w) in ((1, 9), (9, 1), (2, 2), (5, 5)) else (False,), "mid")
for h, w in SEAMS:
    CASES["seam_%dx%d" % (h, w)] = (lambda h=h, w=w: Fx.depth_frame_geometry(h, w), 2.0, (False,), "mid")
for s in (0, 1):
    CASES["plateaus_%d" % s] = (lambda s=s: Fx.depth_frame_plateaus(s), 2.0, (False,), "mid")
RUNS = [(n, e) for n, c in CASES.items() for e in c[2]]
RUN_IDS = ["%s-%s" % (n, "extrapolate" if e else "plain") for n, e in RUNS]

_cache = {}
WORST = {}                        # (case, blur) -> largest |float32 oracle - float64| in metres, for the report


def frame(name):
    if name not in _cache:
        mm = CASES[name][0]()
        mm.setflags(write=False)
        _cache[name] = mm
    return _cache[name]


def ulp32(x):
    """one float32 ulp at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x)).astype(f32)).astype(f64)


# ---- float64 evaluations of the two blurs, independent of oracle/depth_oracle.py --------------------------------------------------
def gaussian5_f64(img):
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    return ndimage.correlate1d(ndimage.correlate1d(img.astype(f64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")


def _reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), stated without numpy.pad"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _replicate(p, n):
    return min(max(p, 0), n - 1)


def _two_folds(p, n):
    """reflect101 as csrc/depth_fill_common.h states it: one fold at each end, then a clamp (the rule itself but for n = 2, p = 3)"""
    if p < 0:
        p = -p
    if p >= n:
        p = 2 * n - 2 - p
    return 0 if p < 0 else (n - 1 if p >= n else p)


def gaussian5_border_f64(img, border):
    """the separable [1 4 6 4 1] / 16 in float64 with the taps outside the frame taken by `border(p, n)`"""
    k = (0.0625, 0.25, 0.375, 0.25, 0.0625)
    H, W = img.shape
    v = img.astype(f64)
    rows = sum(k[t + 2] * v[:, [border(x + t, W) for x in range(W)]] for t in range(-2, 3))
    return sum(k[t + 2] * rows[[border(y + t, H) for y in range(H)], :] for t in range(-2, 3))


def bilateral5_table_f64(img, border=_reflect101):
    """the table rule of bilateralFilter_32f in float64: 4096 bins over [min, max] of the float32 image, linear interpolation
    between the entries, no rounding anywhere.  The bin width is the rule's own float32 scale_index (a parameter of the table, not
    a rounding of the sum).  Also returns the largest table index any tap reads and the table."""
    img32 = np.asarray(img, f32)
    mn, mx = float(img32.min()), float(img32.max())
    if abs(mn - mx) < EPS:
        return img32.astype(f64), -1, None
    scale = float(f32(BIL_BINS) / f32(mx - mn))
    lut = np.exp((np.arange(BIL_BINS + 2) / scale) ** 2 * (-0.5 / 1.5 ** 2))
    H, W = img32.shape
    v0 = img32.astype(f64)
    num, den, top = v0.copy(), np.ones((H, W)), 0
    for di in range(-2, 3):
        for dj in range(-2, 3):
            if (di == 0 and dj == 0) or di * di + dj * dj > 4:
                continue
            ys = [border(y + di, H) for y in range(H)]
            xs = [border(x + dj, W) for x in range(W)]
            v = v0[np.ix_(ys, xs)]
            a = np.abs(v - v0) * scale
            i = np.floor(a).astype(np.int64)
            top = max(top, int(i.max()))
            w = np.exp(-0.5 * (di * di + dj * dj) / 2.0 ** 2) * (lut[i] + (a - i) * (lut[i + 1] - lut[i]))
            num += v * w
            den += w
    return num / den, top, lut


def window_max_abs(img):
    return ndimage.maximum_filter(np.abs(img.astype(f64)), size=5, mode="nearest")


# ---- the oracle and its float64 counterpart for one run ----------------------------------------------------------------------------
def oracle(name, extrapolate, blur):
    """everything the tests share about one (case, extrapolate, blur): the oracle's stages and results (float32 metres, uint16), the
    float64 evaluation behind the exact median image, the oracle's per-pixel distance to it and the GPU's per-pixel bound"""
    key = (name, extrapolate, blur)
    if key in _cache:
        return _cache[key]
    mm, md = frame(name), CASES[name][1]
    st = {}
    m32 = D.fill_depth(mm / 1e3, md, extrapolate, blur, stages=st)
    o = dict(stages=st, m32=m32, mm16=D.grab_depth(mm, md, extrapolate, blur), md=md)
    med = st["median"]
    if blur == "bilateral":
        pre64 = bilateral5_table_f64(med)[0]
    elif blur == "gaussian":
        pre64 = np.where(med > T, gaussian5_f64(med), med.astype(f64))
    else:
        pre64 = med.astype(f64)
    inv64 = float(f32(md)) - pre64
    o["m64"] = np.where(pre64 > float(T), inv64, pre64)
    o["other64"] = np.where(pre64 > float(T), pre64, inv64)       # the other branch of the last comparison
    # the last comparison is a step of the function itself: where float64 sits within the margin of 0.1, or the float32 oracle
    # took the other branch, a float32 evaluation may land on either side
    o["on_step"] = ((st["blurred"] > T) != (pre64 > float(T))) | (np.abs(pre64 - float(T)) <= MARGIN_ULPS[blur] * ulp32(float(T)))
    o["dist"] = error_vs_f64(m32, o)
    o["bound"] = o["dist"] + MARGIN_ULPS[blur] * ulp32(o["m64"])
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    WORST[(name, extrapolate, blur)] = float(o["dist"].max())
    _cache[key] = o
    return o


def error_vs_f64(m, o):
    """|m - float64| per pixel; on the pixels that sit on the step of the last comparison, the distance to the nearer branch"""
    m = m.astype(f64)
    e = np.abs(m - o["m64"])
    return np.where(o["on_step"], np.minimum(e, np.abs(m - o["other64"])), e)


def mm_of(m):
    """(depth * 1000).astype(uint16) of predict_ros.py:41 as oracle/depth_oracle.py states it.  The expression is a float32 one (its
    product rounds 0.7f * 1000 up to 700), so float64 metres are first rounded to the float32 that fill_depth returns"""
    return ((m.astype(f32) * 1000).astype(np.int64) & 0xFFFF).astype(np.uint16)


def millimetre_flips(name, extrapolate, blur):
    """pixels (off the step) where the float32 oracle and float64 truncate to different millimetres"""
    o = oracle(name, extrapolate, blur)
    return (mm_of(o["m32"]) != mm_of(o["m64"])) & ~o["on_step"]


# The uint16 frames.  The fill chain MAKES plateaus (a grey dilation repeats the local maximum), and the blur of a plateau is a whole
# number of millimetres give or take an ulp: on most of these frames float32 and float64 already truncate to different millimetres
# somewhere, whatever the seed.  So the millimetre rule is stated per pixel:
#   settled pixels   the whole interval float64 +- bound truncates to one millimetre value: the GPU must give exactly that value;
#   other pixels     within a bound of a millimetre boundary, or on the 0.1 step: compared in metres, and at most 1 mm off;
# and the runs of FRAME_WIDE, on which float32 oracle and float64 agree on every millimetre (no flip at all, which is what a share
# under 1e-3 means on frames this small), are held to the project's frame-wide rule as well: at most 1 mm, on under 1e-3 of the
# pixels.  Every other blurred run is compared per pixel as above only.  test_oracle_distance_to_float64_and_millimetre_flips
# holds this list to what the CPU finds, in both directions.
FRAME_WIDE = {(n, e, b) for n, e in RUNS for b in ("bilateral", "gaussian")
              if n == "constant" or n in tuple("geometry_%dx%d" % hw for hw in SMALL[:7])}
FRAME_WIDE |= {("near_constant", False, "gaussian"), ("columns_45x24", False, "bilateral"), ("columns_45x24", False, "gaussian"),
               ("columns_45x24", True, "gaussian"), ("geometry_19x27", False, "gaussian")}


def millimetres_settled(name, extrapolate, blur):
    o = oracle(name, extrapolate, blur)
    return (mm_of(o["m64"] - o["bound"]) == mm_of(o["m64"] + o["bound"])) & ~o["on_step"]


def held_to_the_frame_wide_rule(name, extrapolate, blur):
    return blur is None or (name, extrapolate, blur) in FRAME_WIDE


# ---- proofs: each family reaches the branch it names -----------------------------------------------------------------------------
def prove_thresholds(name):
    mm, md = frame(name), CASES[name][1]
    far = int(round(md * 1000))
    d0 = (mm / 1e3).astype(f32)
    near = mm <= 102
    assert (d0[near] < T).any() and (d0[near] == T).any() and (d0[near] > T).any()          # fd_prepare_kernel, before the inversion
    assert {99, 100, 101} <= set(mm[near].tolist()) and {far - 99, far - 100, far - 101} <= set(mm.ravel().tolist())
    edge = (mm >= far - 102) & (mm <= far - 98)
    inv = f32(md) - d0[edge]
    assert (inv < T).any() and (inv > T).any()                                              # ... and what it leaves: hole or surface
    rep = dict(near=(int((d0 < T).sum()), int((d0 == T).sum())), inverted_on_0p1=int((inv == T).sum()))
    for blur in BLURS:                                                                      # fd_finish_kernel, after the blur
        pre = oracle(name, False, blur)["stages"]["blurred"]
        n = (int((pre < T).sum()), int((pre == T).sum()), int((pre > T).sum()))
        assert n[0] > 20 and n[2] > 20, (blur, n)
        if blur != "bilateral":                  # (the bilateral sum of a flat 0.1 region need not round back to 0.1)
            assert n[1] > 20, (blur, n)
        rep[str(blur)] = n
    # a max_depth that is no float32: keeping the double into the subtraction rounds differently on some valid pixel
    valid = d0 > T
    kept_double = (float(md) - d0[valid].astype(f64)).astype(f32)
    rep["double_differs"] = int((kept_double != f32(md) - d0[valid]).sum())
    assert (rep["double_differs"] > 20) == (float(f32(md)) != md), rep
    return rep


def bilateral_index_reach(name, extrapolate=False):
    """(largest table index a tap reads when the index is formed in float32 as the filter forms it, number of table entries that
    underflowed to zero in float32)"""
    med = oracle(name, extrapolate, None)["stages"]["median"]
    _, _, lut = bilateral5_table_f64(med)
    scale = f32(BIL_BINS) / f32(float(med.max()) - float(med.min()))
    p = np.pad(med, 2, mode="reflect")
    H, W = med.shape
    top = max(int(np.floor(np.abs(p[2 + di:2 + di + H, 2 + dj:2 + dj + W] - med) * scale).max())
              for di in range(-2, 3) for dj in range(-2, 3) if di * di + dj * dj <= 4)
    return top, int((lut.astype(f32) == 0).sum())


def prove_constant(name):
    med = oracle(name, False, None)["stages"]["median"]
    rng = float(med.max()) - float(med.min())
    if name == "constant":
        assert rng < EPS and (frame(name) == 0).sum() >= 5
    else:
        assert EPS <= rng < 1.001e-3                       # one millimetre: no uint16 frame gets closer to FLT_EPSILON from above
        assert bilateral_index_reach(name)[0] == BIL_BINS  # idx + 1 = BIL_BINS + 1, the table's last entry
    return rng


def prove_huge_range(name):
    med = oracle(name, False, None)["stages"]["median"]
    top, zeros = bilateral_index_reach(name)
    # the image's min and max are neighbours: a tap between them reads the table's last bins (idx + 1 >= BIL_BINS, and BIL_BINS + 1
    # where len * (BIL_BINS / len) rounds to BIL_BINS in float32)
    assert med.min() < -60 and med.max() > 1.8 and top >= BIL_BINS - 1 and zeros > BIL_BINS // 2, (med.min(), med.max(), top, zeros)
    return float(med.min()), float(med.max()), top, zeros


def prove_columns(name):
    """the kinds of column fd_extrapolate_kernel sees (the image after the 7 x 7 fill)"""
    mm = frame(name)
    H, W = mm.shape
    img = oracle(name, True, None)["stages"]["holes_filled"]
    valid = img > T
    top = np.argmax(valid, axis=0)
    empty = ~valid.any(0)
    # an empty column that a wrong `top` would change: some pixel above the last row differs from the last row's
    empty_live = empty & (img[:-1] != img[-1:]).any(0)
    row0 = valid[0]
    last_only = (mm[:-1] == 0).all(0) & (mm[-1] > 100) & valid.any(0)
    rep = dict(empty=int(empty.sum()), empty_live=int(empty_live.sum()), row0=int(row0.sum()), deepest_top=int(top.max()),
               last_row_only_input=int(last_only.sum()), tops=len(set(top[~empty].tolist())))
    if W > 256:
        assert rep["empty_live"] >= 3 and rep["row0"] >= 10 and rep["tops"] >= 6, rep
        # "the only valid pixel in the last row" exists for the INPUT only: the diamond dilation in front of the extrapolation lifts
        # every valid pixel by two rows, the close keeps them and the 7 x 7 fill adds three, so such a column reaches the kernel with
        # its first valid row at H - 6, and no column of any frame with its first valid row at H - 1
        assert rep["last_row_only_input"] >= 3 and (top[last_only] == H - 6).sum() >= 3 and rep["deepest_top"] < H - 1, rep
        assert top[256] > 0 and not empty[256]             # the second workgroup's column has work of its own
    else:
        assert W < 31 < H and rep["tops"] >= 3, rep
    ex = oracle(name, True, None)["stages"]["extrapolated"]
    assert (ex != img).sum() > 20                          # the extrapolation writes
    after = oracle(name, True, None)["stages"]["filled"]
    assert (after != ex).sum() > 20                        # ... and the 31 x 31 fill behind it does, on a frame smaller than 31
    return rep


def border_reach(name, extrapolate=False):
    """pixels of the frame at which each stage's border rule decides the result: the rule against its nearest alternative, on the
    image that stage really gets.  For the two blurs the difference has to be visible, 1e-4 m being 50 times the mid-range bound."""
    st = oracle(name, extrapolate, None)["stages"]
    ones5 = np.ones((5, 5), np.uint8)
    dilated = D.dilate(D.dilate(st["prepared"], D.DIAMOND5), ones5)         # what the erosion of the close gets
    med = st["median"]
    rep = dict(
        # the morphology ignores what lies outside the frame: against an outside of zeros
        erode=int((D.erode(dilated, ones5) != ndimage.grey_erosion(dilated, footprint=ones5.astype(bool), mode="constant", cval=0.0)).sum()),
        # the median repeats the edge pixel: against reflect-101
        median=int((med != ndimage.median_filter(st["filled"], size=5, mode="mirror")).sum()),
        # the blurs reflect: against repeating the edge pixel
        gaussian=int(((np.abs(gaussian5_border_f64(med, _reflect101) - gaussian5_border_f64(med, _replicate)) > 1e-4) & (med > T)).sum()),
        bilateral=int((np.abs(bilateral5_table_f64(med)[0] - bilateral5_table_f64(med, _replicate)[0]) > 1e-4).sum()))
    # one fold at each end and a clamp (the kernels' statement) against folding until inside (the rule): the same image, exactly
    assert np.array_equal(gaussian5_border_f64(med, _two_folds), gaussian5_border_f64(med, _reflect101))
    assert np.array_equal(bilateral5_table_f64(med, _two_folds)[0], bilateral5_table_f64(med)[0])
    return rep


# Which border rule the small frames reach.  Every window of the 5 x 5 dilation holds the whole of an axis of three pixels or fewer, so
# from the close on the image is constant along such an axis, through the fills, the extrapolation and the median
# (test_an_axis_of_three_or_fewer_is_flat_at_the_blurs).  Hence:
#   1 x 1, 2 x 2                constant by the time of the median: they reach the morphology's rule (the erosion would give 0 if the
#                               outside counted as zeros) and the launch geometry, and NO border rule of the median or the blurs;
#   1 x 9, 9 x 1, 2 x 7, 7 x 2, constant across the strip, a step two pixels from its end along it (the generator builds it): the
#   1 x 257                     replicate rule of the median and the reflect-101 rule of both blurs decide pixels there;
#   5 x 5                       most 5 x 5 frames come out of the chain flat; this one (its seed is chosen for it) keeps 10 mm of
#                               structure, and the border rule of both blurs decides pixels on it;
#   19 x 27, the seam frames    the morphology's and the blurs' rules on all four sides; the median's only where a filled hole touches
#                               the edge (the close leaves three equal pixels there, which replicate and reflect read alike): counted,
#                               not required.
# So the blurs' reflect-101 cannot be observed on an axis of three or fewer.  That covers the axis of two, the one length on which one
# fold at each end and a clamp (csrc/depth_fill_common.h) differ from the rule.  The frames that carry the reflect-101 check are those
# of REFLECT_101_CARRIERS, beside the threshold, huge-range, columns and plateau frames, which reach it as any frame with structure
# near its edge does.
FLAT_AT_THE_BLURS = ("geometry_1x1", "geometry_2x2")
REFLECT_101_CARRIERS = tuple("geometry_%dx%d" % hw for hw in SMALL if hw not in ((1, 1), (2, 2))) + tuple("seam_%dx%d" % hw for hw in SEAMS)


def prove_geometry(name):
    mm = frame(name)
    H, W = mm.shape
    assert (mm > 100).any() and (H * W < 4 or (mm == 0).any())
    if name in ("geometry_1x257", "geometry_19x27"):
        assert H * W % 256 == 1
    if name.startswith("seam"):
        assert H - 16 in (15, 16, 17) and W - 32 in (31, 32, 33)
    assert (name in FLAT_AT_THE_BLURS) != (name in REFLECT_101_CARRIERS)
    for extrapolate in CASES[name][2]:
        rep = border_reach(name, extrapolate)
        med = oracle(name, extrapolate, None)["stages"]["median"]
        assert rep["erode"] > 0, rep
        if H <= 3:
            assert (med == med[:1]).all()
        if W <= 3:
            assert (med == med[:, :1]).all()
        if name in FLAT_AT_THE_BLURS:
            assert med.min() == med.max() > T and rep["median"] == rep["gaussian"] == rep["bilateral"] == 0, rep
        else:
            assert rep["gaussian"] > 0 and rep["bilateral"] > 0 and (rep["median"] > 0 or min(H, W) > 2), rep
    return dict(shape=(H, W), **rep)


def prove_plateaus(name):
    """pixels whose 12th, 13th and 14th smallest taps differ: taking v[11] or v[13] for the median changes the image"""
    img = oracle(name, False, None)["stages"]["filled"]
    p = np.pad(img, 2, mode="edge")
    H, W = img.shape
    s = np.sort(np.stack([p[i:i + H, j:j + W] for i in range(5) for j in range(5)], 0), axis=0)
    below, above = int((s[11] != s[12]).sum()), int((s[13] != s[12]).sum())
    distinct = np.array([[len(set(s[:, y, x].tolist())) for x in range(W)] for y in range(H)])
    assert below >= 20 and above >= 20 and (distinct <= 3).mean() > 0.9, (below, above)
    return below, above


def prove(name):
    """the proof of the family `name` belongs to; returns what it counted"""
    fam = name.split("_")[0]
    if fam == "thresholds":
        return prove_thresholds(name)
    if fam in ("constant", "near"):
        return prove_constant(name)
    if fam == "huge":
        return prove_huge_range(name)
    if fam == "columns":
        return prove_columns(name)
    if fam == "plateaus":
        return prove_plateaus(name)
    return prove_geometry(name)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def test_generators_are_deterministic_and_small():
    for name, (make, _, _, _) in CASES.items():
        a, b = make(), make()
        assert a.dtype == np.uint16 and a.ndim == 2 and np.array_equal(a, b)
        assert a.shape[0] <= 70 and a.shape[1] <= 300, (name, a.shape)
    assert not np.array_equal(Fx.depth_frame_plateaus(0), Fx.depth_frame_plateaus(1))
    assert not np.array_equal(Fx.depth_frame_huge_range(0), Fx.depth_frame_huge_range(1))


@pytest.mark.parametrize("name", list(CASES))
def test_family_reaches_its_branch(name):
    print("%s: %s" % (name, prove(name)))


@pytest.mark.parametrize("name", list(CASES))
def test_morphology_and_median_vs_scipy_bitwise(name):
    """as tests/test_fill_depth.py does for the smooth frames: on the inverted image and on the image the median really gets"""
    st = oracle(name, CASES[name][2][-1], None)["stages"]
    for img in (st["prepared"], st["filled"]):
        for k in (D.DIAMOND5, np.ones((5, 5), np.uint8), np.ones((7, 7), np.uint8), np.ones((31, 31), np.uint8)):
            fp = k.astype(bool)
            assert np.array_equal(D.dilate(img, k), ndimage.grey_dilation(img, footprint=fp, mode="constant", cval=-np.inf))
            assert np.array_equal(D.erode(img, k), ndimage.grey_erosion(img, footprint=fp, mode="constant", cval=np.inf))
        assert np.array_equal(D.median5(img), ndimage.median_filter(img, size=5, mode="nearest"))


@pytest.mark.parametrize("name,extrapolate", RUNS, ids=RUN_IDS)
def test_blurs_vs_float64_per_pixel(name, extrapolate):
    med = oracle(name, extrapolate, None)["stages"]["median"]
    scale = ulp32(window_max_abs(med))
    g = np.abs(D.gaussian5(med) - gaussian5_f64(med)) / scale
    b = np.abs(D.bilateral5(med) - bilateral5_table_f64(med)[0]) / scale
    print("%s: gaussian %.2f ulp, bilateral %.2f ulp of the window's largest |tap|" % (name, g.max(), b.max()))
    assert g.max() <= ORACLE_ULPS["gaussian"] and b.max() <= ORACLE_ULPS["bilateral"]
    if float(med.max()) - float(med.min()) < EPS:
        assert np.array_equal(D.bilateral5(med), med)


def test_table_and_closed_form_part_ways_on_the_huge_range():
    """why the float64 side states the table: with bins of 16 mm the interpolated table is off the closed-form exp by more than
    the 2e-6 m of the mid-range bound, on the mid-range frames by a tenth of it"""
    def closed(img):
        H, W = img.shape
        p = np.pad(img.astype(f64), 2, mode="reflect")
        num, den = img.astype(f64).copy(), np.ones((H, W))
        for di in range(-2, 3):
            for dj in range(-2, 3):
                if (di == 0 and dj == 0) or di * di + dj * dj > 4:
                    continue
                v = p[2 + di:2 + di + H, 2 + dj:2 + dj + W]
                w = np.exp(-0.5 * (v - img) ** 2 / 1.5 ** 2) * np.exp(-0.5 * (di * di + dj * dj) / 2.0 ** 2)
                num += v * w; den += w
        return num / den
    huge = oracle("huge_range", False, None)["stages"]["median"]
    mid = oracle("plateaus_0", False, None)["stages"]["median"]
    assert np.abs(bilateral5_table_f64(huge)[0] - closed(huge)).max() > 1e-6
    assert np.abs(bilateral5_table_f64(mid)[0] - closed(mid)).max() < 2e-7


@pytest.mark.parametrize("name,extrapolate", RUNS, ids=RUN_IDS)
def test_oracle_distance_to_float64_and_millimetre_flips(name, extrapolate):
    """the figures the GPU bound is made of, and the condition of the uint16 rule: decided here, on the CPU"""
    for blur in BLURS:
        o = oracle(name, extrapolate, blur)
        flips = millimetre_flips(name, extrapolate, blur)
        print("%s %s: float32 oracle vs float64 %.3e m, %d pixels on the 0.1 step, %d millimetre flips, %d settled of %d"
              % (name, blur, o["dist"].max(), int(o["on_step"].sum()), int(flips.sum()),
                 int(millimetres_settled(name, extrapolate, blur).sum()), flips.size))
        if blur is None:
            assert o["dist"].max() == 0 and not flips.any()           # selections and one exact subtraction
        if CASES[name][3] == "mid":
            assert o["dist"].max() < 1e-6                              # half of the project's 2e-6: the oracle leaves the GPU room
        settled = millimetres_settled(name, extrapolate, blur)
        assert np.array_equal(mm_of(o["m32"])[settled], mm_of(o["m64"])[settled]) and np.array_equal(mm_of(o["m32"]), o["mm16"])
        assert flips.any() == (not held_to_the_frame_wide_rule(name, extrapolate, blur)), int(flips.sum())
        # the step excuses a pixel only where the image in front of the blur already sits on 0.1 (a flat band at the threshold, which
        # the blur=None run of the same frame holds bit for bit): no blur carries a pixel there from elsewhere
        on = o["on_step"]
        assert (np.abs(o["stages"]["median"][on].astype(f64) - float(T)) <= MARGIN_ULPS["bilateral"] * ulp32(float(T))).all()
        assert not on.any() or name.startswith(("thresholds", "columns"))


def test_an_axis_of_three_or_fewer_is_flat_at_the_blurs():
    """Why no frame can show the blurs' border rule along an axis of three pixels or fewer: the 5-wide dilation of the close reads
    two pixels to either side, which from any pixel of such an axis is all of it, so the dilated image is constant along the axis.
    The erosion and the fills take a minimum or a maximum over windows that are alike for every pixel along a constant axis, the
    extrapolation copies within columns that are constant or all alike, and the replicate median keeps a constant axis constant.
    (Four and five pixels are not enough: a random 4 x 6 frame is a counterexample.)  Checked on random frames of every such size,
    with every kind of value the chain distinguishes."""
    rng = np.random.default_rng(0)
    levels = np.array([0, 0, 0, 99, 100, 101, 640, 700, 1300, 1899, 1900, 1901, 2600, 65535])
    for h in range(1, 4):
        for w in range(1, 13):
            for H, W in ((h, w), (w, h)):
                for _ in range(4):
                    mm = levels[rng.integers(0, len(levels), (H, W))].astype(np.uint16)
                    for extrapolate in (False, True):
                        st = {}
                        D.fill_depth(mm / 1e3, 2.0, extrapolate, None, stages=st)
                        med = st["median"]
                        if H <= 3:
                            assert (med == med[:1]).all(), (mm, extrapolate)
                        if W <= 3:
                            assert (med == med[:, :1]).all(), (mm, extrapolate)
                        # ... so a frame that small both ways is blurred the same whatever rule places the outside taps
                        for border in (_replicate, _two_folds) if max(H, W) <= 3 else ():
                            assert np.array_equal(gaussian5_border_f64(med, border), gaussian5_border_f64(med, _reflect101))
                            assert np.array_equal(bilateral5_table_f64(med, border)[0], bilateral5_table_f64(med)[0])


def test_extended_stages_do_not_change_the_result():
    """the `stages` the proofs read are copies: the chain with and without them is the same, on every max_depth"""
    for name in ("thresholds_1.7", "thresholds_0.95", "columns_45x24"):
        mm, md = frame(name), CASES[name][1]
        for blur in BLURS:
            assert np.array_equal(D.fill_depth(mm / 1e3, md, True, blur), D.fill_depth(mm / 1e3, md, True, blur, stages={}))
    # max_depth enters as float32(max_depth), as NumPy evaluates `max_depth - depth[valid]` on a float32 image
    d = (frame("thresholds_1.7") / 1e3).astype(f32)
    st = {}
    D.fill_depth(frame("thresholds_1.7") / 1e3, 1.7, False, None, stages=st)
    assert np.array_equal(st["prepared"][d > T], (1.7 - d)[d > T]) and (1.7 - d).dtype == f32


def test_zz_report_oracle_distances():
    """(runs last) the largest float32-oracle-to-float64 distance per case and blur"""
    for (name, extrapolate, blur), w in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        if blur is not None:
            print("%-18s %-11s %-9s float32 oracle vs float64 %.3e m" % (name, "extrapolate" if extrapolate else "plain", blur, w))
