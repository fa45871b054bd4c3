"""GPU: the depth-fill kernels (csrc/depth_fill.hip one launch per step, csrc/depth_fill_fused.hip the tiled chain and the rectangle
pass) against oracle/depth_oracle.py on the frames of tests/test_fill_depth_hard_frames_oracle.py -- the ones built to reach the
branches smooth mid-range surfaces never reach.  Every test first runs that file's proof that the frame reaches its branch.

  blur=None            float32 metres and the uint16 frame equal the oracle's bit for bit (the chain only selects values).
  bilateral, gaussian  per pixel |GPU - float64| <= |float32 oracle - float64| + MARGIN_ULPS ulps of the pixel's float64 value, the
                       float64 side being the same rules without rounding (for the bilateral the 4096-bin table, interpolated).
                       The margin is the number of float32 operations of a pixel's accumulation chain in the kernel source:
                         bilateral 14 = 12 additions into `sum` + the division + fd_finish_kernel's subtraction,
                         gaussian  11 = 5 additions per pass, two passes + fd_finish_kernel's subtraction.
                       Families whose values stay in mid-range are ALSO held to the project's |GPU - oracle| < 2e-6 m.
                       Largest float32-oracle-to-float64 distance per family as measured on the CPU (metres; bilateral, gaussian):
                         thresholds 5.6e-7 5.4e-7 | constant 0 0 | near_constant 2.2e-7 8.9e-8 | huge_range 1.1e-5 2.3e-6 |
                         columns 4.4e-7 2.5e-7 | geometry 4.0e-7 2.8e-7 | seam 4.4e-7 2.6e-7 | plateaus 3.3e-7 2.0e-7
                       (test_zz_report prints them again, beside what the GPU did: on an MI355X the kernels gave the float32 oracle's
                       value bit for bit on every family, so their distance to float64 was the oracle's own).
  uint16 after a blur  the fill chain makes plateaus, whose blur is a whole millimetre give or take an ulp, so these frames are NOT
                       free of pixels within an ulp of a millimetre boundary.  Per pixel instead: where float64 +- bound truncates
                       to one millimetre the GPU gives exactly it; elsewhere at most 1 mm off; the runs listed in FRAME_WIDE of the
                       CPU file (float32 oracle and float64 agree on every millimetre there) are also held to the frame-wide rule
                       (under 1e-3 of the pixels off).
  pixels on the step   the last `> 0.1` is a step of the function: where float64 is within the margin of 0.1 either branch counts.
                       The CPU file shows that this happens only where the image in front of the blur sits on 0.1 already (flat
                       bands of the threshold and columns frames), which the blur=None run of the same frame holds bit for bit.
  border rules         the CPU file says which frames reach which (REFLECT_101_CARRIERS): the blurs' reflect-101 decides pixels on
                       every geometry frame but 1 x 1 and 2 x 2, which are flat by then whatever they hold.
  rectangle routes     se3tn_fill_depth_rect / _rects on the rectangles of test_gpu_fill_depth_rects.rects(): bit for bit the oracle
                       with blur=None, bit for bit the full chain with a blur (the full chain being held to float64 above)."""
import numpy as np
import pytest

import test_fill_depth_hard_frames_oracle as HF
import test_gpu_fill_depth_rects as RR

pytestmark = pytest.mark.gpu

BLURS = HF.BLURS
MID_BOUND = 2e-6
GPU_WORST = {}       # (family, blur) -> [largest |GPU - float64|, largest bound used, largest |GPU - float32 oracle|]
_proved = {}


@pytest.fixture(scope="module")
def eng():
    import se3tracknet_amd as se3
    return se3.Engine(0, 1)


def proved(name):
    if name not in _proved:
        _proved[name] = HF.prove(name)
    return _proved[name]


def family(name):
    return name if name in ("near_constant", "huge_range") else name.split("_")[0]


def rects_of(name):
    """test_gpu_fill_depth_rects.rects() for a frame of this file: the whole frame, the four corners, 1 x 1 at both ends, a block
    across the tile seams, a row, a column, overlapping and repeated rectangles, an empty one"""
    # rects() takes the name of a frame of its own module's FRAMES table and reads nothing but its shape, so the frame is entered
    # there under a name of this file's (the table is read by name only, after collection: no test of that module sees the entry)
    key = "hard_frames/" + name
    RR.FRAMES.setdefault(key, lambda: HF.frame(name))
    return RR.rects(key)


@pytest.mark.parametrize("blur", BLURS, ids=[str(b) for b in BLURS])
@pytest.mark.parametrize("name,extrapolate", HF.RUNS, ids=HF.RUN_IDS)
def test_full_chain_vs_oracle(eng, name, extrapolate, blur):
    proved(name)
    mm, md = np.array(HF.frame(name)), HF.CASES[name][1]      # (a writable copy for torch.from_numpy)
    o = HF.oracle(name, extrapolate, blur)
    got_mm, got_m = eng.fill_depth(mm, md, extrapolate, blur, return_metres=True)
    assert got_m.dtype == np.float32 and got_mm.dtype == np.uint16 and got_m.shape == mm.shape == got_mm.shape
    if blur is None:
        assert np.array_equal(got_m, o["m32"]), np.argwhere(got_m != o["m32"])[:5]
        assert np.array_equal(got_mm, o["mm16"])
        return
    err = HF.error_vs_f64(got_m, o)
    off_step = ~o["on_step"]
    to_oracle = np.abs(got_m.astype(np.float64) - o["m32"])[off_step].max() if off_step.any() else 0.0
    w = GPU_WORST.setdefault((family(name), blur), [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], float(err.max())), max(w[1], float(o["bound"].max())), max(w[2], float(to_oracle))
    print("%s %s: |GPU - float64| %.3e (bound up to %.3e, oracle's own %.3e), |GPU - float32 oracle| %.3e off the step"
          % (name, blur, err.max(), o["bound"].max(), o["dist"].max(), to_oracle))
    worst = np.unravel_index(np.argmax(err - o["bound"]), err.shape)
    assert (err <= o["bound"]).all(), (worst, err[worst], o["bound"][worst])
    if HF.CASES[name][3] == "mid":
        assert to_oracle < MID_BOUND
    d = np.abs(got_mm.astype(int) - o["mm16"].astype(int))
    settled = HF.millimetres_settled(name, extrapolate, blur)
    assert (d[settled] == 0).all() and (d[off_step] <= 1).all()
    if HF.held_to_the_frame_wide_rule(name, extrapolate, blur):
        assert d[off_step].size == 0 or (d[off_step] > 0).mean() < 1e-3


@pytest.mark.parametrize("blur", BLURS, ids=[str(b) for b in BLURS])
@pytest.mark.parametrize("name,extrapolate", HF.RUNS, ids=HF.RUN_IDS)
def test_rectangle_routes_vs_oracle_and_full_chain(eng, name, extrapolate, blur):
    proved(name)
    mm, md = np.array(HF.frame(name)), HF.CASES[name][1]      # (a writable copy for torch.from_numpy)
    want = HF.oracle(name, extrapolate, None)["mm16"] if blur is None else eng.fill_depth(mm, md, extrapolate, blur)
    rs = rects_of(name)
    got = eng.fill_depth_rects(mm, rs, md, extrapolate, blur)                       # one call: the tiled chain once, every rectangle
    for (x0, y0, x1, y1), g in zip(rs, got):
        assert g.shape == (max(y1 - y0, 0), max(x1 - x0, 0)) if x1 > x0 and y1 > y0 else g.size == 0
        assert np.array_equal(g, want[y0:y1, x0:x1] if g.size else g), ("rects", (x0, y0, x1, y1))
    for x0, y0, x1, y1 in dict.fromkeys(rs):                                        # one call each
        if x1 > x0 and y1 > y0:
            g = eng.fill_depth_rect(mm, (x0, y0, x1, y1), md, extrapolate, blur)
            assert np.array_equal(g, want[y0:y1, x0:x1]), ("rect", (x0, y0, x1, y1))


@pytest.mark.parametrize("extrapolate", [False, True], ids=["plain", "extrapolate"])
@pytest.mark.parametrize("route", ["rect", "rects"])
def test_range_words_do_not_outlive_their_frame(eng, route, extrapolate):
    """huge range, constant, huge range again through the rectangle route of ONE engine, frames of one size so that the min / max
    words and the table sit at the same addresses: the constant frame comes back copied through (equal to blur=None), the third
    call equals the first byte for byte"""
    from oracle import depth_oracle as D
    from oracle import fixtures as Fx
    huge = Fx.depth_frame_huge_range(0)
    H, W = huge.shape
    const = Fx.depth_frame_constant(0, H, W)
    med = {}
    D.fill_depth(const / 1e3, 2.0, extrapolate, None, stages=med)
    assert float(med["median"].max()) - float(med["median"].min()) < HF.EPS and proved("huge_range")

    def call(mm):
        if route == "rect":
            return eng.fill_depth_rect(mm, (0, 0, W, H), 2.0, extrapolate, "bilateral")
        return np.concatenate([g.ravel() for g in eng.fill_depth_rects(mm, [(0, 0, W, H), (W - 9, H - 7, W, H)], 2.0, extrapolate, "bilateral")])
    first = call(huge)
    second = call(const)
    third = call(huge)
    assert np.array_equal(second[:H * W].reshape(H, W) if route == "rects" else second, D.grab_depth(const, 2.0, extrapolate, None))
    assert first.tobytes() == third.tobytes()
    assert np.array_equal(first[:H * W].reshape(H, W) if route == "rects" else first, eng.fill_depth(huge, 2.0, extrapolate, "bilateral"))


def test_zz_report_fill_depth_distances():
    """(runs last) per family and blur: the float32 oracle's own distance to float64 (CPU), the GPU's, the largest bound used"""
    print("margin: %d ulps (bilateral), %d ulps (gaussian) of the pixel's float64 value" % (HF.MARGIN_ULPS["bilateral"], HF.MARGIN_ULPS["gaussian"]))
    own = {}
    for (name, _, blur), w in HF.WORST.items():
        if blur is not None:
            own[(family(name), blur)] = max(own.get((family(name), blur), 0.0), w)
    for key in sorted(own):
        g = GPU_WORST.get(key)
        print("%-14s %-9s float32 oracle vs float64 %.3e m | GPU vs float64 %s | bound up to %s | GPU vs float32 oracle %s"
              % (key[0], key[1], own[key], *(("%.3e" % v for v in g) if g else ("not run",) * 3)))
        if g:
            assert g[0] <= g[1]
