"""The rule of se3tn_color_stats stated independently (a helper module: numpy and plain Python, no library call and no call of
utils.color_stats): one loop over the 176 x 176 crop pixels of a (model, observed) descriptor pair.

A descriptor is dict(rgb=uint8 [H,W,3], depth=uint16 [H,W], window=(left, top, right, bottom)).  The crop pixel (x, y) shows the image
pixel (left + sx, top + sy) with  sx = min(floor(x * (1.0 / (176.0 / width))), width - 1)  evaluated in float64, three operations in
this order (cv2.resize INTER_NEAREST, tests/crop_rule_cases.py), and zero -- colour and depth -- outside the image.  A pixel is
compared exactly when both depths are valid (100 < d < 2000) and |o - m| <= tol; the colour is read where the depth was read.

cases(): the descriptor pairs the CPU and the GPU tests share, expected(): their records, computed once."""
import functools
import math

import numpy as np

RES = 176
TOL = 6
SUMS = ("sum_m", "sum_o", "sum_mm", "sum_oo", "sum_mo", "sum_abs")
FIT_KEYS = ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "tol_mm", "_reserved")


def _table(size):
    inv = 1.0 / (float(RES) / float(size))
    return [min(int(math.floor(float(x) * inv)), size - 1) for x in range(RES)]


def _valid(d):
    return 100 < d < 2000


def record(model, observed, tol):
    """(fit, colour) of one pair as dicts of Python ints (the colour sums as lists of three)"""
    tabs = []
    for c in (model, observed):
        l, t, r, b = c["window"]
        tabs.append(([l + s for s in _table(r - l)], [t + s for s in _table(b - t)]))
    fit = dict.fromkeys(FIT_KEYS, 0)
    col = {k: [0, 0, 0] for k in SUMS}
    col["px"] = 0
    fit["tol_mm"] = col["tol_mm"] = int(tol)
    (mx, my), (ox, oy) = tabs
    mH, mW = model["depth"].shape
    oH, oW = observed["depth"].shape
    mdep, odep = model["depth"].tolist(), observed["depth"].tolist()
    mrgb, orgb = model["rgb"], observed["rgb"]
    for y in range(RES):
        fmy, foy = my[y], oy[y]
        for x in range(RES):
            fmx, fox = mx[x], ox[x]
            m = mdep[fmy][fmx] if 0 <= fmy < mH and 0 <= fmx < mW else 0
            o = odep[foy][fox] if 0 <= foy < oH and 0 <= fox < oW else 0
            if not _valid(m):
                continue
            fit["model_px"] += 1
            if not _valid(o):
                continue
            fit["seen_px"] += 1
            d = o - m
            if abs(d) > tol:
                fit["front_px" if d < 0 else "behind_px"] += 1
                continue
            fit["inlier_px"] += 1
            fit["sum_abs_mm"] += abs(d)
            col["px"] += 1
            pm, po = mrgb[fmy, fmx], orgb[foy, fox]
            for ch in range(3):
                a, b_ = int(pm[ch]), int(po[ch])
                col["sum_m"][ch] += a
                col["sum_o"][ch] += b_
                col["sum_mm"][ch] += a * a
                col["sum_oo"][ch] += b_ * b_
                col["sum_mo"][ch] += a * b_
                col["sum_abs"][ch] += abs(b_ - a)
    return fit, col


def as_arrays(se3, recs):
    """a list of record() results as the library's structured arrays (fit [n], colour [n])"""
    fit = np.zeros(len(recs), se3._lib.FIT_DTYPE)
    col = np.zeros(len(recs), se3._lib.COLOR_FIT_DTYPE)
    for i, (f, c) in enumerate(recs):
        for k in FIT_KEYS:
            fit[k][i] = f[k]
        col["px"][i], col["tol_mm"][i] = c["px"], c["tol_mm"]
        for k in SUMS:
            col[k][i] = c[k]
    return fit, col


# ---- the shared cases --------------------------------------------------------------------------------------------------------------
H, W = 230, 260
WINDOWS = dict(identity=(40, 30, 216, 206), up_nonsquare=(90, 60, 173, 137), down_nonsquare=(-20, -10, 250, 225),
               left_top=(-30, -45, 120, 100), right_bottom=(150, 120, 300, 290), miss=(400, 100, 550, 240))


def _images(seed, h, w):
    """model / observed (rgb, depth): a surface around 600 mm, the observed one -12 .. 12 mm off it (inliers, in front, behind), both
    with holes and the validity thresholds; the observed colours follow the model's with noise, so the sums differ in every word"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = (600 + 50 * np.sin(xx / 19.0) + 40 * np.cos(yy / 13.0) + rng.integers(-3, 4, (h, w))).astype(np.int64)
    o = m + rng.integers(-12, 13, (h, w))
    for img, vals in ((m, (0, 100, 2000, 65535, 101, 1999)), (o, (0, 100, 2000, 65535, 101, 1999, 300, 1500))):
        sel = rng.random((h, w))
        for k, v in enumerate(vals):
            img[(sel > 0.03 * k) & (sel < 0.03 * k + 0.02)] = v
    mrgb = rng.integers(0, 256, (h, w, 3))
    orgb = np.clip(mrgb * np.array([0.8, 0.5, -0.6]) + np.array([20, 60, 200]) + rng.integers(-30, 31, (h, w, 3)), 0, 255)
    return (mrgb.astype(np.uint8), m.astype(np.uint16)), (orgb.astype(np.uint8), o.astype(np.uint16))


def _thresholds():
    """176 x 176 images, identity windows: rows 0-3 hold the depths 100 / 101 / 1999 / 2000 in both images (only 101 and 1999 are
    valid); below them the model is 600 and the observed 600 + TOL on even columns (compared), 600 + TOL + 1 on odd ones (behind),
    and in the lower half 600 - TOL / 600 - TOL - 1 (compared / in front)"""
    rng = np.random.default_rng(3)
    m = np.full((RES, RES), 600, np.uint16)
    o = np.full((RES, RES), 600, np.uint16)
    o[:, 0::2] += TOL
    o[:, 1::2] += TOL + 1
    o[RES // 2:, 0::2] = 600 - TOL
    o[RES // 2:, 1::2] = 600 - TOL - 1
    for r, v in enumerate((100, 101, 1999, 2000)):
        m[r] = o[r] = v
    return (rng.integers(0, 256, (RES, RES, 3), dtype=np.uint8), m), (rng.integers(0, 256, (RES, RES, 3), dtype=np.uint8), o)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (model descriptor, observed descriptor)"""
    (mrgb, mdep), (orgb, odep) = _images(1, H, W)
    (m2rgb, m2dep), _ = _images(2, 120, 160)
    full = (0, 0, RES, RES)
    out = {}
    for k, win in WINDOWS.items():
        out[k] = (dict(rgb=mrgb, depth=mdep, window=win), dict(rgb=orgb, depth=odep, window=win))
    # model and observed under different descriptors: another image size, another window, another scale
    out["different"] = (dict(rgb=m2rgb, depth=m2dep, window=(10, 5, 130, 110)), dict(rgb=orgb, depth=odep, window=WINDOWS["up_nonsquare"]))
    # a model that is there against an observed window that misses its image: px == 0 with model_px > 0
    out["observed_miss"] = (dict(rgb=mrgb, depth=mdep, window=WINDOWS["identity"]), dict(rgb=orgb, depth=odep, window=WINDOWS["miss"]))
    (trgb, tdep), (trgb2, tdep2) = _thresholds()
    out["thresholds"] = (dict(rgb=trgb, depth=tdep, window=full), dict(rgb=trgb2, depth=tdep2, window=full))
    white, flat = np.full((RES, RES, 3), 255, np.uint8), np.full((RES, RES), 700, np.uint16)
    out["saturating"] = (dict(rgb=white, depth=flat, window=full), dict(rgb=white.copy(), depth=flat.copy(), window=full))
    for m, o in out.values():
        for c in (m, o):
            c["rgb"].setflags(write=False); c["depth"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """name -> record() of the case at TOL"""
    return {k: record(m, o, TOL) for k, (m, o) in cases().items()}
