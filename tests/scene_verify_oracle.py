"""The rule of se3tn_color_stats_scene stated independently (a helper module: numpy and plain Python, no library call, no call of
utils.fit_stats / utils.color_stats and none of color_fit_oracle.record): one loop over the 176 x 176 crop pixels of a (model, observed,
scene) descriptor triple.

A descriptor is dict(depth=uint16 [H,W], window=(left, top, right, bottom)), model and observed with rgb=uint8 [H,W,3] as well.  The crop
pixel (x, y) shows the image pixel (left + sx, top + sy) with  sx = min(floor(x * (1.0 / (176.0 / width))), width - 1)  evaluated in
float64, three operations in this order, and zero outside the image -- each of the three descriptors by its own window and size.
With m / o / s the model / observed / scene depth of the crop pixel and valid(d) = 100 < d < 2000:

    hidden   valid(m) and valid(s) and s <= m + tol     the pixel enters model_px and hidden_px and nothing else
    else     model, seen, inlier / front / behind as without a scene; the colours are compared at the inliers.

The depth record has the eight words of se3tn_fit with hidden_px as the last."""
import math

import numpy as np

RES = 176
SUMS = ("sum_m", "sum_o", "sum_mm", "sum_oo", "sum_mo", "sum_abs")
FIT_KEYS = ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "tol_mm", "hidden_px")


def _sources(window):
    """per crop column / row the image column / row it shows"""
    left, top, right, bottom = window
    out = []
    for first, size in ((left, right - left), (top, bottom - top)):
        inv = 1.0 / (float(RES) / float(size))
        out.append([first + min(int(math.floor(float(k) * inv)), size - 1) for k in range(RES)])
    return out


def _depth_at(rows, H, W, fy, fx):
    return rows[fy][fx] if 0 <= fy < H and 0 <= fx < W else 0


def classify(m, o, s, tol):
    """the name of the one verdict on a pixel: None (no model), 'hidden', 'unseen', 'inlier', 'front' or 'behind'"""
    if not 100 < m < 2000:
        return None
    if 100 < s < 2000 and s <= m + tol:
        return "hidden"
    if not 100 < o < 2000:
        return "unseen"
    if abs(o - m) <= tol:
        return "inlier"
    return "front" if o < m else "behind"


def record(model, observed, scene, tol):
    """(fit, colour) of one triple as dicts of Python ints (the colour sums as lists of three)"""
    (mx, my), (ox, oy), (sx, sy) = (_sources(c["window"]) for c in (model, observed, scene))
    (mH, mW), (oH, oW), (sH, sW) = (c["depth"].shape for c in (model, observed, scene))
    mdep, odep, sdep = (c["depth"].tolist() for c in (model, observed, scene))
    mrgb, orgb = model["rgb"], observed["rgb"]
    fit = dict.fromkeys(FIT_KEYS, 0)
    col = {k: [0, 0, 0] for k in SUMS}
    col["px"] = 0
    fit["tol_mm"] = col["tol_mm"] = int(tol)
    for y in range(RES):
        for x in range(RES):
            m = _depth_at(mdep, mH, mW, my[y], mx[x])
            o = _depth_at(odep, oH, oW, oy[y], ox[x])
            s = _depth_at(sdep, sH, sW, sy[y], sx[x])
            verdict = classify(m, o, s, tol)
            if verdict is None:
                continue
            fit["model_px"] += 1
            if verdict == "hidden":
                fit["hidden_px"] += 1
                continue
            if verdict == "unseen":
                continue
            fit["seen_px"] += 1
            fit[verdict + "_px"] += 1
            if verdict != "inlier":
                continue
            fit["sum_abs_mm"] += abs(o - m)
            col["px"] += 1
            pm, po = mrgb[my[y], mx[x]], orgb[oy[y], ox[x]]
            for ch in range(3):
                a, b = int(pm[ch]), int(po[ch])
                col["sum_m"][ch] += a
                col["sum_o"][ch] += b
                col["sum_mm"][ch] += a * a
                col["sum_oo"][ch] += b * b
                col["sum_mo"][ch] += a * b
                col["sum_abs"][ch] += abs(b - a)
    return fit, col


def as_arrays(se3, recs):
    """a list of record() results as the library's structured arrays (fit [n] of SCENE_CROP_FIT_DTYPE, colour [n])"""
    fit = np.zeros(len(recs), se3._lib.SCENE_CROP_FIT_DTYPE)
    col = np.zeros(len(recs), se3._lib.COLOR_FIT_DTYPE)
    for i, (f, c) in enumerate(recs):
        for k in FIT_KEYS:
            fit[k][i] = f[k]
        col["px"][i], col["tol_mm"][i] = c["px"], c["tol_mm"]
        for k in SUMS:
            col[k][i] = c[k]
    return fit, col


def counts(ms, os_, ss, tol):
    """the six counts and sum |o - m| of the rule over the product ms x os_ x ss, in the order of FIT_KEYS without tol_mm:
    what tests/c_abi/scene_verify_check.cpp prints for fit_classify_scene of csrc/fit_rule.h"""
    out = dict.fromkeys(("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "hidden_px"), 0)
    for m in ms:
        for o in os_:
            for s in ss:
                verdict = classify(m, o, s, tol)
                if verdict is None:
                    continue
                out["model_px"] += 1
                if verdict == "hidden":
                    out["hidden_px"] += 1
                elif verdict != "unseen":
                    out["seen_px"] += 1
                    out[verdict + "_px"] += 1
                    if verdict == "inlier":
                        out["sum_abs_mm"] += abs(o - m)
    return out
