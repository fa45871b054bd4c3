"""The rule of se3tn_scene_stats as a per-pixel Python loop (a helper module: no numpy arithmetic on images, no device): what
utils.scene_stats and the kernel are held to, word for word."""
import numpy as np

FIELDS = ("model_px", "visible_px", "hidden_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "hidden_by", "tol_mm", "n_objects")


def valid(d):
    return 100 < d < 2000


def scene_stats(layers, rects, observed, tol):
    """-> (list of n dicts with FIELDS, ids [H][W], scene [H][W]) as Python ints"""
    obs = np.asarray(observed).tolist()
    H, W = len(obs), len(obs[0])
    n = len(rects)
    lay = [None if l is None else np.asarray(l).tolist() for l in layers]
    rec = [dict.fromkeys(FIELDS, 0) for _ in range(n)]
    ids = [[0] * W for _ in range(H)]
    scene = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            m = []
            for i, (x0, y0, x1, y1) in enumerate(rects):
                m.append(lay[i][y - y0][x - x0] if (x0 <= x < x1 and y0 <= y < y1) else 0)
            owner = -1
            for i in range(n):
                if valid(m[i]) and (owner < 0 or m[i] < m[owner]):
                    owner = i
            if owner >= 0:
                ids[y][x], scene[y][x] = owner + 1, m[owner]
            o = obs[y][x]
            for i in range(n):
                if not valid(m[i]):
                    continue
                r = rec[i]
                r["model_px"] += 1
                if owner != i:
                    r["hidden_px"] += 1
                    r["hidden_by"] |= 1 << owner
                    continue
                r["visible_px"] += 1
                if not valid(o):
                    continue
                r["seen_px"] += 1
                d = o - m[i]
                if abs(d) <= tol:
                    r["inlier_px"] += 1
                    r["sum_abs_mm"] += abs(d)
                elif d < 0:
                    r["front_px"] += 1
                else:
                    r["behind_px"] += 1
    for r in rec:
        r["tol_mm"], r["n_objects"] = tol, n
    return rec, ids, scene


def as_array(se3, rec):
    out = np.zeros(len(rec), se3._lib.SCENE_FIT_DTYPE)
    for i, r in enumerate(rec):
        for k in FIELDS:
            out[k][i] = r[k]
    return out
