"""The texture filter of the full-frame renderer in float64, with a derived per-pixel bound (TEST INFRASTRUCTURE ONLY).

What is stated here is the `a.mode == 1 && a.tex` branch of raster_resolve_kernel (csrc/raster.hip) from the point where the
float32 texture coordinates exist.  Their arithmetic (ss_rules.interpolate) is pinned bit for bit by the byte equality of depth and
vertex colours; the filter is what starts after it:

  inputs    (u, v) float32 at the pixel, and at the three corners (xq, yq), (xq + 1, yq), (xq, yq + 1) of its 2 x 2 quad
            (xq = x & ~1, yq = y & ~1, window coordinates), all on the winning triangle's planes
  rho       dx = (q1 - q0) * (tw, th),  dy = (q2 - q0) * (tw, th),  rho = fmax(|dx|, |dy|)
  lod       fmin(fmax(log2(fmax(rho, 1e-8)), 0), levels - 1) with C's fmaxf / fminf: a NaN operand yields the OTHER operand.
            A quad corner extrapolated across w = 0 on a near-clipped triangle can make rho NaN or inf: NaN -> 1e-8 -> lod 0,
            inf -> the top level.  (Python's max / min chain of ss_rules.render_frame raises on a NaN rho.)
  sample    level l is max(tw >> l, 1) x max(th >> l, 1); image row 0 is the TOP, v = 0 the bottom: x = u w - 0.5,
            y = (1 - v) h - 0.5; x0 = floor(x) mod w, x1 = (x0 + 1) mod w (REPEAT on both axes, negative indices wrapped),
            bilinear weights ax = x - floor(x), ay likewise
  blend     l0 = floor(lod), l1 = min(l0 + 1, levels - 1), c = c0 + (lod - l0) (c1 - c0);  c / 255 * kd, clamped to [0, 1]

`evaluate` returns that real value c per channel and a half-width delta: a CORRECT float32 evaluation of the same statement, in any
order of operations that does not change the formulas, lies in [c - delta, c + delta].  The filter is continuous in u, v and lod
(bilinear and trilinear interpolation, REPEAT), so a float32 evaluation whose floor() falls on the other side of a texel or level
boundary still lies within (error of the argument) x (slope).  delta is the sum of four terms, in texture units 0..255 until the last
line (ulp(z): spacing of float32 at |z|; every f32 operation is correctly rounded, error <= ulp / 2 of its result):

  1. coordinates.  x = u w - 0.5: the product and the difference round once each, and ax = x - floor(x) rounds when x is a tiny
     negative number (<= 2^-25): |dx| <= 1.5 ulp(max(|u w|, |x|, 1)).  y = (1 - v) h - 0.5: 1 - v rounds (<= ulp(1 - v) / 2, times h:
     <= ulp((1 - v) h)), then as x: |dy| <= 2.5 ulp(max(|(1 - v) h|, |y|, 1)).  The bilinear surface changes by at most
     sx |dx| + sy |dy| + |t00 - t10 - t01 + t11| |dx| |dy| with sx = max(|t10 - t00|, |t11 - t01|), sy = max(|t01 - t00|, |t11 - t10|)
     the texel differences of the cell -- and where ax (ay) is within |dx| (|dy|) of 0 or 1, so that the evaluation may sit in the
     neighbouring cell, the slope is taken as 255.  Per level; the two levels combine with the weights (1 - fl), fl.
  2. lod.  rho: per component a difference, a product with tw / th and a square (3 roundings: relative 2^-24 each, doubled by the
     square except its own: 5 x 2^-24 on the square), one sum (6 x 2^-24), sqrtf correctly rounded (halves the argument's error, adds
     one rounding): relative 4 x 2^-24 on rho, i.e. 4 x 2^-24 / ln 2 on log2 rho.  log2f is within 1 ulp of its result (ROCm math
     documentation): ulp(max(|lod|, 1)) bounds that on the clamped range.  lod - l0 is exact.  e_lod = 4 x 2^-24 / ln 2 + ulp(max(lod, 1));
     the colour changes by e_lod |c1 - c0| -- and by e_lod 255 where lod is within e_lod of an integer (the neighbouring pair of levels).
  3. blends.  Per sample: 1 - ax, two products and a sum per row (the rows weigh (1 - ay), ay: 4 roundings between them), 1 - ay,
     two products, the sum: 8 roundings; the samples weigh (1 - fl), fl: 8 between them; c1 - c0, its product with fl, the sum: 3;
     the product with 1 / 255 and the rounding of that constant: 2.  13 roundings of values <= 255, each <= ulp(255) / 2 = 2^-17.
  4. kd.  Everything above scales by kd / 255; the product with kd rounds once: ulp(c kd) / 2.

The admissible bytes of a pixel are unorm8(c - delta) .. unorm8(c + delta) with ss_rules.unorm8 (the truncated 16-bit rule, its own
float32 product included: unorm8 is monotone, so it maps the interval's ends to the ends of the byte range).  Nothing in delta is
fitted to any implementation's output.

Assumes |x|, |y| < 2^31 (the kernel converts floor(x) to int)."""
import numpy as np

from . import raster_oracle as R
from . import ss_rules as S

f32, f64 = np.float32, np.float64
TWO_BYTE_CAP = 0.10        # a cap that keeps the interval check from degenerating into "+-1 everywhere"; not a measurement
N_BLEND_ROUNDINGS = 13
HALF_ULP_255 = 2.0 ** -17


def ulp32(z):
    """spacing of float32 at |z| (z float64 array)"""
    return np.spacing(np.abs(np.asarray(z, f64)).astype(f32)).astype(f64)


# ---- the filter's inputs: float32 uv at every covered pixel and at its quad corners --------------------------------------------------
def gather(vertices, faces, uv, ob2cam, K, W, H):
    """Coverage, depth and ownership by the rules (ss_rules.rasterize, as ss_rules.render_frame does it), then per covered pixel the
    float32 uv ss_rules.interpolate gives at the pixel and at its three quad corners.  Window rows count bottom-up; `rows` are the
    image rows after the read-back flip.  Returns dict(rows, cols, uv [n,2], q [n,3,2], wq [n,3] (the interpolated 1/w plane at the
    corners, before the reciprocal: <= 0 or not finite where a corner lies across w = 0), tri [n])."""
    PV = S.frame_pv(ob2cam, K, W, H)
    v32 = np.asarray(vertices, f32)
    pv = S.project(S.clip_positions(v32, PV), W, H)
    _, owner, setups = S.rasterize(pv, faces, W, H)
    uv32 = np.asarray(uv, f32)
    out = dict(rows=[], cols=[], uv=[], q=[], wq=[], tri=[])
    for t, s in setups.items():
        ys, xs = np.nonzero(owner == t)
        if len(ys) == 0:
            continue
        uvt = uv32[s.idx]
        xq, yq = xs // 2 * 2, ys // 2 * 2
        corners = [(xq, yq), (xq + 1, yq), (xq, yq + 1)]
        out["rows"].append(H - 1 - ys); out["cols"].append(xs); out["tri"].append(np.full(len(ys), t))
        out["uv"].append(S.interpolate(s, uvt, xs, ys))
        out["q"].append(np.stack([S.interpolate(s, uvt, cx, cy) for cx, cy in corners], 1))
        Pw = ((s.M[0] + s.M[1]).astype(f32) + s.M[2]).astype(f32)
        with np.errstate(all="ignore"):
            out["wq"].append(np.stack([S._plane_eval(Pw, *S._quad_coords(cx, cy, s.dx, s.dy)) for cx, cy in corners], 1))
    return {k: np.concatenate(v) for k, v in out.items()}


# ---- the filter in float64 ------------------------------------------------------------------------------------------------------------
def level_of_detail(q, tw, th, nlev):
    """q [n,3,2] float32 -> (lod [n] float64 in [0, nlev - 1], rho [n]); fmaxf / fminf semantics (np.fmax / np.fmin)"""
    q = np.asarray(q, f32).astype(f64)
    with np.errstate(all="ignore"):
        size = np.array([tw, th], f64)
        dx, dy = (q[:, 1] - q[:, 0]) * size, (q[:, 2] - q[:, 0]) * size
        rho = np.fmax(np.sqrt((dx * dx).sum(1)), np.sqrt((dy * dy).sum(1)))
        lod = np.fmin(np.fmax(np.log2(np.fmax(rho, 1e-8)), 0.0), float(nlev - 1))
    return lod, rho


def bilinear(level, u, v):
    """level uint8 [h,w,3]; u, v float64 [n] -> (c [n,3], bound of term 1 [n,3]) in texture units"""
    h, w = level.shape[:2]
    t = level.astype(f64)
    uw, vh = u * w, (1.0 - v) * h
    x, y = uw - 0.5, vh - 0.5
    xf, yf = np.floor(x), np.floor(y)
    ax, ay = (x - xf)[:, None], (y - yf)[:, None]
    x0, y0 = np.mod(xf, w).astype(np.int64), np.mod(yf, h).astype(np.int64)
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    t00, t10, t01, t11 = t[y0, x0], t[y0, x1], t[y1, x0], t[y1, x1]
    c = (t00 * (1 - ax) + t10 * ax) * (1 - ay) + (t01 * (1 - ax) + t11 * ax) * ay
    ex = (1.5 * ulp32(np.maximum(np.maximum(np.abs(uw), np.abs(x)), 1.0)))[:, None]
    ey = (2.5 * ulp32(np.maximum(np.maximum(np.abs(vh), np.abs(y)), 1.0)))[:, None]
    sx = np.where((ax < ex) | (ax > 1 - ex), 255.0, np.maximum(np.abs(t10 - t00), np.abs(t11 - t01)))
    sy = np.where((ay < ey) | (ay > 1 - ey), 255.0, np.maximum(np.abs(t01 - t00), np.abs(t11 - t10)))
    return c, sx * ex + sy * ey + np.abs(t00 - t10 - t01 + t11) * ex * ey


def evaluate(levels, kd, uv, q):
    """levels: raster_oracle.mip_pyramid(texture); kd [3] or None; uv [n,2], q [n,3,2] float32.
    Returns (c [n,3] float64 in [0, 1], delta [n,3] float64, aux dict(lod, rho, l0))."""
    nlev = len(levels)
    th, tw = levels[0].shape[:2]
    kd = np.asarray((1.0, 1.0, 1.0) if kd is None else kd, f32).astype(f64)
    uv = np.asarray(uv, f32).astype(f64)
    lod, rho = level_of_detail(q, tw, th, nlev)
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, nlev - 1)
    fl = (lod - l0)[:, None]
    n = len(uv)
    c0, c1, d0, d1 = (np.zeros((n, 3)) for _ in range(4))
    for l in range(nlev):
        for idx, c, d in ((l0, c0, d0), (l1, c1, d1)):
            m = idx == l
            if m.any():
                c[m], d[m] = bilinear(levels[l], uv[m, 0], uv[m, 1])
    c255 = c0 + fl * (c1 - c0)
    e_lod = (4 * 2.0 ** -24 / np.log(2.0) + ulp32(np.maximum(lod, 1.0)))[:, None]
    near_level = (fl < e_lod) | (fl > 1 - e_lod)
    d255 = (1 - fl) * d0 + fl * d1 + e_lod * np.where(near_level, 255.0, np.abs(c1 - c0)) + N_BLEND_ROUNDINGS * HALF_ULP_255
    ck = c255 / 255.0 * kd
    delta = d255 / 255.0 * kd + 0.5 * ulp32(ck)
    return np.clip(ck, 0.0, 1.0), delta, dict(lod=lod, rho=rho, l0=l0)


def admissible(c, delta):
    """byte range (lo, hi, nearest) of every pixel-channel"""
    return S.unorm8(c - delta), S.unorm8(c + delta), S.unorm8(c)


class Expect:
    """What the full-frame render of a textured mesh may show: lo / hi / nearest [H,W,3] uint8 (background 0), covered [H,W] bool,
    and per covered pixel (rows, cols order of `g`) the filter's inputs and intermediate values."""

    def __init__(self, vertices, faces, uv, texture, kd, ob2cam, K, W, H):
        self.g = g = gather(vertices, faces, uv, ob2cam, K, W, H)
        self.levels = R.mip_pyramid(texture)
        self.c, self.delta, self.aux = evaluate(self.levels, kd, g["uv"], g["q"])
        lo, hi, nearest = admissible(self.c, self.delta)
        self.covered = np.zeros((H, W), bool)
        self.covered[g["rows"], g["cols"]] = True
        self.lo, self.hi, self.nearest = (np.zeros((H, W, 3), np.uint8) for _ in range(3))
        self.lo[g["rows"], g["cols"]], self.hi[g["rows"], g["cols"]], self.nearest[g["rows"], g["cols"]] = lo, hi, nearest
        for a in (self.covered, self.lo, self.hi, self.nearest):
            a.setflags(write=False)


def check(rgb, expect, name):
    """rgb uint8 [H,W,3] against Expect: every covered pixel-channel in its admissible set, no set of more than two bytes, at most
    TWO_BYTE_CAP of the covered pixel-channels with two.  Prints and returns (covered pixels, two-byte share, not-nearest share)."""
    e, g = expect, expect.g
    rgb = np.asarray(rgb)
    assert rgb.shape == e.lo.shape and rgb.dtype == np.uint8, (name, rgb.shape, rgb.dtype)
    cov = e.covered
    n = int(cov.sum())
    width = e.hi[cov].astype(int) - e.lo[cov].astype(int)
    two = float((width >= 1).mean()) if n else 0.0
    off = float((rgb[cov] != e.nearest[cov]).mean()) if n else 0.0
    print("%s: %d covered pixels, two admissible bytes on %.4f of the pixel-channels, not the nearest byte on %.4f"
          % (name, n, two, off))
    assert n > 0, name
    assert width.max() <= 1, (name, "a set holds more than two bytes", int(width.max()))
    assert two <= TWO_BYTE_CAP, (name, "two-byte share", two)
    got = rgb[g["rows"], g["cols"]].astype(int)
    lo, hi = e.lo[g["rows"], g["cols"]].astype(int), e.hi[g["rows"], g["cols"]].astype(int)
    bad = (got < lo) | (got > hi)
    if bad.any():
        k, ch = [int(i[0]) for i in np.nonzero(bad)]
        lev = e.levels[int(e.aux["l0"][k])]
        h, w = lev.shape[:2]
        u, v = float(g["uv"][k, 0]), float(g["uv"][k, 1])
        cell = (int(np.floor(u * w - 0.5)) % w, int(np.floor((1 - v) * h - 0.5)) % h)
        raise AssertionError("%s: %d of %d pixel-channels outside their admissible set; first: row %d col %d channel %d triangle %d "
                             "got %d, admissible %d..%d (c %.6f +- %.2e), uv (%.7g, %.7g), rho %.6g lod %.6f, level %d (%d x %d) cell %s"
                             % (name, int(bad.sum()), bad.size, g["rows"][k], g["cols"][k], ch, g["tri"][k], got[k, ch], lo[k, ch],
                                hi[k, ch], e.c[k, ch] * 255, e.delta[k, ch] * 255, u, v, e.aux["rho"][k], e.aux["lod"][k],
                                int(e.aux["l0"][k]), h, w, cell))
    return n, two, off
