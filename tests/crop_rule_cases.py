"""Cases for the crop stage's index rule at the window sizes that decide it (numpy and the oracle only: no device, no library).

crop_bbox resizes its window to 176 x 176 with cv2.resize(INTER_NEAREST), whose source index is
    sx = min(floor(x * (1.0 / (176.0 / src))), src - 1)         three float64 operations, in this order
(O.resize_nearest_indices; tests/test_opencv_rules_independent.py pins that table to the literal double evaluation for every source
size 1..2000).  Wherever x * src / 176 is an exact integer, the order of evaluation decides whether the index is `exact` or
`exact - 1`: ALTERNATIVES names four other evaluations a kernel could slide into, decisive() the sizes and crop positions at which
each of them gives another index than the rule.  A crop kernel that is run at none of those sizes has not been held to the rule.

The sweep (SWEEP_SIZES, sweep_cases()): every size 1..352 (twice the crop: where a tracker's window lives) and every decisive
size up to 2000, each once as a width and once as a height of a non-square window of ONE seeded 2048 x 2048 frame, under two
placements (inside the frame; over its left and top edge).  tests/test_crop_rule_cases.py states on the oracle alone that every case
has teeth (each alternative that differs at the case's sizes changes the oracle's crop); tests/test_gpu_crop_sizes.py runs the
device copies of the rule on the same cases."""
import functools

import numpy as np

from oracle import se3_oracle as O

DST = 176
LIMIT = 2000                      # where the CPU pin of the oracle's table stops
FRAME_HW = (2048, 2048)
FRAME_SEED, MODEL_FRAME_SEED, EDGE_SEED = 20, 21, 22
PLACEMENTS = ("inside", "edge")
CHUNKS = 4                        # ~137 cases each: above 64, so that a se3tn_preprocess call crosses CropArgs::MAX with both placements
HEIGHT_SHIFT = 131                # crop i: width SWEEP_SIZES[i], height SWEEP_SIZES[(i + HEIGHT_SHIFT) % n]
# OffsetDepth's scalar (mm): values float32 holds exactly and values it does not (the NUMPY1 rule rounds the scalar to float32 first)
Z_OFFSETS_MM = (812.5, 433.333333333, -640.25, -1234.56789, 0.1, 1999.9999, 3000.7)


def _x(dst):
    return np.arange(dst, dtype=np.int64)


def rule(dst, src):
    """the yardstick: the oracle's table"""
    return O.resize_nearest_indices(dst, src)


def _exact_integers(dst, src):
    return np.minimum((_x(dst) * src) // dst, src - 1)


def _one_division(dst, src):
    return np.minimum(np.floor(_x(dst).astype(np.float64) * np.float64(src) / np.float64(dst)).astype(np.int64), src - 1)


def _scale_first(dst, src):
    return np.minimum(np.floor(_x(dst).astype(np.float64) * (np.float64(src) / np.float64(dst))).astype(np.int64), src - 1)


def _float32(dst, src):
    ifx = np.float32(1.0 / (float(dst) / float(src)))
    prod = _x(dst).astype(np.float32) * ifx
    assert prod.dtype == np.float32
    return np.minimum(np.floor(prod).astype(np.int64), src - 1)


# name -> (dst, src) -> index table [dst].  For the precondition tests of tests/test_crop_rule_cases.py and nothing else.
ALTERNATIVES = {
    "exact_integers": _exact_integers,       # (x * src) // dst
    "one_division": _one_division,           # floor(x * src / 176.0)
    "scale_first": _scale_first,             # floor(x * (src / 176.0))
    "float32": _float32,                     # floor((float)x * (float)ifx)
}


@functools.lru_cache(maxsize=None)
def decisive(limit=LIMIT):
    """{size: {alternative: crop positions [k] at which its index differs from the rule's}} for every size 1..limit at which at
    least one alternative differs (an alternative that agrees at a size is not listed there)"""
    out = {}
    for s in range(1, limit + 1):
        want = rule(DST, s)
        diff = {}
        for name, fn in ALTERNATIVES.items():
            pos = np.nonzero(fn(DST, s) != want)[0]
            if len(pos):
                diff[name] = pos
        if diff:
            out[s] = diff
    return out


def decisive_positions(size):
    """crop positions at which any alternative differs at this size (empty if the size is not decisive)"""
    d = decisive().get(int(size), {})
    return np.unique(np.concatenate(list(d.values()))) if d else np.zeros(0, np.int64)


def _sweep_sizes():
    return tuple(sorted(set(range(1, 2 * DST + 1)) | set(decisive())))


SWEEP_SIZES = _sweep_sizes()


class Case:
    """one crop of the sweep: window sizes, both placements' windows (left, top, right, bottom) and the pre-processing parameters"""

    def __init__(self, index, width, height, windows, z_mm, stats, chunk):
        self.index, self.width, self.height, self.windows, self.stats, self.chunk = index, width, height, windows, stats, chunk
        # the tracker's descriptor carries pose z * 1000 (tracker.py), the oracle takes the pose: both see the same double
        self.pose_z = z_mm / 1000.0
        self.z_offset_mm = float(np.float64(self.pose_z) * 1000)
        self.offset_rule = ("numpy1", "numpy2")[chunk % 2]       # one context has one rule: alternates by chunk

    def pose(self):
        P = np.eye(4)
        P[2, 3] = self.pose_z
        return P

    def __repr__(self):
        return "Case(%d: %d x %d)" % (self.index, self.width, self.height)


def place(width, height, ex, ey, rng):
    """the two windows of a width x height crop: anywhere inside the frame; over the left and top edge by (ex, ey) pixels, at most
    size - 1 so that the window still touches the frame (crop_bbox, like the reference, raises on a window that misses it).  At a
    decisive size the overhang also stays below the source index of the LAST decisive position: with the seeded 1..40 alone the small
    decisive sizes (26 pixels: one decisive column, source 13) had all their decisive columns on the zero canvas, where no
    evaluation can show (the teeth test of tests/test_crop_rule_cases.py failed there), so the placement was bounded, not the case
    dropped."""
    H, W = FRAME_HW
    l, t = int(rng.integers(0, W - width + 1)), int(rng.integers(0, H - height + 1))
    ex, ey = min(ex, width - 1), min(ey, height - 1)
    px, py = decisive_positions(width), decisive_positions(height)
    if len(px):
        ex = max(1, min(ex, int(px[-1]) * width // DST - 1))
    if len(py):
        ey = max(1, min(ey, int(py[-1]) * height // DST - 1))
    return {"inside": (l, t, l + width, t + height), "edge": (-ex, -ey, width - ex, height - ey)}


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """the ~545 cases.  Chunk k is cases[k::CHUNKS]: every chunk holds small and large windows alike."""
    n = len(SWEEP_SIZES)
    rng = np.random.default_rng(EDGE_SEED)
    cases = []
    for i, w in enumerate(SWEEP_SIZES):
        h = SWEEP_SIZES[(i + HEIGHT_SHIFT) % n]
        ex, ey = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        cases.append(Case(i, w, h, place(w, h, ex, ey, rng), Z_OFFSETS_MM[i % len(Z_OFFSETS_MM)], (i // 3) & 1, i % CHUNKS))
    return tuple(cases)


def chunk(k):
    return [c for c in sweep_cases() if c.chunk == k]


@functools.lru_cache(maxsize=None)
def frame(seed=FRAME_SEED):
    """rgb uint8 [H,W,3] uniform over 0..255, depth uint16 [H,W] uniform over 0..2499: the validity thresholds 100, 101, 1999, 2000
    and the hole 0 all occur, and neighbouring pixels differ"""
    rng = np.random.default_rng(seed)
    H, W = FRAME_HW
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 2500, (H, W)).astype(np.uint16)
    rgb.setflags(write=False); depth.setflags(write=False)
    return rgb, depth


def bbox_of(window):
    """the corner array crop_bbox takes ((v, u) rows), of a window (left, top, right, bottom)"""
    l, t, r, b = window
    return np.array([[t, l], [b, l], [t, r], [b, r]], np.int32)


def oracle_crop(rgb, depth, window):
    """O.crop_bbox under a window: rgb uint8 [176,176,3], depth uint16 [176,176]"""
    return O.crop_bbox(rgb, depth, bbox_of(window), (DST, DST))


def oracle_preprocess(rgb_crop, depth_crop, case, mean, std):
    """OffsetDepth + NormalizeChannels + ToTensor of a crop: float32 [4,176,176]"""
    d = O.normalize_depth(depth_crop, case.pose(), case.offset_rule)
    s = 4 * case.stats
    return O.normalize_channels(rgb_crop.astype(np.float32), d, mean[s:s + 4], std[s:s + 4])


def crop_with_tables(rgb, depth, window, xs, ys):
    """PRECONDITION ONLY: the crop that given index tables xs, ys [176] produce -- crop_bbox restated around the tables (zero canvas
    outside the frame), so that a test can ask what an alternative evaluation would have shown.  rgb may be None (depth only)."""
    l, t, r, b = window
    H, W = depth.shape
    fx, fy = l + np.asarray(xs, np.int64), t + np.asarray(ys, np.int64)
    ok = ((fy >= 0) & (fy < H))[:, None] & ((fx >= 0) & (fx < W))[None, :]
    cy, cx = np.clip(fy, 0, H - 1), np.clip(fx, 0, W - 1)
    dep = np.where(ok, depth[cy][:, cx], 0).astype(np.uint16)
    if rgb is None:
        return None, dep
    return np.where(ok[:, :, None], rgb[cy][:, cx], 0).astype(np.uint8), dep


def alternative_crop(rgb, depth, window, name):
    """PRECONDITION ONLY: the crop under ALTERNATIVES[name] ("rule": under the oracle's table, = O.crop_bbox)"""
    l, t, r, b = window
    fn = rule if name == "rule" else ALTERNATIVES[name]
    return crop_with_tables(rgb, depth, window, fn(DST, r - l), fn(DST, b - t))


def differing(case_sizes):
    """names of the alternatives that differ at one of the given sizes"""
    d = decisive()
    return sorted({name for s in case_sizes for name in d.get(int(s), {})})


# ---- se3tn_fit_stats: pairs whose model and observed descriptors have different decisive sizes ----------------------------------
FIT_TOL = 6
FIT_PAIRS = 40


@functools.lru_cache(maxsize=None)
def fit_frames():
    """model / observed depth frames uint16 [2048,2048]: a surface of 590..610 mm per pixel (differences of -20..20 against a
    tolerance of 6: inliers, in front, behind), with holes and the validity thresholds sprinkled in.  Independent per pixel, so a crop
    shifted by one column or row has other records."""
    out = []
    for seed in (MODEL_FRAME_SEED, MODEL_FRAME_SEED + 100):
        rng = np.random.default_rng(seed)
        d = rng.integers(590, 611, FRAME_HW).astype(np.uint16)
        sel = rng.random(FRAME_HW)
        for k, v in enumerate((0, 100, 101, 1999, 2000, 65535)):
            d[(sel > 0.03 * k) & (sel < 0.03 * k + 0.02)] = v
        d.setflags(write=False)
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fit_cases():
    """FIT_PAIRS pairs (name, model window, observed window): the four sizes of a pair are four different decisive sizes (most of
    them <= 352, every fourth pair from the larger ones), the placements alternate inside / edge independently for the two"""
    d = decisive()
    small = [s for s in d if s <= 2 * DST]
    large = [s for s in d if s > 2 * DST]
    rng = np.random.default_rng(EDGE_SEED + 1)
    out = []
    for i in range(FIT_PAIRS):
        pool = large if i % 4 == 3 else small
        j = 4 * i
        mw, mh, ow, oh = (pool[(7 * (j + k) + 3 * k) % len(pool)] for k in range(4))
        ex, ey = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        m = place(mw, mh, ex, ey, rng)[PLACEMENTS[i % 2]]
        o = place(ow, oh, ey, ex, rng)[PLACEMENTS[(i // 2) % 2]]
        out.append(("fit%02d_%dx%d_%dx%d" % (i, mw, mh, ow, oh), m, o))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _no_colour():
    return np.zeros(FRAME_HW + (3,), np.uint8)


def oracle_depth_crop(depth, window):
    """O.crop_bbox's depth crop of a depth frame alone"""
    return oracle_crop(_no_colour(), depth, window)[1]


@functools.lru_cache(maxsize=None)
def _fit_expected(fit_stats):
    model, observed = fit_frames()
    return {name: fit_stats(oracle_depth_crop(model, mw), oracle_depth_crop(observed, ow), FIT_TOL) for name, mw, ow in fit_cases()}


def fit_expected(se3, name):
    """the record of a fit case: utils.fit_stats of the two oracle crops (computed once for all cases)"""
    return _fit_expected(se3.utils.fit_stats)[name]


# ---- the tracking entry points: poses whose crop window has a given decisive size -----------------------------------------------
TRACK_SIZES = (72, 84, 144, 168, 248, 288, 336)
TRACK_WIDTH_MM = 150.0


def track_cases():
    """(name, window size, image point the window is centred near) on a 480 x 640 frame: every size of TRACK_SIZES inside the frame,
    one window over the left / top edge and one over the right / bottom edge"""
    centres = ((320, 240), (205, 151), (330, 252), (420, 260), (300, 228), (322, 241), (318, 239))
    out = [("inside%d" % s, s, c) for s, c in zip(TRACK_SIZES, centres)]
    return out + [("left_top144", 144, (41, 33)), ("right_bottom248", 248, (561, 402))]


def window_of(pose, K, width_mm=TRACK_WIDTH_MM):
    bb = O.compute_bbox(pose, K, width_mm, (1000, 1000, 1000))
    return (int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max()))


def find_pose(size, K, centre_px, width_mm=TRACK_WIDTH_MM, seed=3):
    """a pose (rotation of fixtures.pose(seed)) whose crop window under O.compute_bbox is size x size pixels and centred near the
    image point centre_px = (u, v): z from the pinhole relation, then a scan of nearby z and sub-pixel shifts until the rounded
    corners give the size on both axes"""
    from oracle import fixtures as Fx
    z0 = width_mm * K[0, 0] / size / 1000.0
    for dz in np.arange(0, 400) * (z0 * 2e-4) * np.resize([1, -1], 400):
        z = z0 + dz
        for du in (0.0, 0.3, 0.6):
            for dv in (0.0, 0.3, 0.6):
                x = (centre_px[0] + du - K[0, 2]) * z / K[0, 0]
                y = (centre_px[1] + dv - K[1, 2]) * z / K[1, 1]
                P = Fx.pose(seed, (x, y, z))
                l, t, r, b = window_of(P, K, width_mm)
                if r - l == size and b - t == size:
                    return P
    raise AssertionError("no pose found for a %d-pixel window at %s" % (size, (centre_px,)))
