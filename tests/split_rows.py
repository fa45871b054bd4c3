"""The split-row storage of SE3TN_PREC_F16X3, restated for the tests (torch + numpy, no GPU and no library call).

The storage rule, from the source:
  * csrc/mfma_common.h:174 split_byte_off: channels c .. c+3 of pixel `pix` of a map with `ld` float32 words per pixel start at byte
    4 pix ld + 128 (c >> 5) + 2 (c & 31).  A map [n,H,W,C] of float32 words therefore holds, per pixel, C / 32 chunks of 128 bytes, the
    bytes a float32 chunk of 32 channels takes: 32 f16 `hi` halves, then 32 f16 `lo` halves.
  * csrc/mfma_common.h:185 store_split4: hi = f16(x), lo = f16(x - f32(hi)), both round to nearest even, stored at the offset above and
    64 bytes further on.  |x| <= 65000 or the caller raises the overflow flag.
  * csrc/mfma_common.h:177 load_split4: the value read back is f32(hi) + f32(lo).
  * csrc/kernels_misc.hip:16 split_pixel: a network-input pixel (R, G, B, D) holds 4 f16 hi | 4 f16 lo in its 16 bytes, same arithmetic.

Facts the tests lean on (tests/test_split_rows_host.py checks them on 10^7 values over 1e-6 .. 65000 and the special values):
f32(hi) + f32(lo) is exact in float32; |lo| <= ulp_f16(hi) / 2; the decoded value is within 2^-22 relative of x for |x| >= 2^-3 and within
2^-25 absolute below that.  Splitting a decoded value again does NOT give the same halves (signs of zero, subnormals): no invariant."""
import numpy as np
import torch

CHUNK = 32                  # channels per chunk of a split row
REL_BOUND = 2.0 ** -22      # |decode(encode(x)) - x| <= REL_BOUND |x|   for |x| >= REL_FROM
ABS_BOUND = 2.0 ** -25      #                          <= ABS_BOUND       below
REL_FROM = 2.0 ** -3


# ---- reading ---------------------------------------------------------------------------------------------------------------------------
def _halves(t, width):
    """(hi, lo) float16 views of a float32 word tensor [..., C]: `width` halves of hi, then `width` of lo, over and over; each [..., C]"""
    assert t.dtype == torch.float32 and t.shape[-1] * 2 % (2 * width) == 0, (t.dtype, tuple(t.shape))
    h = t.contiguous().view(torch.float16)
    h = h.reshape(t.shape[:-1] + (t.shape[-1] * 2 // (2 * width), 2, width))
    return h[..., 0, :].reshape(t.shape), h[..., 1, :].reshape(t.shape)


def map_halves(t):
    """(hi, lo) of a split map [n,H,W,C] (C % 32 == 0), float16 [n,H,W,C] each"""
    return _halves(t, CHUNK)


def pixel_halves(t):
    """(hi, lo) of split input pixels [n,H,W,4], float16 [n,H,W,4] each"""
    return _halves(t, 4)


def decode_map(t):
    """split map of float32 words [n,H,W,C] -> the float32 values it stores, same shape: float(hi) + float(lo) (CPU or CUDA tensor)"""
    hi, lo = map_halves(t)
    return hi.float() + lo.float()


def decode_pixels(t):
    """split input pixels [n,H,W,4] (`inA` / `inB`) -> float32 [n,H,W,4]"""
    hi, lo = pixel_halves(t)
    return hi.float() + lo.float()


# ---- writing (numpy: astype(float16) rounds to nearest even and keeps subnormals) --------------------------------------------------------
def split(x):
    """float32 array -> (hi, lo) float16 arrays: store_split4's arithmetic"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _encode(x, width):
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape[-1] % width == 0, x.shape
    hi, lo = split(x)
    g = x.shape[:-1] + (x.shape[-1] // width, 1, width)
    both = np.concatenate([hi.reshape(g), lo.reshape(g)], axis=-2)     # [..., chunks, 2, width]
    return np.ascontiguousarray(both).reshape(x.shape[:-1] + (2 * x.shape[-1],)).view(np.float32)


def encode_map(x):
    """float32 values [..., C] (C % 32 == 0) -> the float32 words of their split rows, same shape"""
    return _encode(x, CHUNK)


def encode_pixels(x):
    """float32 pixels [..., 4] -> the float32 words of split_pixel, same shape"""
    return _encode(x, 4)


# ---- the invariant of a stored pair ---------------------------------------------------------------------------------------------------
def _ulp_f16(hi):
    """ulp of each float16 as float32: 2^(e - 10) for a normal 2^e <= |hi| < 2^(e+1), 2^-24 for zero and subnormals; built from the
    exponent field (inf / NaN: a finite number, the caller tests finiteness itself)"""
    field = (hi.contiguous().view(torch.int16).to(torch.int32) >> 10) & 31
    k = torch.clamp(field, min=1) - 25                                 # 2^k, k = -24 .. 6
    return ((k + 127) << 23).view(torch.float32)


def ill_formed(hi, lo):
    """bool tensor: the (hi, lo) pairs no split store can have written -- a half that is not finite, |lo| > ulp_f16(hi) / 2, or
    f32(hi) + f32(lo) not exact in float32 (TwoSum's error term)"""
    a, b = hi.float(), lo.float()
    bad = ~(torch.isfinite(a) & torch.isfinite(b))
    bad |= b.abs() > 0.5 * _ulp_f16(hi)
    s = a + b
    bb = s - a
    bad |= ((a - (s - bb)) + (b - bb)) != 0
    return bad


def well_formed(t, pixels=False):
    """True when every (hi, lo) pair of the split map [n,H,W,C] (pixels: of the split input pixels [n,H,W,4]) is one a split store
    writes: see ill_formed.  An all-zero word (borders) is well formed."""
    hi, lo = pixel_halves(t) if pixels else map_halves(t)
    return not bool(ill_formed(hi, lo).any())


def count_ill_formed(t, pixels=False):
    hi, lo = pixel_halves(t) if pixels else map_halves(t)
    return int(ill_formed(hi, lo).sum())
