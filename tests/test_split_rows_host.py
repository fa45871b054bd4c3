"""CPU: tests/split_rows.py, the tests' statement of the f16x3 split-row storage, against its own bounds and against library code.

  * encode then decode on 10^7 values over 1e-6 .. 65000 and the special values: the documented bounds, and well_formed;
  * the decode applied to the split weight panels of se3tn_split_weights_host (the same [32 hi | 32 lo] rows, written by the library's
    host code): times the panel's per-cout 2^-k it gives back the packed float32 panel; the stem's 4 | 4 entries likewise;
  * well_formed rejects what a wrong store would leave: swapped halves, the neighbouring channel's lo, a NaN half."""
import numpy as np
import pytest
import torch

import split_rows as SR
from oracle import se3_oracle as O

SPECIALS = np.array([0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 65000.0, -65000.0, -2.0 ** -14, 2.0 ** -3,
                     np.nextafter(np.float32(2.0 ** -3), np.float32(0)), 1.0, 2048.0, 2049.0, 1e-6, -1e-6], np.float32)


@pytest.fixture(scope="module")
def values():
    """10^7 float32 values, log-uniform in magnitude over 1e-6 .. 65000, both signs, and the special values; a multiple of 32 long"""
    rng = np.random.default_rng(11)
    n = 10 ** 7
    x = np.exp(rng.uniform(np.log(1e-6), np.log(65000.0), n)).astype(np.float32)
    x = np.minimum(x, np.float32(65000.0)) * np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    x = np.concatenate([x, SPECIALS])
    return np.concatenate([x, np.zeros(-len(x) % 32, np.float32)])


def _check_bounds(x, got):
    assert got.dtype == np.float32 and got.shape == x.shape
    err = np.abs(got.astype(np.float64) - x.astype(np.float64))
    big = np.abs(x) >= SR.REL_FROM
    assert (err[big] <= SR.REL_BOUND * np.abs(x[big]).astype(np.float64)).all(), float((err[big] / np.abs(x[big])).max())
    assert (err[~big] <= SR.ABS_BOUND).all(), float(err[~big].max())


def test_encode_then_decode_meets_the_bounds_and_is_well_formed(values):
    x = values.reshape(1, 1, -1, 32)
    words = SR.encode_map(x)
    assert words.dtype == np.float32 and words.shape == x.shape
    t = torch.from_numpy(words)
    _check_bounds(x, SR.decode_map(t).numpy())
    assert SR.well_formed(t)
    # the facts behind well_formed, in float64: the float32 sum is the exact sum, |lo| <= ulp(hi) / 2
    hi, lo = SR.split(x)
    exact = hi.astype(np.float64) + lo.astype(np.float64)
    assert (SR.decode_map(t).numpy().astype(np.float64) == exact).all()
    a = np.abs(hi.astype(np.float64))
    ulp = np.where(a < 2.0 ** -14, 2.0 ** -24, 2.0 ** (np.floor(np.log2(np.where(a > 0, a, 1.0))) - 10))
    assert (np.abs(lo.astype(np.float64)) <= ulp / 2).all()
    # the layout: chunk by chunk 32 hi halves, then 32 lo halves
    h = words.view(np.float16).reshape(-1, 2, 32)
    assert (h[:, 0].view(np.uint16) == hi.reshape(-1, 32).view(np.uint16)).all()
    assert (h[:, 1].view(np.uint16) == lo.reshape(-1, 32).view(np.uint16)).all()


def test_pixels_encode_then_decode(values):
    x = values.reshape(1, 1, -1, 4)
    words = SR.encode_pixels(x)
    t = torch.from_numpy(words)
    _check_bounds(x, SR.decode_pixels(t).numpy())
    assert SR.well_formed(t, pixels=True)
    hi, lo = SR.split(x)
    h = words.view(np.float16).reshape(-1, 2, 4)
    assert (h[:, 0].view(np.uint16) == hi.reshape(-1, 4).view(np.uint16)).all()
    assert (h[:, 1].view(np.uint16) == lo.reshape(-1, 4).view(np.uint16)).all()
    # the same values, one pixel per 16 bytes or one chunk per 128: the same decoded numbers
    assert (SR.decode_pixels(t).numpy().reshape(-1).view(np.uint32) ==
            SR.decode_map(torch.from_numpy(SR.encode_map(values.reshape(1, 1, -1, 32)))).numpy().reshape(-1).view(np.uint32)).all()


def test_resplitting_a_decoded_value_is_no_invariant():
    """why well_formed does not re-encode: x = -0 is stored as (hi, lo) = (-0, +0) and decodes to +0, which splits to (+0, +0)"""
    x = np.zeros((1, 1, 1, 32), np.float32)
    x[..., 0] = -0.0
    x[..., 1] = np.float32(1.0) + np.float32(2.0 ** -13)       # lo = 2^-13; decoded exactly, re-split identically
    x[..., 2] = np.float32(2.0 ** -25) * np.float32(-1.0)      # half the smallest subnormal: hi = -0
    w = SR.encode_map(x)
    again = SR.encode_map(SR.decode_map(torch.from_numpy(w)).numpy())
    assert SR.well_formed(torch.from_numpy(w)) and SR.well_formed(torch.from_numpy(again))
    assert (w.view(np.uint32) != again.view(np.uint32)).any()


# ---- the helper against library code --------------------------------------------------------------------------------------------------
# csrc/infer_plan.h conv_specs: (cin, cout, groups) of the ten 3x3 convs; csrc/se3tn_internal.h blob_layout / split_layout: a 64-word
# header (blob only), the two stems [64][204] and their [64] vectors, then per conv its groups' panels followed by cout x groups words
# (bias | per-cout 2^-k) -- every section is as long in the split buffer as in the blob
SPECS = [(64, 64, 2), (64, 64, 2), (64, 64, 1), (64, 64, 1), (128, 256, 1), (256, 256, 1), (256, 256, 1), (256, 1024, 1), (512, 512, 2),
         (512, 512, 2)]
HEADER, STEM = 64, 64 * 204


def _conv_sections(i):
    """(word offset of conv i's first panel, of its per-cout vectors) in the split buffer; the blob's are HEADER further on"""
    o = 2 * STEM + 2 * 64
    for cin, cout, groups in SPECS[:i]:
        o += 9 * cin * cout * groups + cout * groups
    cin, cout, groups = SPECS[i]
    return o, o + 9 * cin * cout * groups


@pytest.fixture(scope="module")
def panels():
    """packed float32 blob and split buffer (float32 words) of a state dict with the awkward rows of
    test_f16x3_split_panels_derived_on_device_equal_host_statement: a dead cout, a power-of-two maximum, a 1e-6 and a 1e5 row"""
    import se3tracknet_amd as se3
    eng = se3.Engine(device=-1, max_batch=1)       # host-only context
    sd = O.make_state_dict(7)
    w = sd["trans_conv2.conv1.weight"].clone()
    w[3] = 0; w[4] *= 1e-3; w[4, 0, 0, 0] = 4.0; w[5] *= 1e-6; w[6] *= 1e5
    sd["trans_conv2.conv1.weight"] = w
    for k in ("weight", "bias", "running_mean", "running_var"):      # identity BN: the rows reach the panel as they are
        sd["trans_conv2.bn1." + k] = torch.ones(512) if k == "weight" else torch.zeros(512)
    sd["trans_conv2.bn1.running_var"] = torch.ones(512) - 1e-5
    blob = eng.pack_state_dict(sd)
    split = eng.split_weights_host(blob)
    return blob.numpy().view(np.float32), split.numpy().view(np.float32)


@pytest.mark.parametrize("conv,group", [(8, 0), (8, 1), (4, 0), (0, 1)], ids=["trans_conv2.conv1", "rot_conv2.conv1", "convAB1", "convB2.conv1"])
def test_decoded_split_panel_times_its_scale_is_the_packed_panel(panels, conv, group):
    blob, split = panels
    cin, cout, groups = SPECS[conv]
    words = 9 * cin * cout
    ws, sc = _conv_sections(conv)
    # [chunk][tap][cout][32 f16 hi | 32 f16 lo]: one chunk per row, the layout of a map with C = 32
    rows = torch.from_numpy(split[ws + group * words: ws + (group + 1) * words].copy()).reshape(1, cin // 32 * 9, cout, 32)
    assert SR.well_formed(rows)
    scale = split[sc + group * cout: sc + (group + 1) * cout]
    assert (np.log2(scale) == np.round(np.log2(scale))).all()                       # exact powers of two
    got = SR.decode_map(rows).numpy()[0].astype(np.float64) * scale.astype(np.float64)[None, :, None]
    want = blob[HEADER + ws + group * words: HEADER + ws + (group + 1) * words].reshape(cin // 32 * 9, cout, 32).astype(np.float64)
    row_max = np.abs(want).max((0, 2))
    err = np.abs(got - want).max((0, 2))
    assert (err <= SR.REL_BOUND * row_max).all(), (int((err / np.where(row_max > 0, row_max, 1)).argmax()), float((err / np.where(row_max > 0, row_max, 1)).max()))
    if conv == 8 and group == 0:    # the awkward rows are what they were meant to be
        med = float(np.median(row_max))
        assert row_max[3] == 0 and err[3] == 0 and row_max[4] == 4.0 and row_max[5] < 1e-5 * med and row_max[6] > 1e4 * med
        assert scale[3] == 1.0 and scale[4] == 2.0 ** -8


@pytest.mark.parametrize("branch", [0, 1])
def test_decoded_split_stem_entries_times_their_scale_are_the_packed_stem(panels, branch):
    """the stem's weights: 16-byte entries of 4 f16 hi | 4 f16 lo, the layout of the split input pixels"""
    blob, split = panels
    ent = torch.from_numpy(split[branch * STEM: (branch + 1) * STEM].copy()).reshape(1, 64, 51, 4)
    assert SR.well_formed(ent, pixels=True)
    scale = split[2 * STEM + branch * 64: 2 * STEM + (branch + 1) * 64].astype(np.float64)
    got = SR.decode_pixels(ent).numpy()[0].astype(np.float64).reshape(64, 204) * scale[:, None]
    want = blob[HEADER + branch * STEM: HEADER + (branch + 1) * STEM].reshape(64, 204).astype(np.float64)
    row_max = np.abs(want).max(1)
    assert row_max.min() > 0
    assert (np.abs(got - want).max(1) <= SR.REL_BOUND * row_max).all()


# ---- what well_formed must reject -------------------------------------------------------------------------------------------------------
def _map():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 5, 5, 64)) * 3).astype(np.float32)
    x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0        # a zero border, as the activations carry
    return x, SR.encode_map(x)


def test_well_formed_rejects_swapped_halves_a_neighbours_lo_and_nan():
    x, words = _map()
    assert SR.well_formed(torch.from_numpy(words))
    h = words.view(np.float16).reshape(2, 5, 5, 2, 2, 32)             # [n,H,W,chunk,hi|lo,32]
    # one swapped (hi, lo) pair
    bad = h.copy()
    bad[1, 2, 3, 1, 0, 7], bad[1, 2, 3, 1, 1, 7] = h[1, 2, 3, 1, 1, 7], h[1, 2, 3, 1, 0, 7]
    t = torch.from_numpy(bad.reshape(2, 5, 5, 128).view(np.float32))
    assert not SR.well_formed(t) and SR.count_ill_formed(t) == 1
    # the lo halves of one pixel's chunk taken from the neighbouring channel
    bad = h.copy()
    bad[0, 1, 1, 0, 1, :] = np.roll(h[0, 1, 1, 0, 1, :], 1)
    t = torch.from_numpy(bad.reshape(2, 5, 5, 128).view(np.float32))
    assert not SR.well_formed(t)
    # the whole lo plane of a chunk read from the other chunk
    bad = h.copy()
    bad[:, :, :, 0, 1] = h[:, :, :, 1, 1]
    assert not SR.well_formed(torch.from_numpy(bad.reshape(2, 5, 5, 128).view(np.float32)))
    # a NaN / an infinite half, in hi or in lo
    for half in (0, 1):
        for v in (np.nan, np.inf):
            bad = h.copy()
            bad[0, 3, 2, 1, half, 0] = v
            assert not SR.well_formed(torch.from_numpy(bad.reshape(2, 5, 5, 128).view(np.float32))), (half, v)
    # the same for pixels
    px = SR.encode_pixels(x[..., :4] + 1.0)
    assert SR.well_formed(torch.from_numpy(px), pixels=True)
    p = px.view(np.float16).copy().reshape(2, 5, 5, 2, 4)
    p[0, 0, 0, 0, 1], p[0, 0, 0, 1, 1] = p[0, 0, 0, 1, 1], p[0, 0, 0, 0, 1]
    assert not SR.well_formed(torch.from_numpy(p.reshape(2, 5, 5, 8).view(np.float32)), pixels=True)
    # split input pixels read as if they were chunks of a map: the wrong layout does not pass either
    assert not SR.well_formed(torch.from_numpy(px.reshape(-1)[:192].reshape(1, 1, 6, 32).copy()))


def test_a_zeroed_lo_half_is_well_formed_but_off_by_up_to_half_an_f16_ulp():
    """what well_formed cannot see and the float64 stage comparison must: lo = 0 is a legal pair, the value is then f16(x)"""
    x, words = _map()
    h = words.view(np.float16).copy().reshape(2, 5, 5, 2, 2, 32)
    h[:, :, -2, :, 1] = 0                                             # the last interior pixel of every row
    t = torch.from_numpy(h.reshape(2, 5, 5, 128).view(np.float32))
    assert SR.well_formed(t)
    err = np.abs(SR.decode_map(t).numpy() - x)
    assert err[:, :, :-2].max() <= SR.REL_BOUND * np.abs(x).max()
    assert 2.0 ** -11 * np.abs(x).max() >= err[:, :, -2].max() > 2.0 ** -14 * np.abs(x).max()
