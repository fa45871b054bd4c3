"""CPU: the float64 statement of the full-frame renderer's texture filter (oracle/texture_oracle.py) and its per-pixel bound.

  * the float32 oracle ss_rules.render_frame lies inside the bound on every case of oracle/fixtures.py (cards x textures x Kd, the
    tilted card, the frame soup) with at most 10 % of the pixel-channels admitting two bytes: the bound and the cap are attainable;
  * the fixtures reach what they name (the lod clamps, pure levels, texel edges and the x0 = -1 wrap, several floor(lod) values);
  * quad corners across w = 0: no covered pixel of Fx.soup_frame() has one (its far plane keeps 1 / w >= 0.5, and the 1 / w plane
    would have to fall by that much within a pixel; changing the soup would move every byte the existing soup tests pin), so
    Fx.soup_horizon() brings them: planes that all but hold the camera centre.  Their extrapolated uv are finite there; fmaxf / fminf
    semantics on a NaN / inf rho are tested on stated inputs;
  * teeth: a float32 copy of the filter (filter_f32 below) passes, and fails `check` with any ONE planted fault:
        fault                                                caught on (card x texture, Kd index)
        level index + 1                                      lod1 x noise
        level index - 1                                      lod2 x noise
        level offsets by ceil instead of floor halving       top x noise40x24 (level 5 lies behind the 2 x 1 level, not a 3 x 2 one)
        x1 clamped instead of wrapped                        repeats x noise, edges_u x corners
        v not flipped                                        lod0 x noise
        negative index not wrapped                           edges_u x noise, edges_u x corners
        lod from the x differences only                      aniso_y x noise
        lod clamped at levels - 2                            beyond x noise5x3
        Kd channels rotated                                  lod0 x channels, Kd (0.9, 1.0, 0.8)
        unorm8 by round-to-nearest                           mag4 x noise
        pyramid rounding >> 2 without + 2                    lod1 x noise
  * the pyramid the library uploads (csrc/tex_pyramid.h, compiled into a stand-alone host program: no device, nothing loaded into
    Python) equals raster_oracle.mip_pyramid byte for byte, level offsets included, at every texture size of the fixtures."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import raster_oracle as R
from oracle import ss_rules as S
from oracle import texture_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
H, W = Fx.SOUP_FRAME_HW
K = Fx.SOUP_FRAME_K
PAIRS = sorted({(c, t) for c, t, _ in Fx.filter_cases()}, key=lambda p: (list(Fx.CARDS).index(p[0]), Fx.FILTER_TEXTURES.index(p[1])))


def expect_of(card, texname, kd_i):
    tex = Fx.filter_texture(texname)
    m = Fx.card(card, tex.shape[:2])
    return m, tex, T.Expect(m["vertices"], m["faces"], m["uv"], tex, Fx.FILTER_KDS[kd_i], Fx.card_pose(), K, W, H)


def oracle_f32(m, tex, kd, P):
    kw = {} if kd is None else dict(kd=kd)
    return S.render_frame(m["vertices"], None, m["faces"], P, K, W, H, uv=m["uv"], texture=tex, **kw)


# ---- the float32 oracle inside the bound ----------------------------------------------------------------------------------------------
def test_the_case_list():
    cases = Fx.filter_cases()
    assert {c for c, _, _ in cases} == set(Fx.CARDS) and {t for _, t, _ in cases} == set(Fx.FILTER_TEXTURES)
    assert {k for _, _, k in cases} == {0, 1, 2} and len(cases) == 3 * len(PAIRS)
    sizes = [Fx.filter_texture(t).shape[:2] for t in Fx.FILTER_TEXTURES]
    assert sizes == [(64, 128), (40, 24), (5, 3), (1, 7), (7, 1), (1, 1), (16, 16), (32, 32)]
    for c in Fx.CARDS:                                           # the full-contrast noise texture is on every card
        assert (c, "noise") in PAIRS, c


@pytest.mark.parametrize("card,texname", PAIRS)
def test_float32_oracle_within_the_bound_on_cards(card, texname):
    for kd_i, kd in enumerate(Fx.FILTER_KDS):
        m, tex, e = expect_of(card, texname, kd_i)
        rgb, depth = oracle_f32(m, tex, kd, Fx.card_pose())
        assert 2000 < e.covered.sum() < 4000 and np.array_equal(depth > 0, e.covered)
        assert (rgb[~e.covered] == 0).all()
        T.check(rgb, e, "%s x %s, Kd %s" % (card, texname, kd))
        # w is constant on the card: the level of detail is the closed form of the map, at every pixel
        _, lod = Fx.card_jacobian(card, tex.shape[:2])
        assert np.abs(e.aux["lod"] - lod).max() < 0.01, (card, texname, lod, e.aux["lod"].min(), e.aux["lod"].max())


def test_float32_oracle_within_the_bound_on_the_tilted_card_and_the_soup():
    tex = Fx.filter_texture("noise")
    m, P = Fx.card_tilted()
    e = T.Expect(m["vertices"], m["faces"], m["uv"], tex, None, P, K, W, H)
    rgb, depth = oracle_f32(m, tex, None, P)
    T.check(rgb, e, "tilted card x noise")
    floors = np.unique(e.aux["l0"])
    print("tilted card: depth %d..%d mm, lod %.3f..%.3f" % (depth[depth > 0].min(), depth.max(), e.aux["lod"].min(), e.aux["lod"].max()))
    assert len(floors) >= 3 and depth[depth > 0].min() < 250 and depth.max() > 450
    m, P = Fx.soup_frame(), Fx.soup_frame_pose()
    e = T.Expect(m["vertices"], m["faces"], m["uv"], tex, m["kd"], P, K, W, H)
    rgb, depth = oracle_f32(m, tex, m["kd"], P)
    assert np.array_equal(depth > 0, e.covered) and e.covered.sum() > 10000
    T.check(rgb, e, "frame soup x noise")
    # no covered pixel of this soup has a quad corner across w = 0 (see the module's docstring) ...
    assert (e.g["wq"] > 0).all() and np.isfinite(e.g["q"]).all()
    # ... the horizon soup has, and runs through every level on the way
    m, P = Fx.soup_horizon()
    e = T.Expect(m["vertices"], m["faces"], m["uv"], tex, None, P, K, W, H)
    rgb, depth = oracle_f32(m, tex, None, P)
    across = (e.g["wq"] <= 0).any(1)
    print("horizon soup: %d covered pixels with a quad corner across w = 0, floor(lod) %s" % (across.sum(), np.bincount(e.aux["l0"])))
    assert across.sum() >= 10 and len(np.unique(e.aux["l0"])) == len(R.mip_pyramid(tex)) and np.array_equal(depth > 0, e.covered)
    T.check(rgb, e, "horizon soup x noise")


def test_cards_reach_what_they_name():
    tex = Fx.filter_texture("noise")
    th, tw = tex.shape[:2]
    L = len(R.mip_pyramid(tex))
    assert L == 8
    got = {}
    for card in Fx.CARDS:
        _, _, e = expect_of(card, "noise", 2)
        got[card] = e
    assert got["mag4"].aux["rho"].max() < 0.26 and (got["mag4"].aux["lod"] == 0).all()             # the lower clamp
    assert np.abs(got["lod0"].aux["rho"] - 1).max() < 1e-2 and (got["lod0"].aux["l0"] == 0).all()
    assert (np.abs(got["lod1"].aux["lod"] - 1) < 0.01).all() and (np.abs(got["lod2"].aux["lod"] - 2) < 0.01).all()
    assert (got["top"].aux["l0"] >= L - 2).all() and np.abs(got["top"].aux["lod"] - (L - 1)).max() < 0.01
    assert (got["beyond"].aux["lod"] == L - 1).all() and got["beyond"].aux["rho"].min() > 7.9 * 2 ** (L - 1)   # the upper clamp
    for card in ("aniso_x", "aniso_y"):
        assert np.abs(got[card].aux["lod"] - 2).max() < 0.01
    # edges: pixel centres on texel edges (x = k - 0.5: ax = 0.5) and on texel centres (ax = 0 or 1 up to rounding), and the wrap at 0
    for card, axis in (("edges_u", 0), ("edges_v", 1)):
        uv = got[card].g["uv"].astype(np.float64)
        x = uv[:, 0] * tw - 0.5 if axis == 0 else (1 - uv[:, 1]) * th - 0.5
        a = x - np.floor(x)
        assert (np.abs(a - 0.5) < 1e-4).mean() > 0.4 and (np.minimum(a, 1 - a) < 1e-4).mean() > 0.4, card
        assert (np.floor(x) == (-1 if axis == 0 else th - 1)).sum() > 30, card           # x0 = -1 wraps; y1 = th wraps
        assert (uv[:, axis] < 0).any() and (uv[:, axis] > 0).any()
    uv = got["repeats"].g["uv"]
    assert uv.min() < -3.2 and uv.max() > 2.45 and len(np.unique(np.floor(uv[:, 0]))) >= 6


# ---- a float32 copy of the filter, with planted faults --------------------------------------------------------------------------------
def filter_f32(tex, kd, g, fault=None):
    """the filter in float32, operation by operation as csrc/raster.hip states it; image [H,W,3].  `fault` plants one error."""
    levels = R.mip_pyramid(tex)
    if fault == "pyramid truncates":
        levels = [np.asarray(tex, np.uint8)]
        while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
            t = levels[-1].astype(np.int32)
            h, w = t.shape[:2]
            ys, xs = 2 * np.arange(max(h // 2, 1)), 2 * np.arange(max(w // 2, 1))
            y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
            levels.append(((t[ys][:, xs] + t[ys][:, x1] + t[y1][:, xs] + t[y1][:, x1]) >> 2).astype(np.uint8))
    nlev = len(levels)
    th, tw = levels[0].shape[:2]
    # the levels back to back, as the device holds them
    half = (lambda n: max((n + 1) // 2, 1)) if fault == "ceil offsets" else (lambda n: max(n // 2, 1))
    offs, w_, h_ = [0], tw, th
    for _ in range(nlev - 1):
        offs.append(offs[-1] + w_ * h_ * 3)
        w_, h_ = half(w_), half(h_)
    flat = np.concatenate([l.reshape(-1) for l in levels] + [np.zeros(4096, np.uint8)])
    kd = np.asarray((1.0, 1.0, 1.0) if kd is None else kd, f32)
    if fault == "kd rotated":
        kd = np.roll(kd, 1)
    uv, q = np.asarray(g["uv"], f32), np.asarray(g["q"], f32)
    size = np.array([tw, th], f32)
    with np.errstate(all="ignore"):
        dx, dy = (q[:, 1] - q[:, 0]) * size, (q[:, 2] - q[:, 0]) * size
        rx, ry = np.sqrt(dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]), np.sqrt(dy[:, 0] * dy[:, 0] + dy[:, 1] * dy[:, 1])
        rho = rx if fault == "lod from x only" else np.fmax(rx, ry)
        top = nlev - 2 if fault == "top clamp" else nlev - 1
        lod = np.fmin(np.fmax(np.log2(np.fmax(rho, f32(1e-8)).astype(np.float64)).astype(f32), f32(0)), f32(top))
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, nlev - 1)
    fl = (lod - l0.astype(f32))[:, None]
    shift = {"level + 1": 1, "level - 1": -1}.get(fault, 0)
    s0, s1 = np.clip(l0 + shift, 0, nlev - 1), np.clip(l1 + shift, 0, nlev - 1)

    def sample(lv):
        w, h = np.maximum(tw >> lv, 1), np.maximum(th >> lv, 1)
        x = uv[:, 0] * w.astype(f32) - f32(0.5)
        y = (uv[:, 1] if fault == "v not flipped" else f32(1) - uv[:, 1]) * h.astype(f32) - f32(0.5)
        xf, yf = np.floor(x), np.floor(y)
        ax, ay = (x - xf)[:, None], (y - yf)[:, None]
        if fault == "negative not wrapped":
            x0, y0 = np.maximum(np.fmod(xf, w), 0).astype(np.int64), np.maximum(np.fmod(yf, h), 0).astype(np.int64)
        else:
            x0, y0 = np.mod(xf.astype(np.int64), w), np.mod(yf.astype(np.int64), h)
        x1, y1 = (x0 + 1) % w, (y0 + 1) % h
        if fault == "x1 clamped":
            x1 = np.minimum(x0 + 1, w - 1)
        base = np.asarray(offs)[lv]
        tx = lambda yy, xx: flat[(base + (yy * w + xx) * 3)[:, None] + np.arange(3)].astype(f32)
        t00, t10, t01, t11 = tx(y0, x0), tx(y0, x1), tx(y1, x0), tx(y1, x1)
        return (t00 * (f32(1) - ax) + t10 * ax) * (f32(1) - ay) + (t01 * (f32(1) - ax) + t11 * ax) * ay
    c0, c1 = sample(s0), sample(s1)
    col = ((c0 + fl * (c1 - c0)) * f32(1.0 / 255.0)) * kd[None, :]
    assert col.dtype == f32
    if fault == "unorm8 rounds":
        byte = np.rint(np.clip(col, 0, 1) * f32(255)).astype(np.uint8)
    else:
        byte = S.unorm8(col)
    img = np.zeros((H, W, 3), np.uint8)
    img[g["rows"], g["cols"]] = byte
    return img


TEETH = [("level + 1", "lod1", "noise", 2), ("level - 1", "lod2", "noise", 2), ("ceil offsets", "top", "noise40x24", 2),
         ("x1 clamped", "repeats", "noise", 2), ("x1 clamped", "edges_u", "corners", 2), ("v not flipped", "lod0", "noise", 2),
         ("negative not wrapped", "edges_u", "noise", 2), ("negative not wrapped", "edges_u", "corners", 2),
         ("lod from x only", "aniso_y", "noise", 2), ("top clamp", "beyond", "noise5x3", 2), ("kd rotated", "lod0", "channels", 0),
         ("unorm8 rounds", "mag4", "noise", 2), ("pyramid truncates", "lod1", "noise", 2)]


@pytest.mark.parametrize("fault,card,texname,kd_i", TEETH)
def test_planted_fault_is_caught(fault, card, texname, kd_i):
    m, tex, e = expect_of(card, texname, kd_i)
    T.check(filter_f32(tex, Fx.FILTER_KDS[kd_i], e.g), e, "%s x %s without a fault" % (card, texname))
    with pytest.raises(AssertionError, match="outside their admissible set") as err:
        T.check(filter_f32(tex, Fx.FILTER_KDS[kd_i], e.g, fault), e, "%s x %s with '%s'" % (card, texname, fault))
    print(str(err.value)[:300])


def test_the_float32_copy_is_the_oracle_on_a_card():
    """filter_f32 without a fault is ss_rules.render_frame's filter (up to the float64 log2 there): the teeth bite a real evaluation"""
    m, tex, e = expect_of("lod2.37", "noise", 0)
    rgb, _ = oracle_f32(m, tex, Fx.FILTER_KDS[0], Fx.card_pose())
    mine = filter_f32(tex, Fx.FILTER_KDS[0], e.g)
    assert (np.abs(mine.astype(int) - rgb.astype(int)).max() <= 1) and (mine != rgb).mean() < 0.01


# ---- fmaxf / fminf on NaN and inf -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_rho_follow_fmaxf():
    tex = Fx.filter_texture("noise")
    levels = R.mip_pyramid(tex)
    nan, inf = f32(np.nan), f32(np.inf)
    base = np.array([[0.3, 0.6], [0.31, 0.6], [0.3, 0.61]], f32)
    q = np.stack([base] * 7)
    q[1, 1, 0] = nan                   # the x corner is NaN: rho = the y difference alone (fmaxf drops the NaN)
    q[2, 1] = nan; q[2, 2] = nan       # both NaN: rho NaN -> fmaxf(NaN, 1e-8) = 1e-8 -> lod 0
    q[3, 2, 1] = inf                   # inf: the top level
    q[4, 0] = inf; q[4, 1, 0] = inf    # inf - inf = NaN in x, inf in y: the top level
    q[5, 0] = nan                      # the shared corner NaN: both differences NaN -> lod 0
    q[6, 1, 0] = f32(-3e38); q[6, 0, 0] = f32(3e38)     # overflows float32 in the kernel, not here: the top level either way
    uv = np.tile(base[0], (7, 1))
    lod, rho = T.level_of_detail(q, 128, 64, len(levels))
    # the plain quad: x 0.01 * 128 = 1.28, y 0.01 * 64 = 0.64;  y alone: 0.64 < 1, clamped to 0
    want = [float(np.log2(1.28)), 0.0, 0.0, 7.0, 7.0, 0.0, 7.0]
    assert np.allclose(lod, want, atol=1e-4), lod
    c, delta, aux = T.evaluate(levels, None, uv, q)
    assert np.isfinite(c).all() and np.isfinite(delta).all()
    g = dict(uv=uv, q=q, rows=np.arange(7), cols=np.arange(7))
    got = filter_f32(tex, None, g)[np.arange(7), np.arange(7)].astype(int)
    lo, hi, _ = T.admissible(c, delta)
    assert ((got >= lo) & (got <= hi)).all(), (got, lo, hi)
    top = int(levels[-1][0, 0, 0])
    assert got[3, 0] == got[4, 0] == got[6, 0] and abs(got[3, 0] - top) <= 1
    with pytest.raises(ValueError):    # the Python max / min chain of the float32 oracle cannot state this rule
        int(np.floor(min(max(np.log2(max(float("nan"), 1e-8)), 0.0), 7)))


# ---- the pyramid the device holds -------------------------------------------------------------------------------------------------------
def test_host_pyramid_equals_the_python_pyramid(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "pyramid_host")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pyramid_host.cpp"), "-o", exe])
    texs = [Fx.filter_texture(t) for t in Fx.FILTER_TEXTURES] + [Fx.textured_sphere(0)["texture"]]
    rng = np.random.default_rng(5)
    texs += [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((3, 5), (2, 1), (1, 2), (33, 17))]
    for i, tex in enumerate(texs):
        th, tw = tex.shape[:2]
        src, dst = str(tmp_path / ("t%d.rgb" % i)), str(tmp_path / ("p%d.bin" % i))
        tex.tofile(src)
        out = subprocess.run([exe, src, str(th), str(tw), dst], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.returncode, out.stderr)
        raw = open(dst, "rb").read()
        levels = struct.unpack("<i", raw[:4])[0]
        offs = struct.unpack("<16I", raw[4:68])
        pyr = np.frombuffer(raw[68:], np.uint8)
        want = R.mip_pyramid(tex)
        assert levels == len(want), (th, tw, levels, len(want))
        off = 0
        for l, lv in enumerate(want):
            assert lv.shape[:2] == (max(th >> l, 1), max(tw >> l, 1)), (th, tw, l)    # the sizes sample_bilinear assumes
            assert offs[l] == off, (th, tw, l, offs[l], off)
            assert np.array_equal(pyr[off:off + lv.size], lv.reshape(-1)), (th, tw, l)
            off += lv.size
        assert off == len(pyr) and all(o == 0 for o in offs[levels:])
