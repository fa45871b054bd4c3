"""The full-frame rasteriser's inputs at LARGE frames (oracle/fixtures.py: LARGE_FRAMES, large_frame_K, soup_frame, soup_slivers) on
the CPU, so that no edit can hollow out tests/test_gpu_raster_large_frames.py: what changes with the frame size is that the float32
set-up arithmetic of a triangle stops being exact (the sign-deciding sum, D, the depth planes, the matrix of the varyings: at
120 x 160 every product is below 2^24), that the span tables of the clip path are indexed by rows up to 2047, and that rectangles lie
far from the origin.  This file proves on the oracle alone that the two soups reach all of that, holds both evaluations of the rules
to each other under the 1/256-pixel snap on EVERY soup family, and -- where the GL library is present -- holds the rules to the live
library at 1080 x 1920 and 2048 x 96: coverage, depth bits, the owner read from the depth, and the interpolated colours."""
import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import ss_fast as SF
from oracle import ss_rules as S
from oracle import swiftshader_gl as SG

from test_raster_soups_oracle import BIG_PX, CASES, MIN_PATH_TRIANGLES, soup_args

f32 = np.float32
SMALL = Fx.SOUP_FRAME_HW
BIG_TWO = Fx.LARGE_FRAMES[:2]
# non-vacuity thresholds
MIN_FRAME_COVERED = 1000000       # frame soup at the two large sizes
MIN_BORDER = 200
MIN_SLIVER_PIXELS = 20000
MIN_MISJUDGED = 5                 # near-collinear triangles whose float area is zero or has the wrong sign

_cache = {}


def case(soup, hw):
    """everything the tests share about one (soup, frame): the projection, the rules' z-buffer and owners, the per-triangle arrays"""
    if (soup, hw) not in _cache:
        H, W = hw
        m = Fx.soup_frame() if soup == "frame" else Fx.soup_slivers(hw)
        K, P = Fx.large_frame_K(hw), Fx.soup_frame_pose()
        clip = S.clip_positions(m["vertices"], S.frame_pv(P, K, W, H))
        pv = S.project(clip, W, H)
        zbuf, owner, setups = S.rasterize(pv, m["faces"], W, H)
        _cache[(soup, hw)] = dict(m=m, K=K, P=P, clip=clip, pv=pv, zbuf=zbuf, owner=owner, setups=setups, T=SF._setup_arrays(pv, m["faces"], 4))
    return _cache[(soup, hw)]


def test_the_large_camera_is_the_small_one_scaled():
    assert Fx.LARGE_FRAMES == [(1080, 1920), (2048, 1024), (2048, 96)]
    assert np.array_equal(Fx.large_frame_K(SMALL), Fx.SOUP_FRAME_K)
    K = Fx.large_frame_K((1080, 1920))
    assert np.allclose(K[0], Fx.SOUP_FRAME_K[0] * 12) and np.allclose(K[1], Fx.SOUP_FRAME_K[1] * 9) and np.array_equal(K[2], [0, 0, 1])


@pytest.mark.parametrize("hw", Fx.LARGE_FRAMES)
def test_frame_soup_covers_the_large_frame_its_border_and_its_last_rows(hw):
    """Counted on the coverage of the rules (owner >= 0; the render's depth reads 0 beyond 2 m).  Rows are GL rows here; the render
    flips them, the border is the same set."""
    H, W = hw
    c = case("frame", hw)
    hit = c["owner"] >= 0
    border = int(hit[0].sum() + hit[-1].sum() + hit[:, 0].sum() + hit[:, -1].sum())
    clip_tris = np.nonzero(c["T"]["slow"])[0]
    clip_px = int(np.isin(c["owner"], clip_tris).sum())
    top = int(hit[H - 8:].sum()), int(hit[:8].sum())
    print("frame soup %d x %d: %d pixels covered, %d on the border, %d in the 8 highest GL rows, %d in the 8 lowest; clip path: %d triangles, %d pixels"
          % (H, W, hit.sum(), border, top[0], top[1], len(clip_tris), clip_px))
    assert len(clip_tris) > MIN_PATH_TRIANGLES and clip_px > 500
    if hw in BIG_TWO:
        assert hit.sum() > MIN_FRAME_COVERED and border > MIN_BORDER
    if H == 2048:                                  # rows 2040 .. 2047 of the span tables, and of the image (the read-back flips the rows)
        assert top[0] > 30 and top[1] > 30
        assert int(np.isin(c["owner"][H - 8:], clip_tris).sum()) > 30, "the clip path reaches rows 2040 and above"


@pytest.mark.parametrize("soup,hw", [(s, hw) for s in ("frame", "slivers") for hw in Fx.LARGE_FRAMES])
def test_coordinates_stay_where_both_sides_snap_them(soup, hw):
    """the rasteriser gives up on a window coordinate at |Xf| >= 1e9, oracle/ss_rules.project at 2^30: not reachable by these soups"""
    c = case(soup, hw)
    top = max(int(np.abs(c["pv"]["X"]).max()), int(np.abs(c["pv"]["Y"]).max()))
    print("%s %s: min |w| %.4f, max |X|,|Y| %d" % (soup, hw, np.abs(c["pv"]["w"]).min(), top))
    assert np.abs(c["pv"]["w"]).min() >= 1e-3 and top < 2 ** 24


def areas(c):
    n = len(c["m"]["faces"])
    X, Y = c["pv"]["X"][c["m"]["faces"]], c["pv"]["Y"][c["m"]["faces"]]
    assert X.shape == (n, 3)
    return Fx.float_area(X, Y), Fx.exact_area(X, Y)


def test_sliver_generator_is_seeded_and_shaped():
    for hw in [SMALL] + Fx.LARGE_FRAMES:
        a, b = Fx.soup_slivers(hw), Fx.soup_slivers(hw)
        n = len(a["faces"])
        assert n <= 500 and a["vertices"].shape == (3 * n, 3) and a["vertices"].dtype == np.float32
        assert np.array_equal(a["faces"], np.arange(3 * n).reshape(n, 3)) and a["faces"].dtype == np.int32
        assert a["colors"].shape == (3 * n, 3) and a["colors"].dtype == np.uint8 and a["normals"].shape == (3 * n, 3) and len(a["kd"]) == 3
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert not np.array_equal(Fx.soup_slivers(hw, 1)["vertices"], a["vertices"])
        col = a["colors"].reshape(n, 3, 3).astype(int)
        assert (np.abs(col[:, 0] - col[:, 1]).max(1) > 150).all() and (np.abs(col[:, 1] - col[:, 2]).max(1) > 150).all()


@pytest.mark.parametrize("hw", [SMALL] + Fx.LARGE_FRAMES)
def test_sliver_soup_makes_the_float_area_inexact(hw):
    """The sign of a triangle is a float32 sum of products of snapped coordinates (setup_triangle's order; Fx.float_area states it,
    and the first assertion ties that statement to the rules' own: a triangle is drawn where the float sum is not zero and has the sign
    of the integer area).  At 120 x 160 it is exact on every triangle; at the two large sizes it is inexact on more than half.  The triangles are long (a quarter of the diagonal and more) and thin (1 to 20 pixels)."""
    H, W = hw
    c = case("slivers", hw)
    m, owner = c["m"], c["owner"]
    n = len(m["faces"])
    fa, ea = areas(c)
    inexact = fa != ea
    assert np.array_equal(c["T"]["fast"], (fa != 0) & (ea != 0) & ((fa < 0) == (ea < 0)))
    assert not c["pv"]["flags"].any()                                              # unclipped: the small and the big path only
    assert np.array_equal(np.stack([c["pv"]["X"], c["pv"]["Y"]], -1).reshape(n, 3, 2)[m["lattice"]], m["target"][m["lattice"]])
    sl = np.setdiff1d(np.arange(n - 2), np.r_[m["lattice"], m["short"]])
    T = np.stack([c["pv"]["X"], c["pv"]["Y"]], -1).reshape(n, 3, 2)[sl] / 16.0
    edges = np.sqrt(((T[:, :, None, :] - T[:, None, :, :]) ** 2).sum(-1)).max((1, 2))
    width = np.abs(ea[sl]) / 256.0 / edges
    diag = np.hypot(H, W)
    own = int(((owner >= 0) & (owner < n - 2)).sum())
    seen = len(np.unique(owner[(owner >= 0) & (owner < n - 2)]))
    Xi, Yi = c["T"]["Xi"], c["T"]["Yi"]
    box = (((Xi.max(1) + 15) >> 4) - ((Xi.min(1) + 15) >> 4)) * (((Yi.max(1) + 15) >> 4) - ((Yi.min(1) + 15) >> 4))
    small_path = np.nonzero((box > 0) & (box <= BIG_PX) & c["T"]["fast"])[0]
    small_px, small_inexact = int(np.isin(owner, small_path).sum()), int(inexact[small_path].sum())
    print("slivers %d x %d: float area differs from the exact integer on %d of %d (%.1f %%); long edge %.0f .. %.0f px (diagonal %.0f), width "
          "%.1f .. %.1f px; windings %d / %d; %d pixels owned by %d slivers; thread-per-triangle path (boxes up to 256 px): %d triangles, %d of them inexact, own %d pixels"
          % (H, W, inexact.sum(), n, 100.0 * inexact.mean(), edges.min(), edges.max(), diag, width.min(), width.max(), (ea > 0).sum(), (ea < 0).sum(),
             own, seen, len(small_path), small_inexact, small_px))
    assert edges.min() > 0.24 * diag and edges.max() <= diag and 0.9 < width.min() and width.max() < 20.5
    assert min((ea > 0).sum(), (ea < 0).sum()) > 150
    if hw == SMALL:
        assert inexact.sum() == 0
    else:
        assert own > MIN_SLIVER_PIXELS and seen > 100
        assert len(small_path) >= MIN_PATH_TRIANGLES and small_px > 100 and len(np.setdiff1d(sl, small_path)) > 400       # both unclipped paths
    if hw in BIG_TWO:
        assert inexact.mean() > 0.5 and seen > 300 and small_inexact >= 5
    # depth names the owner: the property the live-library test reads the owner by
    dec = Fx.sliver_owner_from_depth(c["zbuf"], m)
    assert np.array_equal(dec, np.where(owner == n - 1, n - 2, owner))


@pytest.mark.parametrize("hw", Fx.LARGE_FRAMES)
def test_near_collinear_triangles_snap_as_targeted_and_are_misjudged(hw):
    """Twice the area is a few units where the float sum's products reach 2^30.  A misjudged triangle (float area zero, or of the wrong
    sign) draws nothing under the rules, and nothing in the live library (below): the walk direction comes from the float sign."""
    c = case("slivers", hw)
    m = c["m"]
    lat = m["lattice"]
    fa, ea = areas(c)
    assert len(lat) == Fx.SLIVER_LATTICE and (ea[lat] != 0).all() and np.array_equal(ea[lat], Fx.exact_area(m["target"][lat][..., 0], m["target"][lat][..., 1]))
    mis = (fa[lat] == 0) | ((fa[lat] < 0) != (ea[lat] < 0))
    drawn = int(np.isin(c["owner"], lat[mis]).sum())
    print("near-collinear %s: twice the area %s, float %s; %d misjudged, which own %d pixels" % (hw, ea[lat].tolist(), fa[lat].tolist(), mis.sum(), drawn))
    assert mis.sum() >= MIN_MISJUDGED and drawn == 0


@pytest.mark.parametrize("fam,i", CASES)
def test_both_evaluations_of_the_rules_agree_under_the_8_bit_snap(fam, i):
    """every family, not only the three the offset-rule tests run: `small` holds the slivers of the 176 x 176 window, where the
    1/256-pixel snap makes the float area inexact on most triangles"""
    m, P = Fx.soup(fam), Fx.soup_poses(fam)[i]
    win = Fx.gl_window(P, Fx.K_YCB, Fx.SOUP_WIDTH)
    vert, nrm, col, faces = soup_args(m)
    slow = S.render_vispy(vert, nrm, col, faces, P, Fx.K_YCB, win, return_float=True, numpy_rule="numpy1", sub_bits=8)
    fast = SF.render_vispy(vert, nrm, col, faces, P, Fx.K_YCB, win, numpy_rule="numpy1", sub_bits=8)
    Pm, V, _, _ = S.vispy_uniforms(P, Fx.K_YCB, win)
    pv = S.project(S.clip_positions(vert, S._mat_mul_cols(Pm, V)), 176, 176, 8)
    X, Y = pv["X"][faces], pv["Y"][faces]
    ok = (np.abs(X) < 2 ** 30).all(1) & (np.abs(Y) < 2 ** 30).all(1)
    inexact = Fx.float_area(X[ok], Y[ok]) != Fx.exact_area(X[ok], Y[ok])
    print("%s pose %d, 1/256 pixel: %d pixels covered; float area inexact on %d of %d triangles" % (fam, i, (slow[4] >= 0).sum(), inexact.sum(), ok.sum()))
    assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])
    assert (slow[4] >= 0).sum() > 3000
    if fam == "small":
        assert inexact.sum() > 100


# ---- the live library at large frames -------------------------------------------------------------------------------------------------
LIVE_FRAMES = [(1080, 1920), (2048, 96)]
_probes = {}


def probe(hw):
    from oracle.ss_probe import Probe
    if hw not in _probes:
        _probes[hw] = Probe(hw[1], hw[0])
    return _probes[hw]


@pytest.mark.skipif(not SG.available(), reason="needs the kaleido wheel's SwiftShader")
@pytest.mark.parametrize("hw", LIVE_FRAMES)
def test_the_live_library_draws_the_frame_soup_as_the_rules_do(hw):
    """one glDrawElements of the soup's clip-space positions into an H x W float depth target: coverage and depth bits of every pixel"""
    H, W = hw
    c = case("frame", hw)
    _, z = probe(hw).draw(c["clip"], None, faces=c["m"]["faces"])
    zb, ow = c["zbuf"], c["owner"]
    print("frame soup %d x %d: live library covers %d pixels, the rules %d; depth bits differ on %d"
          % (H, W, (z < 1).sum(), (ow >= 0).sum(), (zb.view(np.int32) != z.view(np.int32)).sum()))
    assert np.array_equal(ow >= 0, z < 1), "coverage"
    assert np.array_equal(zb.view(np.int32), z.view(np.int32)), "depth bits"


@pytest.mark.skipif(not SG.available(), reason="needs the kaleido wheel's SwiftShader")
@pytest.mark.parametrize("hw", LIVE_FRAMES)
def test_the_live_library_draws_the_sliver_soup_as_the_rules_do(hw):
    """Coverage, depth bits, and the owner read from the library's DEPTH (every triangle has a band of depth of its own; a varying that
    is constant on a sliver does not come back constant: its matrix M is ill-conditioned).  Then the colours: the library's float
    varyings against S.interpolate on every covered pixel."""
    H, W = hw
    c = case("slivers", hw)
    m, zb, ow = c["m"], c["zbuf"], c["owner"]
    n = len(m["faces"])
    col01 = (m["colors"].astype(np.float64) / 255.0).astype(f32)
    var = np.concatenate([col01, np.ones((3 * n, 1), f32)], 1)
    col, z = probe(hw).draw(c["clip"], var, faces=m["faces"])
    print("slivers %d x %d: live library covers %d pixels, the rules %d; depth bits differ on %d"
          % (H, W, (z < 1).sum(), (ow >= 0).sum(), (zb.view(np.int32) != z.view(np.int32)).sum()))
    assert np.array_equal(ow >= 0, z < 1), "coverage"
    assert np.array_equal(zb.view(np.int32), z.view(np.int32)), "depth bits"
    assert np.array_equal(Fx.sliver_owner_from_depth(z, m), np.where(ow == n - 1, n - 2, ow)), "owner, read from the library's depth"
    want = np.zeros((H, W, 3), f32)
    for t, s in c["setups"].items():
        ys, xs = np.nonzero(ow == t)
        if len(ys):
            want[ys, xs] = S.interpolate(s, col01[s.idx], xs, ys)
    hit = ow >= 0
    diff = (want.view(np.int32) != col[..., :3].view(np.int32)).any(2) & hit
    nan = int((np.isnan(want).any(2) & hit).sum())
    err = np.abs(want.astype(np.float64) - col[..., :3])[hit]
    b_want, b_got = S.unorm8(want), S.unorm8(col[..., :3])
    bytes_differ = int(((b_want != b_got).any(2) & hit).sum())
    print("slivers %d x %d: colours of the live library and S.interpolate differ in bits on %d of %d covered pixels, max |d| %.3g; "
          "non-finite in the rules on %d; as bytes they differ on %d" % (H, W, diff.sum(), hit.sum(), np.nanmax(err) if err.size else 0.0, nan, bytes_differ))
    assert diff.sum() == 0, "S.interpolate reproduces the library's varyings bit for bit"
