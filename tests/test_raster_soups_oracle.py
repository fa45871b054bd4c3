"""The triangle soups of oracle/fixtures.py (what a closed, convex, well-conditioned sphere never shows a rasteriser: depth ties,
pixel centres on edges and vertices, w <= 0, the far plane, polygons cut by many planes, mixed winding, degenerate triangles) on
the CPU: the two evaluations of the GL rules (oracle/ss_rules.py, one triangle at a time; oracle/ss_fast.py, arrays) agree byte
for byte on them, every family provably reaches the path it names (the counts are printed and held to thresholds), the snapped
coordinates stay where neither side gives up on them, and -- where the GL library is present -- the library itself draws each soup
in ONE call to the depth bits and owners of the rules.  tests/test_gpu_raster_soups.py holds the HIP kernels to the same renders."""
import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import ss_fast as SF
from oracle import ss_rules as S
from oracle import swiftshader_gl as SG

f32 = np.float32
SIZE = 176
BIG_PX = 256                 # csrc/raster.hip RASTER_BIG_PX: bounding boxes (clamped to the window) above it take the wave-per-triangle path
# non-vacuity thresholds
MIN_PATH_TRIANGLES = 10      # triangles on the path a family names ...
MIN_PATH_PIXELS = 500        # ... and pixels of the final image they own
MIN_PER_NEGATIVE_W = 5       # near: triangles with one / two / three vertices of w < 0
MIN_LATTICE_ON_EDGE = 200    # lattice: pixel centres exactly on an edge of a drawn triangle
MIN_TIED_PIXELS = 300        # ties: pixels where two or more triangles produce the winning z bit for bit
MIN_COVERED = 3000           # every case
MIN_MANY_PLANE_POLYGONS = 3  # far: clipped polygons with six or more vertices
MAX_POLYGON = 9              # a triangle cut by six planes; the rasteriser's polygon buffers hold 12
PATH_OF = dict(small="small", big="big", near="clip", far="clip")
CASES = [(fam, i) for fam in Fx.SOUP_FAMILIES for i in range(len(Fx.soup_poses(fam)))]


def soup_args(m):
    """what HipRenderer makes of the mesh dict: float32 normals normalised in float32, colours / 255"""
    nrm = m["normals"] / np.linalg.norm(m["normals"], axis=1).reshape(-1, 1)
    return m["vertices"], nrm.astype(f32), (m["colors"].astype(np.float64) / 255.0).astype(f32), m["faces"]


_cache = {}


def case(fam, i):
    """everything the tests below share about one (family, pose): both renders, the projection, the per-triangle arrays"""
    if (fam, i) not in _cache:
        m = Fx.soup(fam)
        P = Fx.soup_poses(fam)[i]
        win = Fx.gl_window(P, Fx.K_YCB, Fx.SOUP_WIDTH)
        vert, nrm, col, faces = soup_args(m)
        slow = S.render_vispy(vert, nrm, col, faces, P, Fx.K_YCB, win, return_float=True, numpy_rule="numpy1")
        fast = SF.render_vispy(vert, nrm, col, faces, P, Fx.K_YCB, win, numpy_rule="numpy1")
        Pm, V, _, _ = S.vispy_uniforms(P, Fx.K_YCB, win)
        clip = S.clip_positions(vert, S._mat_mul_cols(Pm, V))
        pv = S.project(clip, SIZE, SIZE)
        _cache[(fam, i)] = dict(m=m, P=P, win=win, slow=slow, fast=fast, clip=clip, pv=pv, T=SF._setup_arrays(pv, faces, 4), faces=faces)
    return _cache[(fam, i)]


def paths(c):
    """triangle indices per rasteriser path: small | big (unclipped, by the bounding box clamped to the window) | clip"""
    T = c["T"]
    x0 = np.maximum((T["Xi"].min(1) + 15) >> 4, 0); x1 = np.minimum((T["Xi"].max(1) + 15) >> 4, SIZE)
    y0 = np.maximum((T["Yi"].min(1) + 15) >> 4, 0); y1 = np.minimum((T["Yi"].max(1) + 15) >> 4, SIZE)
    box = np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)
    return dict(small=np.nonzero(T["fast"] & (box > 0) & (box <= BIG_PX))[0], big=np.nonzero(T["fast"] & (box > BIG_PX))[0],
                clip=np.nonzero(T["slow"])[0])


def test_generators_are_seeded_and_shaped():
    for fam in Fx.SOUP_FAMILIES:
        a, b = Fx.soup(fam), Fx.soup(fam)
        n = len(a["faces"])
        assert n <= 500 and a["vertices"].shape == (3 * n, 3) and a["vertices"].dtype == np.float32
        assert a["faces"].dtype == np.int32 and a["colors"].shape == (3 * n, 3) and a["colors"].dtype == np.uint8
        assert a["normals"].shape == (3 * n, 3) and a["normals"].dtype == np.float32
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert not np.array_equal(Fx.soup(fam, 1)["vertices"], a["vertices"])
    f = Fx.soup_frame()
    assert len(f["faces"]) <= 500 and (f["uv"] < 0).any() and (f["uv"] > 1).any()


@pytest.mark.parametrize("fam,i", CASES)
def test_both_evaluations_of_the_rules_agree(fam, i):
    c = case(fam, i)
    rgb, d16, _, zbuf, owner = c["slow"]
    assert np.array_equal(c["fast"][0], rgb) and np.array_equal(c["fast"][1], d16)
    covered = int((owner >= 0).sum())
    print("%s pose %d: %d triangles, %d pixels covered, %d owners" % (fam, i, len(c["faces"]), covered, len(np.unique(owner)) - 1))
    assert covered > MIN_COVERED


@pytest.mark.parametrize("fam,i", CASES)
def test_coordinates_stay_where_both_sides_snap_them(fam, i):
    """|w| >= 1e-3 and the snapped |X|, |Y| < 2^24 (1/16 pixel), < 2^28 under the 1/256-pixel rule: far below 1e9, where the
    rasteriser gives up on a coordinate, and 2^30, where oracle/ss_rules.project does -- nothing pins either cut-off to the live
    library, so the soups do not depend on it."""
    c = case(fam, i)
    assert np.abs(c["pv"]["w"]).min() >= 1e-3
    m4 = max(int(np.abs(c["pv"]["X"]).max()), int(np.abs(c["pv"]["Y"]).max()))
    pv8 = S.project(c["clip"], SIZE, SIZE, 8)
    m8 = max(int(np.abs(pv8["X"]).max()), int(np.abs(pv8["Y"]).max()))
    print("%s pose %d: min |w| %.4f, max |X|,|Y| %d (1/16 px), %d (1/256 px)" % (fam, i, np.abs(c["pv"]["w"]).min(), m4, m8))
    assert m4 < 2 ** 24 and m8 < 2 ** 28


@pytest.mark.parametrize("fam,i", [(f, i) for f, i in CASES if f in PATH_OF])
def test_each_family_reaches_the_path_it_names(fam, i):
    c = case(fam, i)
    owner = c["slow"][4]
    p = paths(c)
    own = {k: int(np.isin(owner, v).sum()) for k, v in p.items()}
    print("%s pose %d: triangles small %d big %d clip %d; pixels owned small %d big %d clip %d"
          % (fam, i, len(p["small"]), len(p["big"]), len(p["clip"]), own["small"], own["big"], own["clip"]))
    k = PATH_OF[fam]
    assert len(p[k]) >= MIN_PATH_TRIANGLES and own[k] >= MIN_PATH_PIXELS


def test_small_holds_its_degenerate_triangles():
    c = case("small", 0)
    T, faces, owner = c["T"], c["faces"], c["slow"][4]
    repeated = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    zero_area = (T["area2"] == 0) & ~repeated
    ex = np.abs(T["Xi"].max(1) - T["Xi"].min(1)); ey = np.abs(T["Yi"].max(1) - T["Yi"].min(1))
    drawn = np.isin(np.arange(len(faces)), owner)
    sub_pixel = (np.maximum(ex, ey) < 16) & (T["area2"] != 0) & ~drawn
    # a sliver: longest edge over 100 pixels, height (2 area / longest edge) under 1/16 pixel = one unit of the snapped grid
    longest = np.sqrt(np.maximum.reduce([(T["Xi"][:, a] - T["Xi"][:, b]) ** 2 + (T["Yi"][:, a] - T["Yi"][:, b]) ** 2
                                         for a, b in ((0, 1), (1, 2), (2, 0))]).astype(np.float64))
    sliver = (longest > 100 * 16) & (np.abs(T["area2"]) / np.maximum(longest, 1) < 1.0)
    wind = T["area2"][T["fast"]]
    print("small: repeated index %d, collinear after snapping %d, sub-pixel without a centre %d, slivers %d (drawn %d); windings %d / %d"
          % (repeated.sum(), zero_area.sum(), sub_pixel.sum(), sliver.sum(), (sliver & drawn).sum(), (wind > 0).sum(), (wind < 0).sum()))
    assert repeated.sum() >= 5 and sub_pixel.sum() >= 3 and sliver.sum() >= 3
    assert min((wind > 0).sum(), (wind < 0).sum()) >= 100


def test_near_has_every_count_of_vertices_behind_the_camera():
    c = case("near", 0)
    neg = (c["pv"]["w"][c["faces"]] < 0).sum(1)
    counts = [int((neg == k).sum()) for k in range(4)]
    print("near: triangles with 0 / 1 / 2 / 3 vertices of w < 0:", counts)
    assert min(counts[1:]) >= MIN_PER_NEGATIVE_W
    drawn = np.isin(np.arange(len(neg)), c["slow"][4])
    assert (drawn & (neg == 1)).sum() >= 3 and (drawn & (neg == 2)).sum() >= 3            # and they are seen


def test_far_reaches_the_far_plane_and_many_planes_at_once():
    c = case("far", 0)
    d16, owner = c["slow"][1], c["slow"][4]
    at_far = int(((d16 >= 1995) & (d16 <= 2000)).sum())
    fl = c["pv"]["flags"][c["faces"]]
    crossing = ((fl[:, 0] | fl[:, 1] | fl[:, 2]) & S.CLIP_FAR) != 0
    sizes = []
    for t in np.nonzero(c["T"]["slow"])[0]:
        i0, i1, i2 = c["faces"][t]
        poly = S.clip_polygon([c["pv"]["post"][k].copy() for k in (i0, i1, i2)], int(fl[t, 0] | fl[t, 1] | fl[t, 2]))
        sizes.append(len(poly))
    sizes = np.array(sizes)
    print("far: %d pixels within 5 mm of 2000, %d triangles cross the far plane, clipped polygon sizes %s, %d pixels drawn but beyond 2 m"
          % (at_far, crossing.sum(), np.bincount(sizes).tolist(), ((owner >= 0) & (d16 == 0)).sum()))
    assert at_far >= 20 and crossing.sum() >= MIN_PATH_TRIANGLES
    assert (sizes >= 6).sum() >= MIN_MANY_PLANE_POLYGONS and sizes.max() <= MAX_POLYGON


def on_edge_count(c):
    """pixel centres of the window exactly ON an edge (a vertex included) of a triangle that the image shows: integer edge functions"""
    X, Y = c["pv"]["X"], c["pv"]["Y"]
    owner = c["slow"][4]
    n = 0
    for t in np.unique(owner[owner >= 0]):
        xs, ys = X[c["faces"][t]], Y[c["faces"][t]]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            x0, x1 = sorted((int(xs[a]), int(xs[b]))); y0, y1 = sorted((int(ys[a]), int(ys[b])))
            px = np.arange(max((x0 + 15) // 16, 0), min(x1 // 16, SIZE - 1) + 1) * 16
            py = np.arange(max((y0 + 15) // 16, 0), min(y1 // 16, SIZE - 1) + 1) * 16
            if len(px) and len(py):
                E = (xs[b] - xs[a]) * (py[:, None] - ys[a]) - (ys[b] - ys[a]) * (px[None, :] - xs[a])
                n += int((E == 0).sum())
    return n


def test_lattice_puts_pixel_centres_on_edges():
    c = case("lattice", 0)
    X, Y = c["pv"]["X"], c["pv"]["Y"]
    on_half = int(((X % 8 == 0) & (Y % 8 == 0)).sum())
    n = on_edge_count(c)
    print("lattice: %d of %d vertices on the half-pixel grid, %d on pixel centres; %d pixel centres exactly on an edge; sphere-like small soup: %d"
          % (on_half, len(X), ((X % 16 == 0) & (Y % 16 == 0)).sum(), n, on_edge_count(case("small", 0))))
    assert on_half == len(X) and n >= MIN_LATTICE_ON_EDGE


@pytest.mark.parametrize("i", [0, 1])
def test_ties_has_pixels_where_draw_order_decides(i):
    """per pixel: how many triangles produce the winning z bit for bit (each triangle rasterised alone by the rules)"""
    c = case("ties", i)
    zbuf, owner = c["slow"][3], c["slow"][4]
    same = np.zeros(zbuf.shape, np.int32)
    later_loses = 0
    for t in range(len(c["faces"])):
        z, ow, _ = S.rasterize(c["pv"], c["faces"][t:t + 1], SIZE, SIZE)
        hit = (ow >= 0) & (z.view(np.int32) == zbuf.view(np.int32))
        same += hit
        later_loses += int((hit & (owner < t) & (owner >= 0)).sum())
    tied = int((same >= 2).sum())
    print("ties pose %d: %d pixels where >= 2 triangles give the winning z (up to %d); %d fragments lose to an earlier triangle on equal z"
          % (i, tied, same.max(), later_loses))
    assert (same[owner >= 0] >= 1).all() and tied >= MIN_TIED_PIXELS and later_loses >= MIN_TIED_PIXELS


def test_frame_soup_crosses_the_frame_edges_and_the_near_plane():
    m = Fx.soup_frame()
    H, W = Fx.SOUP_FRAME_HW
    rgb, d = S.render_frame(m["vertices"], (m["colors"] / 255.0).astype(f32), m["faces"], Fx.soup_frame_pose(), Fx.SOUP_FRAME_K, W, H, kd=m["kd"])
    border = int((d[0] > 0).sum() + (d[-1] > 0).sum() + (d[:, 0] > 0).sum() + (d[:, -1] > 0).sum())
    print("frame soup: %d pixels covered, %d on the border, depth %d .. %d mm" % ((d > 0).sum(), border, d[d > 0].min(), d.max()))
    assert (d > 0).sum() > 10000 and border > 200 and d[d > 0].min() <= 102


# ---- the live library on whole soups ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    from oracle.ss_probe import Probe
    return Probe(SIZE, SIZE)


@pytest.mark.skipif(not SG.available(), reason="needs the kaleido wheel's SwiftShader")
@pytest.mark.parametrize("fam,i", CASES)
def test_the_live_library_draws_the_soup_as_the_rules_do(probe, fam, i):
    """One glDrawElements of the whole soup's clip-space positions into a 176 x 176 float target; the varying is constant per
    triangle (its index + 1), so the colour read back names the owner.  Depth bits and owner of every pixel equal S.rasterize."""
    c = case(fam, i)
    faces = c["faces"]
    tid = np.zeros((len(c["clip"]), 4), f32)
    for k in range(3):
        tid[faces[:, k], :] = (np.arange(len(faces), dtype=f32) + 1)[:, None]
    if fam == "small":                       # the faces that repeat an index: their unused vertex stays 0, they draw nothing
        assert ((faces[:, 0] == faces[:, 1]).sum()) >= 5
    col, z = probe.draw(c["clip"], tid, faces=faces)
    zb, ow, _ = S.rasterize(c["pv"], faces, SIZE, SIZE)
    got_owner = np.rint(col[..., 0]).astype(np.int32) - 1
    print("%s pose %d: live library covers %d pixels, the rules %d; owners differ on %d, depth bits on %d"
          % (fam, i, (z < 1).sum(), (ow >= 0).sum(), (got_owner != ow).sum(), (zb.view(np.int32) != z.view(np.int32)).sum()))
    assert np.array_equal(ow >= 0, z < 1), "coverage"
    assert np.array_equal(zb.view(np.int32), z.view(np.int32)), "depth bits"
    assert np.array_equal(got_owner, ow), "owner"
    assert np.array_equal(zb, c["slow"][3]) and np.array_equal(ow, c["slow"][4])
