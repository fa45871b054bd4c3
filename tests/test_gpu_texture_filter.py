"""GPU: the texture filter of the full-frame renderer (raster_resolve_kernel's `a.mode == 1 && a.tex` branch, csrc/raster.hip, on the
pyramid se3tn_mesh_set_texture builds) held PER PIXEL to the float64 statement of oracle/texture_oracle.py: every covered
pixel-channel inside the byte range of c +- delta (delta derived there from the float32 formats, nothing fitted), at most two bytes in
a range, at most 10 % of the pixel-channels with two; depth equal to the rules' (oracle/ss_rules.py), background exactly 0.

Cases (oracle/fixtures.py; tests/test_texture_filter_oracle.py proves on the CPU that the float32 oracle passes them, that eleven
planted faults do not, and that the host pyramid is the Python one): fronto-parallel cards with a closed-form level of detail (both lod
clamps, pure levels, anisotropic and sheared maps, pixel centres on texel edges, uv negative / above 1 / over several repeats) on eight
textures (64 x 128 noise down to 1 x 1, one-texel-wide levels, odd halving) under three Kd (the reference's, zero and saturation,
the default); a tilted card whose lod crosses several levels; the frame soup across the near plane; a soup whose quad corners cross w = 0; scissor rectangles of the tilted
card; three objects with their own materials in one se3tn_on_track_objects call; the textured sphere of the older tests.

Measured on the MI355X (what `check` prints: covered pixels, the share of pixel-channels with two admissible bytes -- cap 0.10 --
and the share that is not the nearest byte of c; per card the largest over its 24 texture x Kd cases).  No pixel-channel of any
case lay outside its admissible set; no kernel or host fix was needed.
    mag4                                24 cases   2604 pixels   two-byte <= 0.0049   not-nearest <= 0.0003
    lod0                                24 cases   2604 pixels   two-byte <= 0.0143   not-nearest <= 0.0000
    lod0.5                              24 cases   2604 pixels   two-byte <= 0.0054   not-nearest <= 0.0001
    lod1                                24 cases   2604 pixels   two-byte <= 0.0017   not-nearest <= 0.0000
    lod2                                24 cases   2604 pixels   two-byte <= 0.0029   not-nearest <= 0.0001
    lod2.37                             24 cases   2604 pixels   two-byte <= 0.0005   not-nearest <= 0.0000
    top                                 24 cases   2604 pixels   two-byte <= 0.0000   not-nearest <= 0.0000
    beyond                              24 cases   2604 pixels   two-byte <= 0.0000   not-nearest <= 0.0000
    aniso_x                             24 cases   2604 pixels   two-byte <= 0.0014   not-nearest <= 0.0000
    aniso_y                             24 cases   2604 pixels   two-byte <= 0.0010   not-nearest <= 0.0001
    sheared                             24 cases   2604 pixels   two-byte <= 0.0022   not-nearest <= 0.0000
    edges_u                             24 cases   2604 pixels   two-byte <= 0.0046   not-nearest <= 0.0001
    edges_v                             24 cases   2604 pixels   two-byte <= 0.0238   not-nearest <= 0.0000
    repeats                             24 cases   2604 pixels   two-byte <= 0.0079   not-nearest <= 0.0001
    tilted card x noise                  2 cases   6326 pixels   two-byte <= 0.0011   not-nearest <= 0.0000
    frame soup x noise                   1 case   15168 pixels   two-byte <= 0.0042   not-nearest <= 0.0000
    horizon soup x noise                 1 case    1059 pixels   two-byte <= 0.0003   not-nearest <= 0.0000
    textured sphere                      2 cases   2744 pixels   two-byte <= 0.0013   not-nearest <= 0.0000
    full frame, textured                 1 case   15168 pixels   two-byte <= 0.0011   not-nearest <= 0.0000
    three objects in one call, two orders: 17222 / 18315 / 7081 pixels of image A, 0 pixel-channels outside their sets"""
import numpy as np
import pytest

from oracle import fixtures as Fx
from oracle import se3_oracle as O
from oracle import ss_rules as S
from oracle import texture_oracle as T

pytestmark = pytest.mark.gpu
f32 = np.float32
H, W = Fx.SOUP_FRAME_HW
K = Fx.SOUP_FRAME_K
CASES = Fx.filter_cases()


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def eng(se3):
    return se3.Engine(0, 1)


def model_of(m, tex=None, kd=None):
    d = dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], normals=m["normals"])
    if tex is not None:
        d.update(uv=m["uv"], texture=tex)
    if kd is not None:
        d["kd"] = kd
    return d


_depth = {}


def rules_depth(key, m, P):
    """coverage and depth by the rules (they do not depend on the material: the vertex-colour render of the same geometry), once per
    module and left unchanged"""
    if key not in _depth:
        _, d = S.render_frame(m["vertices"], (np.asarray(m["colors"], np.float64) / 255.0).astype(f32), m["faces"], P, K, W, H)
        d.setflags(write=False)
        _depth[key] = d
    return _depth[key]


def render_and_check(se3, eng, m, tex, kd, P, key, name):
    e = T.Expect(m["vertices"], m["faces"], m["uv"], tex, kd, P, K, W, H)
    ren = se3.HipRenderer(eng, model_of(m, tex, kd), mode="pyrender", frame_size=(H, W))
    rgb, depth = ren.render_frame(P, K)
    want_d = rules_depth(key, m, P)
    assert np.array_equal(want_d > 0, e.covered)
    assert np.array_equal(depth, want_d), name                       # coverage and depth: every pixel
    assert (rgb[~e.covered] == 0).all(), name                        # the background is exactly 0
    T.check(rgb, e, name)
    return ren, rgb, depth, e


@pytest.mark.parametrize("card,texname,kd_i", CASES)
def test_cards(se3, eng, card, texname, kd_i):
    tex = Fx.filter_texture(texname)
    m = Fx.card(card, tex.shape[:2])
    kd = Fx.FILTER_KDS[kd_i]
    _, rgb, _, e = render_and_check(se3, eng, m, tex, kd, Fx.card_pose(), "card", "%s x %s, Kd %s" % (card, texname, kd))
    assert 2000 < e.covered.sum() < 4000
    if kd_i == 1:                                                    # Kd (0, 1, 2.5): red is 0, blue saturates where the texture is bright
        assert (rgb[..., 0] == 0).all()
        bright = e.c[:, 2] >= 1.0
        assert (rgb[e.g["rows"], e.g["cols"], 2][bright] == 255).all()


def test_tilted_card_and_frame_soup(se3, eng):
    tex = Fx.filter_texture("noise")
    m, P = Fx.card_tilted()
    _, _, _, e = render_and_check(se3, eng, m, tex, None, P, "tilted", "tilted card x noise")
    assert len(np.unique(e.aux["l0"])) >= 3
    m, P = Fx.soup_frame(), Fx.soup_frame_pose()
    _, _, _, e = render_and_check(se3, eng, m, tex, m["kd"], P, "soup", "frame soup x noise")
    assert e.covered.sum() > 10000
    m, P = Fx.soup_horizon()                                         # quad corners across w = 0, every level of the pyramid
    _, _, _, e = render_and_check(se3, eng, m, tex, None, P, "horizon", "horizon soup x noise")
    assert (e.g["wq"] <= 0).any(1).sum() >= 10


RECTS = [("odd origin", (41, 23, 118, 97)), ("one pixel wide", (59, 0, 60, 120))]       # (column 59 crosses lod = 2)


def test_scissor_rectangles_of_the_tilted_card(se3, eng):
    """render_frame_rect equals the slice of render_frame byte for byte where the lod changes across the rectangle and the texture is
    noise (the 2 x 2 quad of the lod is taken at absolute window coordinates, whatever the rectangle's origin)"""
    tex = Fx.filter_texture("noise")
    m, P = Fx.card_tilted()
    ren, rgb, depth, e = render_and_check(se3, eng, m, tex, None, P, "tilted", "tilted card x noise")
    l0 = np.full((H, W), -1)
    l0[e.g["rows"], e.g["cols"]] = e.aux["l0"]
    for name, (x0, y0, x1, y1) in RECTS:
        r_rgb, r_depth = ren.render_frame_rect(P, K, (x0, y0, x1, y1))
        inside = l0[y0:y1, x0:x1]
        print("rect %s %s: %d covered pixels, floor(lod) %s" % (name, (x0, y0, x1, y1), (inside >= 0).sum(), np.unique(inside[inside >= 0])))
        assert (inside >= 0).sum() > 30 and len(np.unique(inside[inside >= 0])) >= 2, name
        assert r_rgb.shape == (y1 - y0, x1 - x0, 3)
        assert np.array_equal(r_depth, depth[y0:y1, x0:x1]) and np.array_equal(r_rgb, rgb[y0:y1, x0:x1]), name


# ---- per-instance materials: three objects in one se3tn_on_track_objects call ---------------------------------------------------------
def _objects():
    noise, small = Fx.filter_texture("noise"), Fx.filter_texture("noise5x3")
    ball = Fx.icosphere(2, 0.03, 1)
    return [
        dict(name="card x noise", mesh=Fx.card("lod2.37", noise.shape[:2]), tex=noise, kd=None, P=Fx.card_pose(), width=100.0),
        dict(name="card x noise5x3", mesh=Fx.card("sheared", small.shape[:2]), tex=small, kd=(0.6, 1.3, 0.85), P=Fx.card_pose(), width=90.0),
        dict(name="vertex colours", mesh=ball, tex=None, kd=(0.7, 0.9, 0.6), P=Fx.pose(5, (-0.02, 0.01, 0.4)), width=110.0),
    ]


def _object_oracle(ob):
    """full-frame lo / hi / depth images of one object: the admissible bytes of the source pixel every crop pixel selects"""
    m = ob["mesh"]
    if ob["tex"] is None:
        rgb, d = S.render_frame(m["vertices"], (np.asarray(m["colors"], np.float64) / 255.0).astype(f32), m["faces"], ob["P"], K, W, H, kd=ob["kd"])
        return rgb, rgb, d                                           # vertex colours are exact: one admissible byte
    e = T.Expect(m["vertices"], m["faces"], m["uv"], ob["tex"], ob["kd"], ob["P"], K, W, H)
    d = rules_depth(("object", ob["name"]), m, ob["P"])
    assert np.array_equal(d > 0, e.covered)
    two = float((e.hi[e.covered] != e.lo[e.covered]).mean())
    assert (e.hi.astype(int) - e.lo.astype(int)).max() <= 1 and two <= T.TWO_BYTE_CAP
    return e.lo, e.hi, d


def test_per_instance_materials_in_one_call(se3):
    """Every image A of the batched launch (each instance with its own texture pyramid, level offsets, size and Kd, or vertex colours
    under its Kd) is crop_bbox of that object's oracle frame: depth exact, colour in the admissible set of the source pixel -- in two
    orders of the objects.  (Small head gains; the network's output is not the subject.)"""
    objs = _objects()
    cam = dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2])
    mean, std = Fx.mean_std(0)
    sd = O.make_state_dict(0, head_gain=0.002)
    trks = []
    for ob in objs:
        trk = se3.Tracker(dict(Fx.DATASET_INFO, camera=cam, object_width=ob["width"], renderer="pyrenderer"), mean, std, {"state_dict": sd},
                          max_samples=1)
        m = ob["mesh"]
        model = dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], normals=m["normals"], kd=ob["kd"]) if ob["tex"] is None \
            else model_of(m, ob["tex"], ob["kd"])
        trk.renderer = se3.HipRenderer(trk.engine, model, mode="pyrender", frame_size=(H, W))
        trks.append(trk)
    want = [_object_oracle(ob) for ob in objs]
    frame_rgb, frame_depth = Fx.structured_frame(400, H, W)
    for order in ([0, 1, 2], [2, 0, 1]):
        mt = se3.MultiTracker([trks[i] for i in order])
        mt.on_track(np.stack([objs[i]["P"] for i in order]), frame_rgb, frame_depth)
        lp = mt.last_prediction
        for j, i in enumerate(order):
            rgbA, depthA = lp["rgbA"][j].cpu().numpy(), lp["depthA"][j].cpu().numpy().view(np.uint16)
            bb = O.compute_bbox(objs[i]["P"], K, objs[i]["width"], (1000, 1000, 1000))
            lo, hi, d = want[i]
            lo_c, d_c = O.crop_bbox(lo, d, bb, (176, 176))
            hi_c, _ = O.crop_bbox(hi, d, bb, (176, 176))
            n = int((d_c > 0).sum())
            bad = int(((rgbA < lo_c) | (rgbA > hi_c)).sum())
            print("order %s, object %d (%s): image A covers %d pixels, %d pixel-channels outside their admissible set"
                  % (order, i, objs[i]["name"], n, bad))
            assert n > 3000, (order, i)
            assert np.array_equal(depthA, d_c), (order, i)
            assert bad == 0, (order, i, bad)
        mt.close()
    # the three images differ: each instance really read its own material
    assert len(np.unique(lp["rgbA"][1].cpu().numpy().reshape(-1, 3), axis=0)) > 300


# ---- the sphere of the older tests ----------------------------------------------------------------------------------------------------
def test_textured_sphere_of_the_older_tests(se3, eng):
    """Fx.textured_sphere at the pose of tests/test_renderer.py, built from the dict: the statistical bound of that test (against the
    float32 oracle) and the per-pixel one"""
    ms = Fx.textured_sphere(2)
    m = dict(ms, normals=ms["vertices"] / np.linalg.norm(ms["vertices"], axis=1, keepdims=True))
    P = Fx.pose(4, (0.01, -0.02, 0.45))
    _, rgb, depth, e = render_and_check(se3, eng, m, ms["texture"], ms["kd"], P, "sphere", "textured sphere")
    orgb, odepth = S.render_frame(np.asarray(ms["vertices"], f32), None, ms["faces"], P, K, W, H, uv=ms["uv"], texture=ms["texture"], kd=ms["kd"])
    assert (depth > 0).sum() > 1500 and np.array_equal(depth, odepth)
    d = np.abs(rgb.astype(int) - orgb.astype(int)).max(2)
    assert np.median(d[depth > 0]) <= 1 and (d > 6).mean() < 0.02
    T.check(orgb, e, "textured sphere, float32 oracle")
