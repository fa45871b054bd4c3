"""What the scene-aware colour tests share (a helper module: numpy and the oracle, no device).

1. cases(): (model, observed, scene) descriptor triples on the 230 x 260 frames of tests/color_fit_oracle.py -- the scene under the
   observed window, under another image size and window, under a window that misses its image -- and a 176 x 176 `boundaries` case in
   which every boundary value of the scene depth meets every branch of the observed depth.  expected(): their records by the loop
   of tests/scene_verify_oracle.py, computed once.

2. The slab and the plate: L, the two-coloured slab of tests/color_fit_scene.py at true_pose(), and P, a tracked plate lying on its
   top face -- the same two-coloured mesh scaled to 72 x 72 x 4 mm, centred on the top face and turned half a turn about z, so its
   colours are the swap of what lies under it.  The plate's top is 4 mm above the slab's: within TOL = 10 of it, so the plain rule
   takes the plate's pixels for the slab's and its swapped colours vote for the half-turned pose.  The frames are splatted as
   color_fit_scene.frames() does it, from both bodies.  If a change of the helper scenes ever turns the plain rule's scores around,
   the plate's scale (0.8) and thickness (4 mm) are the free parameters."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import color_fit_oracle as CO
import color_fit_scene as CS
import pose_grid_scene as SC
import scene_verify_oracle as VO
from oracle import se3_oracle as O
from oracle import ss_rules as S

RES, TOL = CO.RES, CO.TOL
H, W = CO.H, CO.W


# ---- 1. the shared cases ----------------------------------------------------------------------------------------------------------------
def _scene_image(seed, model_depth, tol):
    """a scene over a model image of the same size: mostly 0 (no tracked object), elsewhere the validity thresholds, the hidden
    boundary m + tol / m + tol + 1 and surfaces well in front of and behind the model"""
    rng = np.random.default_rng(seed)
    m = model_depth.astype(np.int64)
    s = np.zeros_like(m)
    sel = rng.random(m.shape)
    for k, v in enumerate((100, 101, 1999, 2000, m + tol, m + tol + 1, m - 30, m + 40, m)):
        on = (sel > 0.06 * k) & (sel < 0.06 * k + 0.05)
        s[on] = (v if np.isscalar(v) else v[on])
    return np.clip(s, 0, 65535).astype(np.uint16)


def _other_scene(seed, h, w):
    """a scene image of another size: a surface around the models' 600 mm, with holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    s = (600 + 45 * np.sin(xx / 11.0) + 45 * np.cos(yy / 17.0) + rng.integers(-4, 5, (h, w))).astype(np.int64)
    s[rng.random((h, w)) < 0.4] = 0
    return s.astype(np.uint16)


BOUNDARY_VALUES = ("0", "100", "101", "1999", "2000", "m+tol", "m+tol+1")
BRANCHES = ("unseen", "inlier", "front", "behind")


def _boundaries():
    """The thresholds case of color_fit_oracle (model rows 0-3: 100 / 101 / 1999 / 2000, below them 600; observed m + TOL | m + TOL + 1
    by column parity, m - TOL | m - TOL - 1 in the lower half) with the observed depth made invalid in columns 6, 7 of every 8; the
    scene holds boundary value (x // 8 + y) % 7 at (y, x) -- so each value meets invalid, inlier, in-front and behind observed pixels.
    Returns (triple, kind [176,176]: the index into BOUNDARY_VALUES)."""
    model, observed = CO.cases()["thresholds"]
    o = observed["depth"].copy()
    xs = np.arange(RES)
    o[:, (xs % 8) >= 6] = 0
    m = model["depth"].astype(np.int64)
    yy, xx = np.mgrid[0:RES, 0:RES]
    kind = (xx // 8 + yy) % 7
    table = np.stack([np.zeros_like(m), np.full_like(m, 100), np.full_like(m, 101), np.full_like(m, 1999), np.full_like(m, 2000),
                      m + TOL, m + TOL + 1])
    s = np.take_along_axis(table, kind[None], 0)[0].astype(np.uint16)
    full = (0, 0, RES, RES)
    return (model, dict(rgb=observed["rgb"], depth=o, window=full), dict(depth=s, window=full)), kind


def boundary_coverage():
    """(value name, branch) -> the number of pixels of the boundaries case with a valid model depth 600 where the scene holds that
    value and the observed depth takes that branch (the branch the pixel WOULD take without a scene)"""
    (model, observed, scene), kind = _boundaries()
    out = {}
    m, o = model["depth"].astype(int), observed["depth"].astype(int)
    for y in range(4, RES):
        for x in range(RES):
            branch = VO.classify(int(m[y, x]), int(o[y, x]), 0, TOL)
            key = (BOUNDARY_VALUES[kind[y, x]], branch)
            out[key] = out.get(key, 0) + 1
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (model, observed, scene) descriptors"""
    co = CO.cases()
    frame_scene = _scene_image(21, co["identity"][0]["depth"], TOL)               # 230 x 260, as the frames
    other = _other_scene(22, 150, 190)
    out = {}
    for k, win in CO.WINDOWS.items():                                             # the scene takes the observed descriptor's window
        out["same_" + k] = co[k] + (dict(depth=frame_scene, window=win),)
    for k in ("identity", "different"):                                           # another image size, another window, another scale
        out["other_" + k] = co[k] + (dict(depth=other, window=(5, 8, 140, 120)),)
    out["scene_miss"] = co["identity"] + (dict(depth=frame_scene, window=CO.WINDOWS["miss"]),)   # nothing hidden
    out["boundaries"] = _boundaries()[0]
    for triple in out.values():
        for c in triple:
            c["depth"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """name -> scene_verify_oracle.record() of the case at TOL"""
    return {k: VO.record(m, o, s, TOL) for k, (m, o, s) in cases().items()}


# ---- 2. the slab and the plate ----------------------------------------------------------------------------------------------------------
HW, K, STOL, OBJECT_WIDTH_MM = CS.HW, CS.K, CS.TOL, CS.OBJECT_WIDTH_MM
PLATE_SCALE = np.array([0.8, 0.8, 0.2])                                           # 72 x 72 x 4 mm
MIN_PX = 64


def plate_mesh():
    m = CS.box_mesh()
    return dict(m, vertices=m["vertices"] * PLATE_SCALE)


def plate_pose():
    """centred on the slab's top face, half a turn about z"""
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("z", 180, degrees=True).as_matrix()
    T[2, 3] = CS.HALF * (1.0 + PLATE_SCALE[2])
    return CS.true_pose() @ T


def plate_model(step=0.009):
    """(points, normals) of the plate's faces"""
    return SC._prism(CS.OUTLINE * PLATE_SCALE[:2], CS._all, -CS.HALF * PLATE_SCALE[2], CS.HALF * PLATE_SCALE[2], step)


@functools.lru_cache(maxsize=None)
def frames(seed=0):
    """(rgb uint8 [H,W,3], depth uint16 [H,W] mm): the table, the slab at true_pose() and the plate at plate_pose(), 5 % holes in the
    depth -- color_fit_scene.frames() with a second body"""
    Hs, Ws = HW
    G = CS.true_pose()
    R, t = G[:3, :3], G[:3, 3]
    n = R[:, 2]
    p0 = R @ np.array([0.0, 0.0, -CS.HALF]) + t
    vv, uu = np.mgrid[0:Hs, 0:Ws]
    ray = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones((Hs, Ws))], -1)
    z = (n @ p0) / (ray @ n)
    rgb = np.tile(CS.TABLE, (Hs, Ws, 1))
    pts, cols = [], []
    for cloud, pose in ((SC._prism(CS.OUTLINE, CS._all, -CS.HALF, CS.HALF, 0.0005)[0], G), (plate_model(0.0005)[0], plate_pose())):
        cols.append(np.where((cloud[:, 0] < 0)[:, None], CS.COLOURS[0][None, :], CS.COLOURS[1][None, :]))
        pts.append(cloud @ pose[:3, :3].T + pose[:3, 3])
    c, col = np.concatenate(pts), np.concatenate(cols)
    u = np.rint(c[:, 0] * K[0, 0] / c[:, 2] + K[0, 2]).astype(int)
    v = np.rint(c[:, 1] * K[1, 1] / c[:, 2] + K[1, 2]).astype(int)
    ok = (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
    u, v, cz, col = u[ok], v[ok], c[ok, 2], col[ok]
    np.minimum.at(z, (v, u), cz)
    win = cz == z[v, u]                                                           # the samples that won their pixel
    rgb[v[win], u[win]] = col[win]
    depth = np.rint(z * 1000.0)
    depth[(depth < 0) | (depth > 65535)] = 0
    depth = depth.astype(np.uint16)
    depth[np.random.default_rng(seed).random((Hs, Ws)) < 0.05] = 0
    rgb, depth = rgb.astype(np.uint8), depth
    rgb.setflags(write=False); depth.setflags(write=False)
    return rgb, depth


@functools.lru_cache(maxsize=None)
def oracle_scene():
    """the composed depth of the one tracked object, the plate at plate_pose(): the oracle's full-frame depth render, uint16 [H,W]
    (one layer: the composition is the layer itself)"""
    m = plate_mesh()
    d = S.render_frame(m["vertices"].astype(np.float32), (m["colors"] / 255).astype(np.float32), m["faces"], plate_pose(), K, HW[1], HW[0])[1]
    d = np.ascontiguousarray(d, np.uint16)
    d.setflags(write=False)
    return d


def crop_window(G):
    bb = O.compute_bbox(G, K, OBJECT_WIDTH_MM, (1000, 1000, 1000))
    return int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())


def triple(G, render=CS.oracle_render):
    """(model, observed, scene) descriptors of the slab hypothesis G against the frames: the 176 x 176 window render of the slab, the
    frame and the scene both under the pose's own crop window"""
    bb_gl = O.compute_bbox(G, K, OBJECT_WIDTH_MM, (1000, -1000, 1000))
    win_gl = (int(bb_gl[:, 1].min()), int(bb_gl[:, 0].min()), int(bb_gl[:, 1].max()), int(bb_gl[:, 0].max()))
    mr, md = render(G, win_gl)
    rgb, depth = frames()
    win = crop_window(G)
    return (dict(rgb=np.ascontiguousarray(mr, np.uint8), depth=np.ascontiguousarray(md).astype(np.uint16), window=(0, 0, RES, RES)),
            dict(rgb=rgb, depth=depth, window=win), dict(depth=oracle_scene(), window=win))


@functools.lru_cache(maxsize=None)
def slab_records(tol=STOL):
    """pose name -> dict(plain=(fit, colour), scene=(fit, colour)) for the hypotheses 'true' and 'flipped', by the loops alone: the
    plain rule (color_fit_oracle.record) and the scene rule (scene_verify_oracle.record), on the oracle renderer's images"""
    out = {}
    for name, G in (("true", CS.true_pose()), ("flipped", CS.flipped_pose())):
        m, o, s = triple(G)
        out[name] = dict(plain=CO.record(m, o, tol), scene=VO.record(m, o, s, tol))
    return out


def score(se3, colour_record, min_px=MIN_PX):
    """utils.color_score of one loop record"""
    rec = np.zeros(1, se3._lib.COLOR_FIT_DTYPE)
    rec["px"], rec["tol_mm"] = colour_record["px"], colour_record["tol_mm"]
    for k in VO.SUMS:
        rec[k] = colour_record[k]
    return float(se3.utils.color_score(rec, min_px)[0])
