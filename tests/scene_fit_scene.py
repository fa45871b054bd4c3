"""The inputs of the scene-fit tests (a helper module: numpy and the oracle, no device).

cases(): synthetic layer sets on a 40 x 56 frame -- the smallest on which every path of the rule and of the kernel's tiling is taken:
more than one 32 x 8 tile in both directions, unions that are no multiple of the tile, rectangles on every edge and corner.

occlusion(): the scene of the feature -- three poses of the slab of tests/color_fit_scene.py in front of the 120 x 160 camera of
tests/pose_grid_scene.py.  A stands in front of B and hides about two thirds of it; C's crop window leaves the frame on the left,
so its rectangle is clipped.  The observed frame is the composed scene +- 2 mm of uniform integer noise over a wall at 900 mm, with
5 % holes."""
import numpy as np
from scipy.spatial.transform import Rotation

import color_fit_scene as CS
from oracle import ss_rules as S

H, W = 40, 56
TOL = 10


def _layer(rng, w, h, lo=300, hi=1500, holes=0.1):
    d = rng.integers(lo, hi, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < holes] = 0
    return d


def _observed(rng, layers, rects, noise=14, holes=0.05, wall=1700):
    """the nearest valid layer value +- noise over a wall, with holes (noise > TOL: inliers, front and behind all occur)"""
    big = np.full((H, W), 1 << 30, np.int64)
    for d, (x0, y0, x1, y1) in zip(layers, rects):
        if x1 > x0 and y1 > y0:
            m = d.astype(np.int64)
            big[y0:y1, x0:x1] = np.minimum(big[y0:y1, x0:x1], np.where((m > 100) & (m < 2000), m, 1 << 30))
    o = np.where(big < (1 << 30), big + rng.integers(-noise, noise + 1, big.shape), wall)
    o[rng.random(o.shape) < holes] = 0
    return o.astype(np.uint16)


def _case(seed, rects, **kw):
    rng = np.random.default_rng(seed)
    layers = [(_layer(rng, x1 - x0, y1 - y0, **kw) if (x1 > x0 and y1 > y0) else None) for x0, y0, x1, y1 in rects]
    return dict(layers=layers, rects=[tuple(r) for r in rects], observed=_observed(rng, layers, rects), tol=TOL)


def cases():
    out = {}
    out["single"] = _case(1, [(5, 3, 45, 30)])
    # model depths 100 / 101 / 1999 / 2000 and |o - m| at tol and tol + 1 on either side, column by column
    m = np.tile(np.array([100, 101, 1999, 2000, 500, 500, 500, 500], np.uint16), (H, W // 8))
    o = np.tile(np.array([500, 101 + TOL, 1999 - TOL, 500, 500 + TOL, 500 + TOL + 1, 500 - TOL, 500 - TOL - 1], np.uint16), (H, W // 8))
    o[1::4] = 100; o[2::4] = 2000; o[3::4] = 0                                 # observed depths that are not valid
    out["thresholds"] = dict(layers=[m], rects=[(0, 0, W, H)], observed=o, tol=TOL)
    same = _layer(np.random.default_rng(2), W, H)
    out["ties"] = dict(layers=[same, same.copy()], rects=[(0, 0, W, H)] * 2, observed=_observed(np.random.default_rng(3), [same], [(0, 0, W, H)]),
                       tol=TOL)
    out["one_px"] = _case(4, [(17, 9, 18, 10), (10, 5, 30, 20)], holes=0.0)
    out["edges"] = _case(5, [(0, 0, 10, 8), (46, 0, 56, 8), (0, 32, 10, 40), (46, 32, 56, 40), (20, 0, 36, 3), (20, 37, 36, 40), (0, 12, 3, 28),
                             (53, 12, 56, 28), (0, 0, W, H)])
    out["gap"] = _case(6, [(2, 2, 12, 12), (40, 25, 54, 38)])
    out["empty_among"] = _case(7, [(4, 4, 30, 30), (0, 0, 0, 0), (20, 10, 50, 36), (9, 30, 9, 35)])
    out["all_empty"] = _case(8, [(0, 0, 0, 0), (5, 5, 5, 9), (7, 3, 2, 9)])
    out["n32"] = _case(9, [(i, i // 4, i + 20, i // 4 + 25) for i in range(32)], lo=600, hi=700)
    z = _case(10, [(3, 2, 40, 30), (20, 10, 52, 39)])
    z["observed"] = np.zeros((H, W), np.uint16)
    out["zeros_observed"] = z
    out["overlap_odd"] = _case(11, [(3, 2, 41, 30), (20, 11, 52, 39), (10, 5, 33, 17)])   # union 49 x 37: 2 x 5 tiles, none of them full
    return out


def random_layers(seed, n, ties=True):
    """n random rectangles of random depths; ties=False: every layer's values are congruent to its index modulo n, so no two
    layers ever hold the same value"""
    rng = np.random.default_rng(seed)
    rects = []
    for _ in range(n):
        x0, y0 = int(rng.integers(0, W - 4)), int(rng.integers(0, H - 4))
        rects.append((x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))))
    layers = [_layer(rng, x1 - x0, y1 - y0, lo=400, hi=480 if ties else 1200) for x0, y0, x1, y1 in rects]
    if not ties:
        layers = [np.where(d > 0, (d.astype(np.int64) // n) * n + i, 0).astype(np.uint16) for i, d in enumerate(layers)]
    return dict(layers=layers, rects=rects, observed=_observed(rng, layers, rects), tol=TOL)


# ---- the occlusion scene ------------------------------------------------------------------------------------------------------------
HW, K = CS.HW, CS.K
OBJECT_WIDTH_MM = CS.OBJECT_WIDTH_MM
WALL_MM = 900
POSES = {"A": ((0.030, 0.004, 0.42), 150, 10), "B": ((-0.005, 0.0, 0.50), 140, 25), "C": ((-0.2, 0.0, 0.5), 140, 0)}


def pose(t, rx, rz):
    G = np.eye(4)
    G[:3, :3] = (Rotation.from_euler("x", rx, degrees=True) * Rotation.from_euler("z", rz, degrees=True)).as_matrix()
    G[:3, 3] = t
    return G


def scene_poses(names="ABC"):
    return np.stack([pose(*POSES[k]) for k in names])


def slab_mesh():
    return CS.box_mesh()


def block_mesh():
    """a second mesh: the slab's faces stretched into a 54 x 108 x 40 mm block"""
    m = CS.box_mesh()
    return dict(m, vertices=m["vertices"] * np.array([0.6, 1.2, 2.0]))


def oracle_depth(mesh, G, hw=None, k=None):
    """the full-frame depth render of the oracle (uint16 [H,W] mm): geometry only"""
    h, w = hw or HW
    return S.render_frame(mesh["vertices"].astype(np.float32), (mesh["colors"] / 255).astype(np.float32), mesh["faces"], G,
                          K if k is None else k, w, h)[1]


def oracle_layers(se3, meshes, poses, widths, hw=None, k=None):
    """per object (layer, rect): the oracle's render cut to se3tn_frame_rect's rectangle of the pose"""
    h, w = hw or HW
    k = K if k is None else k
    layers, rects = [], []
    for mesh, G, width in zip(meshes, poses, widths):
        x0, y0, x1, y1 = se3.frame_rect(G, k, width, h, w) or (0, 0, 0, 0)        # (None: the window misses the frame)
        rects.append((x0, y0, x1, y1))
        layers.append(np.ascontiguousarray(oracle_depth(mesh, G, (h, w), k)[y0:y1, x0:x1]) if (x1 > x0 and y1 > y0) else None)
    return layers, rects


def observe(scene, seed=0):
    """a composed depth image as the sensor would deliver it: +- 2 mm uniform integer noise over the wall, 5 % holes"""
    rng = np.random.default_rng(seed)
    s = scene.astype(np.int64)
    obs = np.where(s > 0, s + rng.integers(-2, 3, s.shape), WALL_MM)
    obs[rng.random(obs.shape) < 0.05] = 0
    return obs.astype(np.uint16)


_OCCLUSION = {}


def occlusion(se3):
    """dict(poses [3,4,4], layers, rects, observed, observed_without_A): computed once"""
    if not _OCCLUSION:
        poses = scene_poses()
        layers, rects = oracle_layers(se3, [slab_mesh()] * 3, poses, [OBJECT_WIDTH_MM] * 3)
        zero = np.zeros(HW, np.uint16)
        scene = se3.utils.scene_stats(layers, rects, zero, TOL)[2]
        without_a = se3.utils.scene_stats(layers[1:], rects[1:], zero, TOL)[2]
        _OCCLUSION.update(poses=poses, layers=layers, rects=rects, observed=observe(scene), observed_without_A=observe(without_a))
    return _OCCLUSION


def make_tracker(se3, mesh, width, seed=0, full_frame=False):
    """a Tracker with random-init fixture weights on the scene's camera, the built-in rasteriser on `mesh`"""
    from oracle import fixtures as Fx
    from oracle import se3_oracle as O
    h, w = HW
    info = dict(Fx.DATASET_INFO, object_width=width,
                camera=dict(height=h, width=w, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
    mean, std = Fx.mean_std(seed)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(seed, head_gain=0.01)}, max_samples=1)
    trk.renderer = se3.HipRenderer(trk.engine, mesh, mode="pyrender", frame_size=HW) if full_frame else se3.HipRenderer(trk.engine, mesh)
    return trk
