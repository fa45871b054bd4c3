"""The scene of the scene-aware search tests (a helper module: numpy and the oracle, no device), built from the slab of
tests/color_fit_scene.py in front of the 120 x 160 camera of tests/pose_grid_scene.py:

  a table      a 186 x 94 x 20 mm top, tilted as the table of pose_grid_scene -- it ends just beyond the slabs, so that no
               candidate finds a free stretch of it to sink into;
  T and L      two slabs of the SAME model side by side on it, 92 mm apart (2 mm between them): T is tracked, L is lost;
  O            a third slab, tracked, held between the camera and L: it covers well over half of L;
  last         where L was last seen: between the two places, so that the default lattice (+- 50 mm in steps of 10) holds the true
               place of L exactly (node +4, -1, +1) and the place of T within a step.

frame() is what the sensor delivers (every surface composed, +- 2 mm integer noise over a wall at 900 mm, 5 % holes); scene() is what
se3tn_scene_fit composes of the tracked objects T and O alone (0 elsewhere).  The renders are the oracle's full-frame depth
(tests/scene_fit_scene.oracle_depth): geometry only."""
import numpy as np

import color_fit_scene as CS
import pose_grid_scene as SC
import scene_fit_scene as SF

HW, K, TOL = SC.HW, SC.K, SC.TOL
OBJECT_WIDTH_MM = CS.OBJECT_WIDTH_MM
SPACING = 0.092                                   # between the centres of T and L, along the table's x axis
ORIGIN = np.array([0.0, 0.004, 0.5])              # the table point midway between T and L, camera frame
LAST_OFFSET = np.array([0.04, -0.01, 0.01])       # true place of L minus the place it was last seen: a lattice node (trans_step 0.01)
TRANS_STEP = 0.01
NAMES = ("T", "L", "O")                           # object order of the tests: T and O are tracked, L (index 1) is lost


def _on_table(xyz):
    """the pose of a slab lying flat on the table with its centre at table coordinates xyz"""
    G = SC.true_pose()
    G[:3, 3] = ORIGIN + G[:3, :3] @ np.asarray(xyz, np.float64)
    return G


def poses():
    """dict T, L, O, last -> 4x4 poses (object in camera, metres)"""
    out = dict(T=_on_table((-SPACING / 2, 0.0, 0.0)), L=_on_table((SPACING / 2, 0.0, 0.0)))
    out["O"] = SF.pose((0.062, 0.012, 0.40), 150, 10)
    last = out["L"].copy()
    last[:3, 3] -= LAST_OFFSET
    out["last"] = last
    return out


def slab_mesh():
    return CS.box_mesh()


def slab_model():
    """(points [280,3], normals [280,3]) of the slab: what the search scores"""
    return CS.box_model()


def table_mesh():
    m = CS.box_mesh()
    return dict(m, vertices=m["vertices"] * np.array([186.0 / 90.0, 94.0 / 90.0, 1.0]))


def table_pose():
    return _on_table((0.0, 0.0, -2 * CS.HALF))                                   # its top is the slabs' lower face


def compose(layers):
    """the nearest valid (100 < d < 2000) depth of full-frame layers, 0 where there is none: scene(p) of include/se3tracknet.h"""
    out = np.zeros(HW, np.uint16)
    for d in layers:
        ok = (d > 100) & (d < 2000) & ((out == 0) | (d < out))
        out[ok] = d[ok]
    return out


_CACHE = {}


def renders():
    """dict table, T, L, O -> the oracle's full-frame depth of each, uint16 [H,W] mm; computed once"""
    if not _CACHE:
        P = poses()
        _CACHE.update(table=SF.oracle_depth(table_mesh(), table_pose()), **{k: SF.oracle_depth(slab_mesh(), P[k]) for k in NAMES})
    return _CACHE


def frame(seed=0):
    """the observed depth, uint16 [H,W] mm"""
    r = renders()
    return SF.observe(compose([r["table"], r["T"], r["L"], r["O"]]), seed)


def scene():
    """the composed depth of the tracked objects T and O, uint16 [H,W] mm, 0 elsewhere"""
    r = renders()
    return compose([r["T"], r["O"]])


def covered_share():
    """the share of L's rendered pixels at which O is nearer"""
    r = renders()
    on = r["L"] > 0
    return float(((r["O"] > 0) & (r["O"] < r["L"]) & on).sum()) / float(on.sum())


# ---- the small cases: a scene frame that sits on every edge of `hidden` --------------------------------------------------------------
BOUNDARY = (0, 100, 101, 1999, 2000)


def pixels_of(pts, R, t, k):
    """(uf, vf, m) of the points under [R | t], in the rule's operation order (facing not applied)"""
    k = np.asarray(k, np.float64).reshape(9)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    c = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)]
    with np.errstate(all="ignore"):
        return np.rint(c[0] * k[0] / c[2] + k[2]), np.rint(c[1] * k[4] / c[2] + k[5]), np.rint(c[2] * 1000.0)


def boundary_scene(case, tol):
    """The scene frame of a case (pts, nrm, rots, trans, depth, K) for tolerance `tol`: random tracked surfaces around the candidates'
    depths over a third of the frame, the boundary values 0, 100, 101, 1999 and 2000, and -- under candidate (rotation 0,
    translation 0) -- one point's pixel holding exactly m + tol (hidden) and another's m + tol + 1 (not hidden).  Returns (scene,
    [(pixel, m)] of those two points)."""
    pts, _, rots, trans, depth, k = case
    H, W = depth.shape
    rng = np.random.default_rng(11)
    scene = np.zeros((H, W), np.uint16)
    mask = rng.random((H, W)) < 0.35
    scene[mask] = rng.integers(440, 560, int(mask.sum()))
    edge = rng.random((H, W)) < 0.15
    scene[edge] = rng.choice(np.array(BOUNDARY, np.uint16), int(edge.sum()))
    uf, vf, m = pixels_of(pts, rots[0], trans[0], k)
    inside = np.flatnonzero((uf >= 0) & (uf < W) & (vf >= 0) & (vf < H))
    pix = {}
    for j in inside:
        pix.setdefault((int(vf[j]), int(uf[j])), []).append(j)
    own = [js[0] for js in pix.values() if len(js) == 1][:2]                     # two points that own their pixel
    assert len(own) == 2
    marks = []
    for j, extra in zip(own, (0, 1)):
        scene[int(vf[j]), int(uf[j])] = int(m[j]) + tol + extra
        marks.append(((int(vf[j]), int(uf[j])), int(m[j])))
    free = [(v, u) for v in range(H) for u in range(W) if (v, u) not in pix][:len(BOUNDARY)]
    for val, at in zip(BOUNDARY, free):                                          # every boundary value is there whatever the draw
        scene[at] = val
    return scene, marks


def device_case():
    """The smallest shapes that cross every boundary of the kernel, on the 24 x 32 frame of small_case() in
    tests/test_pose_grid_host.py: P = 1,100 points (one full tile of 1,024 and a 76-point tail that is no multiple of 64), 19
    translations (one full tile of 16 and a tail of 3 that leaves one wave idle; translation 3 lies behind the camera), 3 rotations
    (rotation 2 carries a NaN).  -> (pts, nrm, rots, trans, depth, K)"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    H, W = 24, 32
    k = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1.0]])
    depth = rng.integers(480, 520, (H, W)).astype(np.uint16)
    mask = rng.random((H, W)) < 0.2
    depth[mask] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    pts = rng.uniform(-0.05, 0.05, (1100, 3))
    pts[:40] *= 0.1                                                              # a sparse core: some points own their pixel
    nrm = pts / np.linalg.norm(pts, axis=1)[:, None]
    nrm[5] = 0.0
    rots = np.array([Rotation.from_rotvec(v).as_matrix() for v in ((0.2, -0.1, 0.3), (1.0, 2.0, -0.5), (0.0, 0.4, 0.0))])
    rots[2, 1, 1] = np.nan
    trans = np.column_stack([rng.uniform(-0.03, 0.03, 19), rng.uniform(-0.03, 0.03, 19), rng.uniform(0.45, 0.55, 19)])
    trans[0] = (0.0, 0.0, 0.5)
    trans[3] = (0.0, 0.0, -0.5)
    return pts, nrm, rots, trans, depth, k
