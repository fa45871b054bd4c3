"""The scene of the pose grid tests (a helper module, numpy only): a thin L-shaped box lying on a tilted table plane beside one clutter
box, seen by the 120 x 160 camera of the renderer tests, with 5 % holes in the depth frame.  The L is 20 mm thick -- twice the
10 mm tolerance of the search -- so that a score which counts the far side of the model prefers to lay it INTO the table, where
both of its large faces pass as inliers, over the true pose, where the lower face is hidden behind the upper one.

The model carries analytic normals (the face a point was sampled on).  The frame is splatted from dense samples of the same faces
(0.5 mm apart, a pixel is about 2 mm wide at the object's distance) over the plane's closed-form depth."""
import numpy as np
from scipy.spatial.transform import Rotation

HW = (120, 160)
K = np.array([[266.7, 0, 78.2], [0, 266.9, 60.3], [0, 0, 1.0]])
HALF = 0.015                                                                     # half the thickness of the L
OUTLINE = np.array([(-0.06, -0.05), (0.06, -0.05), (0.06, -0.01), (-0.02, -0.01), (-0.02, 0.05), (-0.06, 0.05)])   # counter-clockwise
CLUTTER = ((0.065, 0.115), (0.035, 0.085), (-HALF, 0.05))                          # x, y, z ranges of the clutter box, object frame
TOL = 10


def true_pose():
    """the L flat on the table: its z axis (the table's normal) tilted 40 degrees from the optical axis towards the camera"""
    G = np.eye(4)
    G[:3, :3] = (Rotation.from_euler("x", 140, degrees=True) * Rotation.from_euler("z", 25, degrees=True)).as_matrix()
    G[:3, 3] = (0.012, 0.004, 0.5)
    return G


def _inside(xy):
    x, y = xy[:, 0], xy[:, 1]
    return ((x > -0.06) & (x < 0.06) & (y > -0.05) & (y < -0.01)) | ((x > -0.06) & (x < -0.02) & (y > -0.05) & (y < 0.05))


def _cells(a, b, step):
    """centres of the cells of [a, b] cut into round((b - a) / step) equal parts"""
    n = max(int(round((b - a) / step)), 1)
    return a + (np.arange(n) + 0.5) * (b - a) / n


def _prism(outline, inside, z0, z1, step):
    """(points, normals) sampled on the faces of the prism outline x [z0, z1]: cell centres, about `step` apart"""
    lo, hi = outline.min(0), outline.max(0)
    gx, gy = np.meshgrid(_cells(lo[0], hi[0], step), _cells(lo[1], hi[1], step), indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], 1)
    xy = xy[inside(xy)]
    pts, nrm = [], []
    for z, nz in ((z1, 1.0), (z0, -1.0)):
        pts.append(np.column_stack([xy, np.full(len(xy), z)]))
        nrm.append(np.tile([0.0, 0.0, nz], (len(xy), 1)))
    for a, b in zip(outline, np.roll(outline, -1, axis=0)):
        e = b - a
        ln = np.linalg.norm(e)
        s, zz = np.meshgrid(_cells(0.0, ln, step), _cells(z0, z1, step), indexing="ij")
        p = a[None, :] + s.ravel()[:, None] * (e / ln)[None, :]
        pts.append(np.column_stack([p, zz.ravel()]))
        nrm.append(np.tile([e[1] / ln, -e[0] / ln, 0.0], (s.size, 1)))           # outward of a counter-clockwise outline
    return np.concatenate(pts), np.concatenate(nrm)


def l_model(step=0.009):
    """(points [P,3], normals [P,3]) of the L: about 300 points at the default spacing"""
    return _prism(OUTLINE, _inside, -HALF, HALF, step)


def _clutter(step):
    (x0, x1), (y0, y1), (z0, z1) = CLUTTER
    outline = np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
    return _prism(outline, lambda xy: np.ones(len(xy), bool), z0, z1, step)[0]


def l_mesh():
    """the L as a triangle mesh for the rasteriser (two overlapping boxes, vertex colours, no normals): image A of the network"""
    verts, faces = [], []
    for (x0, x1), (y0, y1) in (((-0.06, 0.06), (-0.05, -0.01)), ((-0.06, -0.02), (-0.05, 0.05))):
        base = len(verts)
        verts += [(x, y, z) for z in (-HALF, HALF) for y in (y0, y1) for x in (x0, x1)]
        quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]               # outward
        for q in quads:
            faces += [(base + q[0], base + q[1], base + q[2]), (base + q[0], base + q[2], base + q[3])]
    verts = np.array(verts, np.float64)
    rng = np.random.default_rng(5)
    return dict(vertices=verts, faces=np.array(faces, np.int32), colors=rng.integers(40, 255, (len(verts), 3)).astype(np.float64),
                normals=None)


def frame(seed=0):
    """depth [H,W] uint16 millimetres: the table plane, the clutter box and the L at true_pose(), 5 % holes"""
    H, W = HW
    G = true_pose()
    R, t = G[:3, :3], G[:3, 3]
    n = R[:, 2]                                                                  # the table's normal, towards the camera
    p0 = R @ np.array([0.0, 0.0, -HALF]) + t                                    # a point of the table: under the L
    vv, uu = np.mgrid[0:H, 0:W]
    ray = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    z = (n @ p0) / (ray @ n)
    for cloud in (l_model(0.0005)[0], _clutter(0.0005)):
        c = cloud @ R.T + t
        u = np.rint(c[:, 0] * K[0, 0] / c[:, 2] + K[0, 2]).astype(int)
        v = np.rint(c[:, 1] * K[1, 1] / c[:, 2] + K[1, 2]).astype(int)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        np.minimum.at(z, (v[ok], u[ok]), c[ok, 2])
    depth = np.rint(z * 1000.0)
    depth[(depth < 0) | (depth > 65535)] = 0
    depth = depth.astype(np.uint16)
    depth[np.random.default_rng(seed).random((H, W)) < 0.05] = 0
    return depth
