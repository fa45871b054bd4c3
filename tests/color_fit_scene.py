"""The scene of the colour tests (a helper module: numpy and the oracle, no device): a box that a half turn about its z axis maps onto itself, its two
halves (x < 0, x > 0) in different constant colours, lying on the tilted table of tests/pose_grid_scene.py and seen by the same
120 x 160 camera.  The depth frame cannot tell the true pose from the half-turned one -- the model points and the surface are the same
set -- the colour frame can.

The mesh carries every face with its own four vertices (flat normals, one colour per half): no vertex is shared across the seam, so
nothing interpolates across it.  The frames are splatted as pose_grid_scene.frame does it -- dense samples of the faces (0.5 mm apart)
over the plane's closed-form depth -- the colour frame from the same samples: where a sample wins the depth test its half's colour is
written."""
import numpy as np
from scipy.spatial.transform import Rotation

import pose_grid_scene as SC
from oracle import se3_oracle as O
from oracle import ss_rules as S

HW, K, TOL = SC.HW, SC.K, SC.TOL
# A square slab, 90 x 90 x 20 mm.  The proportions are chosen for the SEARCH, not for the colour rule: a quarter turn keeps the shape too,
# so the depth frame offers four orientations and Tracker.acquire's pool (ACQUIRE below) holds all of them, the true one included; on a
# 100 x 60 x 30 mm box the depth search itself ended 48 degrees off (rolled about the long edge, 17 mm aside, 115 of the true pose's 125
# inliers), which no choice among its hypotheses can mend.
HALF = 0.010
BOX = ((-0.045, 0.045), (-0.045, 0.045), (-HALF, HALF))
OUTLINE = np.array([(-0.045, -0.045), (0.045, -0.045), (0.045, 0.045), (-0.045, 0.045)])      # counter-clockwise
COLOURS = (np.array([215, 60, 40]), np.array([40, 90, 210]))                                    # the half x < 0, the half x > 0
TABLE = np.array([120, 110, 100])
OBJECT_WIDTH_MM = 150.0


def true_pose():
    return SC.true_pose()


def flipped_pose():
    """the true pose after half a turn about the box's z axis: the same surface, the colours exchanged"""
    G = true_pose()
    G[:3, :3] = G[:3, :3] @ Rotation.from_euler("z", 180, degrees=True).as_matrix()
    return G


def _all(xy):
    return np.ones(len(xy), bool)


def box_model(step=0.009):
    """(points [P,3], normals [P,3]) of the box's faces: what the pose search scores"""
    return SC._prism(OUTLINE, _all, -HALF, HALF, step)


def box_mesh():
    """the two halves as triangles: per half the five outer faces, each with its own four vertices and its flat normal"""
    verts, normals, colours, faces = [], [], [], []
    (x0, x1), (y0, y1), (z0, z1) = BOX
    for half, (xa, xb) in enumerate(((x0, 0.0), (0.0, x1))):
        quads = [((0, 0, 1.0), [(xa, y0, z1), (xb, y0, z1), (xb, y1, z1), (xa, y1, z1)]),
                 ((0, 0, -1.0), [(xa, y0, z0), (xb, y0, z0), (xb, y1, z0), (xa, y1, z0)]),
                 ((0, -1.0, 0), [(xa, y0, z0), (xb, y0, z0), (xb, y0, z1), (xa, y0, z1)]),
                 ((0, 1.0, 0), [(xa, y1, z0), (xb, y1, z0), (xb, y1, z1), (xa, y1, z1)])]
        xo = x0 if half == 0 else x1
        quads.append(((-1.0 if half == 0 else 1.0, 0, 0), [(xo, y0, z0), (xo, y1, z0), (xo, y1, z1), (xo, y0, z1)]))
        for n, q in quads:
            q, n = np.array(q), np.array(n)
            if np.cross(q[1] - q[0], q[2] - q[0]) @ n < 0:                               # counter-clockwise seen from outside
                q = q[::-1]
            base = len(verts)
            verts += list(q)
            normals += [n] * 4
            colours += [COLOURS[half]] * 4
            faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return dict(vertices=np.array(verts, np.float64), faces=np.array(faces, np.int32), colors=np.array(colours, np.float64),
                normals=np.array(normals, np.float64))


def frames(seed=0):
    """(rgb uint8 [H,W,3], depth uint16 [H,W] mm): the table and the box at true_pose(), 5 % holes in the depth"""
    H, W = HW
    G = true_pose()
    R, t = G[:3, :3], G[:3, 3]
    n = R[:, 2]
    p0 = R @ np.array([0.0, 0.0, -HALF]) + t
    vv, uu = np.mgrid[0:H, 0:W]
    ray = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    z = (n @ p0) / (ray @ n)
    rgb = np.tile(TABLE, (H, W, 1))
    cloud = SC._prism(OUTLINE, _all, -HALF, HALF, 0.0005)[0]
    col = np.where((cloud[:, 0] < 0)[:, None], COLOURS[0][None, :], COLOURS[1][None, :])
    c = cloud @ R.T + t
    u = np.rint(c[:, 0] * K[0, 0] / c[:, 2] + K[0, 2]).astype(int)
    v = np.rint(c[:, 1] * K[1, 1] / c[:, 2] + K[1, 2]).astype(int)
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    u, v, cz, col = u[ok], v[ok], c[ok, 2], col[ok]
    np.minimum.at(z, (v, u), cz)
    win = cz == z[v, u]                                                                  # the samples that won their pixel
    rgb[v[win], u[win]] = col[win]
    depth = np.rint(z * 1000.0)
    depth[(depth < 0) | (depth > 65535)] = 0
    depth = depth.astype(np.uint16)
    depth[np.random.default_rng(seed).random((H, W)) < 0.05] = 0
    return rgb.astype(np.uint8), depth


# ---- the two poses against the frames, by the NumPy rule ----------------------------------------------------------------------------
def records(se3, render):
    """(fit [2], colour [2]) of [true, flipped]: `render(pose, gl_window)` -> the 176 x 176 model image, against O.crop_bbox of the
    frames at the pose's own bbox, by the NumPy rule"""
    rgb, depth = frames()
    fit, col = [], []
    for G in (true_pose(), flipped_pose()):
        bb_gl = O.compute_bbox(G, K, OBJECT_WIDTH_MM, (1000, -1000, 1000))
        win = (int(bb_gl[:, 1].min()), int(bb_gl[:, 0].min()), int(bb_gl[:, 1].max()), int(bb_gl[:, 0].max()))
        mr, md = render(G, win)
        orr, od = O.crop_bbox(rgb, depth, O.compute_bbox(G, K, OBJECT_WIDTH_MM, (1000, 1000, 1000)))
        fit.append(se3.utils.fit_stats(md, od, TOL))
        col.append(se3.utils.color_stats(mr, md, orr, od, TOL))
    return np.stack(fit), np.stack(col)


def oracle_render(G, win):
    mesh = box_mesh()
    return S.render_vispy(mesh["vertices"].astype(np.float32), mesh["normals"].astype(np.float32), (mesh["colors"] / 255.0).astype(np.float32),
                          mesh["faces"], G, K, win, numpy_rule="numpy1")


# ---- the tracker of the scene -------------------------------------------------------------------------------------------------------
ACQUIRE = dict(inplane=24, stride=8, tol_mm=TOL, top=8, refine=0, align=20)      # the search both the test and the recorded parent pose ran
SEARCH_STEP_DEG = 15.0                                               # the rotation step the search's lattices end at (recover.lattice_factors)
GOLDEN_ACQUIRE = "color_fit_acquire_parent.npz"                      # tests/golden: acquire(**ACQUIRE) of the commit before the colour switch


def make_tracker(se3, directory):
    """Random-init fixture weights, max_samples = 8, object_cloud and object_normals from a .ply of box_model() written into
    `directory`, the built-in rasteriser on box_mesh()"""
    import os
    from oracle import fixtures as Fx
    Hs, Ws = HW
    info = dict(Fx.DATASET_INFO, object_width=OBJECT_WIDTH_MM,
                camera=dict(height=Hs, width=Ws, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))
    pts, nrm = box_model()
    ply = os.path.join(str(directory), "box.ply")
    with open(ply, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % len(pts))
        f.write("".join("property double %s\n" % k for k in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n")
        for v, n in zip(pts, nrm):
            f.write("%.17g %.17g %.17g %.17g %.17g %.17g\n" % (tuple(v) + tuple(n)))
    mean, std = Fx.mean_std(0)
    trk = se3.Tracker(info, mean, std, {"state_dict": O.make_state_dict(0, head_gain=0.01)}, model_path=ply, max_samples=8)
    trk.renderer = se3.HipRenderer(trk.engine, box_mesh())
    return trk


def rotation_error_deg(pose):
    """the angle between a pose's rotation and the true one, up to the symmetry the box really has: half a turn about its x axis
    maps the box AND its colours onto themselves (each half stays on its side), so no frame can tell those two apart"""
    Rt = true_pose()[:3, :3]
    out = []
    for sym in (np.eye(3), Rotation.from_euler("x", 180, degrees=True).as_matrix()):
        c = (np.trace((Rt @ sym).T @ np.asarray(pose)[:3, :3]) - 1.0) / 2.0
        out.append(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    return min(out)
