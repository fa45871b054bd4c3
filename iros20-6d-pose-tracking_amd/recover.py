"""Re-acquiring a lost object: the candidate poses ``Tracker.recover`` searches and the order it ranks them in.

The reference re-initialises a lost track from an external detector (PoseCNN at the frames ``--reinit_frames`` lists,
predict.py:539-541).  Without one, the search is local: a lattice of poses around the last pose the track had, every candidate
scored against the observed depth frame on the device (``Engine.score_poses`` -> se3tn_score_poses / se3tn_rank_poses), the best few
pulled in by the network (``Tracker.on_track_batch``) and scored once more.

With no pose at all (``Tracker.acquire``) the search is global: ``rotation_grid`` x ``depth_seeds`` -- rotations that cover SO(3)
times translations seeded from the depth frame itself -- scored as a product (``Engine.score_pose_grid`` -> se3tn_score_pose_grid)
counting only the model points that face the camera, then the local lattice (``lattice_factors``) around the best few.
"""
import numpy as np

KEY_FIELD_MAX = (1 << 20) - 1   # as csrc/pose_search_plan.h: the two 20-bit fields of a key


def pose_key(fit, index=None):
    """The 64-bit key se3tn_rank_poses orders records by (csrc/pose_search_plan.h ps_key), as Python ints in an object array:
    inlier_pts * 2^40 + (2^20 - 1 - min(behind_pts, 2^20 - 1)) * 2^20 + (2^20 - 1 - index); index defaults to the record's place.
    More inliers first, then fewer seen-through points, then the lower index.  Reads inlier_pts and behind_pts only: records of
    _lib.POINT_FIT_DTYPE and of _lib.SCENE_POINT_FIT_DTYPE (the scene-aware searches) alike."""
    fit = np.atleast_1d(fit)
    idx = np.arange(len(fit)) if index is None else np.atleast_1d(index)
    return np.array([(min(int(f["inlier_pts"]), KEY_FIELD_MAX + 1) << 40) + ((KEY_FIELD_MAX - min(int(f["behind_pts"]), KEY_FIELD_MAX)) << 20)
                     + (KEY_FIELD_MAX - int(i)) for f, i in zip(fit, idx)], dtype=object)


def _rotation(axis, angle_deg):
    """Rotation by angle_deg about camera axis 0 | 1 | 2 (right-handed)"""
    a = np.deg2rad(float(angle_deg))
    c, s = np.cos(a), np.sin(a)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[i, i] = c; R[i, j] = -s; R[j, i] = s; R[j, j] = c
    return R


def pose_lattice(base, trans_radius=0.05, trans_step=0.01, rot_deg=(15.0,)):
    """Deterministic candidates [n,4,4] around the pose `base` (4x4 object-in-camera, metres), in the CAMERA frame:
    R = dR . R_base, t = t_base + dt.  The enumeration order is part of the contract (se3tn_rank_poses breaks ties by index):
      rotations outermost -- identity first, then for each angle a of rot_deg: +a, -a about camera x, +a, -a about y, +a, -a about z;
      translations dt over the cubic grid {-r, .., r}^3 in steps of trans_step, r = round(trans_radius / trans_step) steps,
      x outermost, z innermost, ascending (dt = i * trans_step with integer i: the grid is symmetric and holds 0 exactly).
    n = (2 r + 1)^3 * (1 + 6 len(rot_deg)); the base pose itself is candidate ((r (2r + 1) + r) (2r + 1)) + r."""
    rots, trans = lattice_factors(base, trans_radius, trans_step, rot_deg)
    m = len(trans)
    out = np.tile(np.eye(4), (len(rots) * m, 1, 1))
    for q, R in enumerate(rots):
        out[q * m:(q + 1) * m, :3, :3] = R
        out[q * m:(q + 1) * m, :3, 3] = trans
    return out


def lattice_factors(base, trans_radius=0.05, trans_step=0.01, rot_deg=(15.0,)):
    """pose_lattice as the product it is: (rots [n_r,3,3], trans [n_t,3]) with candidate r * n_t + t of pose_lattice(...) being
    [rots[r] | trans[t]], bit for bit -- rots[r] = dR_r . R_base in pose_lattice's rotation order (identity first), trans[t] =
    t_base + dt_t in its translation order (x outermost, z innermost).  What Engine.score_pose_grid takes instead of n poses."""
    base = np.asarray(base, np.float64).reshape(4, 4)
    if not (trans_step > 0 and trans_radius >= 0):
        raise ValueError("pose_lattice: trans_step must be > 0 and trans_radius >= 0")
    r = int(round(float(trans_radius) / float(trans_step)))
    steps = np.arange(-r, r + 1, dtype=np.float64) * float(trans_step)
    gx, gy, gz = np.meshgrid(steps, steps, steps, indexing="ij")          # x outermost, z innermost
    dts = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    rots = [np.eye(3)]
    for a in rot_deg:
        for axis in range(3):
            rots += [_rotation(axis, +a), _rotation(axis, -a)]
    return np.array([dR @ base[:3, :3] for dR in rots]), base[:3, 3] + dts


GOLDEN_ANGLE = np.pi * (3.0 - np.sqrt(5.0))


def rotation_grid(n_views, n_inplane):
    """Deterministic rotations [n_views * n_inplane, 3, 3] (object -> camera) that cover SO(3) evenly: a Fibonacci lattice of view
    directions times equally spaced turns about the optical axis.  Order: views outermost, in-plane turns innermost --
    rotation v * n_inplane + p is Rz(2 pi p / n_inplane) . V_v.
      view v:  the object-frame direction d_v = (s cos(v g), s sin(v g), z_v),  z_v = 1 - (2 v + 1) / n_views,  s = sqrt(1 - z_v^2),
               g the golden angle pi (3 - sqrt 5), points at the camera: V_v has the rows e1 = (0,0,1) x e3 / |.|, e2 = e3 x e1,
               e3 = -d_v, so V_v d_v = (0, 0, -1) and det V_v = +1 (|z_v| < 1 for every v: the cross product never vanishes);
      turn p:  Rz(a) = [[cos a, -sin a, 0], [sin a, cos a, 0], [0, 0, 1]] in the camera frame.
    Neighbouring views are about sqrt(4 pi / n_views) rad apart, neighbouring turns 2 pi / n_inplane."""
    n_views, n_inplane = int(n_views), int(n_inplane)
    if n_views < 1 or n_inplane < 1:
        raise ValueError("rotation_grid: n_views and n_inplane must be >= 1")
    out = np.empty((n_views * n_inplane, 3, 3))
    for v in range(n_views):
        z = 1.0 - (2.0 * v + 1.0) / n_views
        s = np.sqrt(1.0 - z * z)
        d = np.array([s * np.cos(v * GOLDEN_ANGLE), s * np.sin(v * GOLDEN_ANGLE), z])
        e3 = -d / np.linalg.norm(d)
        e1 = np.cross([0.0, 0.0, 1.0], e3)
        e1 /= np.linalg.norm(e1)
        V = np.stack([e1, np.cross(e3, e1), e3])
        for p in range(n_inplane):
            out[v * n_inplane + p] = _rotation(2, 360.0 * p / n_inplane) @ V
    return out


def depth_seeds(depth_mm, K, stride=16, behind_m=0.03, roi=None):
    """Candidate translations [n,3] (metres, camera frame) for an object somewhere in a depth frame: one per VALID pixel
    (100 < d < 2000, the validity rule of the scoring) of the grid v = top, top + stride, ... < bottom, u = left, left + stride, ...
    < right, in row-major order (v outermost), back-projected along the pixel's ray to the depth z = d / 1000 + behind_m -- the
    object's centre lies behind the surface the sensor sees:  x = (u - K[0,2]) * z / K[0,0],  y = (v - K[1,2]) * z / K[1,1].
    roi = (left, top, right, bottom) in pixels, clipped to the frame (default: the whole frame)."""
    d = np.asarray(depth_mm)
    if d.ndim != 2:
        raise ValueError("depth_seeds: depth must be [H,W]")
    stride = int(stride)
    if stride < 1:
        raise ValueError("depth_seeds: stride must be >= 1")
    K = np.asarray(K, np.float64).reshape(3, 3)
    H, W = d.shape
    left, top, right, bottom = (0, 0, W, H) if roi is None else [int(x) for x in roi]
    left, top, right, bottom = max(left, 0), max(top, 0), min(right, W), min(bottom, H)
    vs, us = np.arange(top, bottom, stride), np.arange(left, right, stride)
    if len(vs) == 0 or len(us) == 0:
        return np.zeros((0, 3))
    vv, uu = np.meshgrid(vs, us, indexing="ij")
    dd = d[vv, uu].astype(np.float64)
    ok = (dd > 100) & (dd < 2000)
    z = dd[ok] / 1000.0 + float(behind_m)
    x = (uu[ok].astype(np.float64) - K[0, 2]) * z / K[0, 0]
    y = (vv[ok].astype(np.float64) - K[1, 2]) * z / K[1, 1]
    return np.stack([x, y, z], axis=1)
