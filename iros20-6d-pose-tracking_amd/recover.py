"""Re-acquiring a lost object: the candidate poses ``Tracker.recover`` searches and the order it ranks them in.

The reference re-initialises a lost track from an external detector (PoseCNN at the frames ``--reinit_frames`` lists,
predict.py:539-541).  Without one, the search is local: a lattice of poses around the last pose the track had, every candidate
scored against the observed depth frame on the device (``Engine.score_poses`` -> se3tn_score_poses / se3tn_rank_poses), the best few
pulled in by the network (``Tracker.on_track_batch``) and scored once more.
"""
import numpy as np

KEY_FIELD_MAX = (1 << 20) - 1   # as csrc/pose_search_plan.h: the two 20-bit fields of a key


def pose_key(fit, index=None):
    """The 64-bit key se3tn_rank_poses orders records by (csrc/pose_search_plan.h ps_key), as Python ints in an object array:
    inlier_pts * 2^40 + (2^20 - 1 - min(behind_pts, 2^20 - 1)) * 2^20 + (2^20 - 1 - index); index defaults to the record's place.
    More inliers first, then fewer seen-through points, then the lower index."""
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
    m = len(dts)
    out = np.tile(np.eye(4), (len(rots) * m, 1, 1))
    for q, dR in enumerate(rots):
        out[q * m:(q + 1) * m, :3, :3] = dR @ base[:3, :3]
        out[q * m:(q + 1) * m, :3, 3] = base[:3, 3] + dts
    return out
