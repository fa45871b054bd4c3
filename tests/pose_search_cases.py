"""The small cases of the pose search and pose grid tests (a helper module, numpy only), shared by tests/test_gpu_pose_search.py,
tests/test_gpu_pose_grid.py and tests/test_pose_point_rule_host.py so that the device and the host program see the same inputs:
  boundary_*()    identity rotation, points at z = 1 and K = [[1, 0, 0.5], [0, 1, 1.5]]: u = x + 0.5 and v = y + 1.5 are exact, so
                  points sit ON the frame's edges; the frame's pixels cycle through the values around every threshold;
  blob(P)         P points in a 90 mm ball with the normals of a convex blob, grid_depth() the 48 x 64 frame around 500 mm with holes
                  and borderline values, grid_factors() 3 rotations and 53 translations around (0, 0, 0.5);
  write_case() / read_records()   the files tests/c_abi/pose_point_rule_check.cpp reads and writes.
"""
import struct

import numpy as np
from scipy.spatial.transform import Rotation

import pose_search_oracle as PSO

BOUNDARY_K = np.array([[1.0, 0, 0.5], [0, 1.0, 1.5], [0, 0, 1.0]])
GRID_HW = (48, 64)
GRID_K = np.array([[100.0, 0, 31.5], [0, 101.0, 23.5], [0, 0, 1.0]])
GRID_TT = 16                               # csrc/pose_grid_plan.h PG_TT: translations per workgroup


def boundary_points(hw):
    """points ON -0.5 (rounds to -0.0: inside), 0.5 (to 0), W - 1.5 and W - 0.5 (to W for even W: outside; to W - 1 for odd W), the
    same for v, and two points far beyond any integer"""
    Hh, Ww = hw
    xs = [-1.0, 0.0, Ww - 2.0, Ww - 1.0]
    ys = [-2.0, -1.0, Hh - 3.0, Hh - 2.0]
    return np.array([(x, y, 1.0) for x in xs for y in ys] + [(1e18, 0.0, 1.0), (0.0, -1e300, 1.0)])


def boundary_poses():
    """the identity (m = 1000 exactly), half a millimetre further, behind the camera"""
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[1, 2, 3] = 0.0005     # c.z * 1000 = 1000.5: m rounds half to even
    poses[2, 2, 3] = -2.0       # behind the camera
    return poses


def boundary_values(tol):
    """0, 100, 101, 1999, 2000, 65535 and 1000 -+ (tol - 1, tol, tol + 1) where a uint16 holds them"""
    vals = [0, 100, 101, 1999, 2000, 65535] + [1000 + s * (tol + e) for s in (-1, 1) for e in (-1, 0, 1)]
    return np.array([v for v in vals if 0 <= v <= 65535], np.uint16)


def boundary_depth(hw, vals, shift):
    """the frame whose pixels cycle through vals, shifted `shift` places: over all shifts every pixel takes every value"""
    Hh, Ww = hw
    return vals[(np.arange(Hh * Ww) + shift) % len(vals)].reshape(Hh, Ww)


def blob(P):
    """P points in a 90 mm ball and their normals: the direction from the centre (a convex blob: about half of it faces the camera)"""
    rng = np.random.default_rng(P)
    pts = rng.normal(size=(P, 3))
    pts *= (0.045 * rng.uniform(0.3, 1.0, P) / np.linalg.norm(pts, axis=1))[:, None]
    return np.ascontiguousarray(pts), np.ascontiguousarray(pts / np.linalg.norm(pts, axis=1)[:, None])


def grid_depth():
    H, W = GRID_HW
    rng = np.random.default_rng(48)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (500 + 0.6 * (xx - W / 2) - 0.4 * (yy - H / 2) + 12 * np.sin(xx / 5.0)).astype(np.uint16)
    mask = rng.random((H, W)) < 0.1
    d[mask] = rng.choice(np.array([0, 100, 101, 1999, 2000, 65535], np.uint16), int(mask.sum()))
    return np.ascontiguousarray(d)


def grid_factors():
    """3 rotations and 53 translations: prefixes of these are the grids of the tiling tests.  Translation 7 is behind the camera,
    translation 11 far off the frame"""
    rng = np.random.default_rng(5)
    rots = Rotation.from_rotvec(rng.normal(size=(3, 3))).as_matrix()
    trans = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, (3 * GRID_TT + 5, 3))
    trans[7] = (0.0, 0.0, -0.5)
    trans[11] = (2.0, 0.0, 0.5)
    return np.ascontiguousarray(rots), np.ascontiguousarray(trans)


def write_case(path, pts, nrm, poses, rots, trans, frames, K, tol_mm, facing):
    """the binary case file tests/c_abi/pose_point_rule_check.cpp reads; frames [F,H,W]; nrm may be None when facing is 0"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    nrm = np.zeros_like(pts) if nrm is None else np.ascontiguousarray(nrm, np.float64).reshape(-1, 3)
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    rots = np.ascontiguousarray(np.asarray(rots, np.float64).reshape(-1, 9))
    trans = np.ascontiguousarray(np.asarray(trans, np.float64).reshape(-1, 3))
    frames = np.ascontiguousarray(frames, np.uint16)
    F, H, W = frames.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<10i", 0x5052, len(pts), len(poses), len(rots), len(trans), F, H, W, tol_mm, int(facing)))
        for a in (np.asarray(K, np.float64).reshape(9), pts, nrm, poses, rots, trans):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(frames.tobytes())


def read_records(path, frames, n_poses, n_candidates):
    """per frame (records of the poses, records of the lattice candidates) as the program wrote them"""
    raw = np.fromfile(path, PSO.DTYPE)
    assert len(raw) == frames * (n_poses + n_candidates), len(raw)
    raw = raw.reshape(frames, n_poses + n_candidates)
    return [(r[:n_poses], r[n_poses:]) for r in raw]
