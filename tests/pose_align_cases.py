"""The cases of the pose alignment tests (a helper module, numpy only), shared by tests/test_pose_align_host.py and
tests/test_gpu_pose_align.py so that each reference is computed once:
  l_case()        the L of tests/pose_grid_scene.py on its 120 x 160 frame: a perturbed pose that aligns, one behind the camera, one with
                  a NaN, one off the frame, a second perturbed pose; points 7 and 8 carry a zero normal;
  plane_case()    a frontal plane: 15 x 15 points on z = 0 with the normal (0, 0, -1), seen at 500 mm on a 48 x 64 frame; pose 0 is exactly
                  frontal (damping 0: the in-plane directions have an exactly zero pivot), pose 1 tilted by 3 degrees and 4 mm off;
  perturbed(40)   the 40 seeded perturbations of the true pose;
  acquire_chain() stage 1, the local lattice and the alignment of Tracker.acquire(views=40, inplane=6, stride=8) on the oracle alone.
"""
import functools
import struct

import numpy as np
from scipy.spatial.transform import Rotation

import pose_align_oracle as PAO
import pose_grid_oracle as PGO
import pose_grid_scene as SC
import pose_search_oracle as PSO

BOUND_M = 0.5 / 266.7 + 0.001          # one pixel's footprint at 0.5 m plus the 1 mm depth quantum: 2.9 mm
BOUND_DEG = float(np.degrees(BOUND_M / 0.120))     # that length over the L's 120 mm: 1.4 degrees
DEFAULTS = dict(gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6)


def perturbed(count=40, seed=1):
    """for each trial, in this order: axis = normal(3) normalised, angle = uniform(0, 12) degrees applied on the left,
    translation += uniform(-0.012, 0.012, 3)"""
    rng = np.random.default_rng(seed)
    G = SC.true_pose()
    out = []
    for _ in range(count):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(0, 12)
        T = G.copy()
        T[:3, :3] = Rotation.from_rotvec(np.deg2rad(angle) * axis).as_matrix() @ G[:3, :3]
        T[:3, 3] += rng.uniform(-0.012, 0.012, 3)
        out.append(T)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def l_scene():
    pts, nrm = SC.l_model()
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm), SC.frame(0)


def bad_poses():
    """behind the camera, a NaN, off the frame"""
    G = SC.true_pose()
    behind, nan, off = G.copy(), G.copy(), G.copy()
    behind[2, 3] = -0.5
    nan[1, 1] = np.nan
    off[0, 3] = 2.0
    return behind, nan, off


def l_case():
    """(points, normals, poses [5,4,4], depth, K)"""
    pts, nrm, depth = l_scene()
    nrm = nrm.copy()
    nrm[7:9] = 0.0                                          # a zero normal never faces (two points of the upper face)
    two = perturbed(2, seed=11)
    poses = np.array([two[0], *bad_poses(), two[1]])
    poses[0, 3] = (5.0, 6.0, 7.0, 8.0)                      # row 3 of an input is not read
    return pts, nrm, poses, depth, SC.K


def plane_case():
    """(points, normals, poses [2,4,4], depth, K)"""
    g = (np.arange(15) - 7) * 0.005
    gx, gy = np.meshgrid(g, g, indexing="ij")
    pts = np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1))
    nrm = np.tile([0.0, 0.0, -1.0], (len(pts), 1))
    depth = np.full((48, 64), 500, np.uint16)
    K = np.array([[200.0, 0, 31.5], [0, 200.0, 23.5], [0, 0, 1.0]])
    frontal = np.eye(4)
    frontal[:3, 3] = (0.001, -0.002, 0.504)
    tilted = np.eye(4)
    tilted[:3, :3] = Rotation.from_euler("xy", (3.0, -2.0), degrees=True).as_matrix()
    tilted[:3, 3] = (0.001, -0.002, 0.504)
    return pts, nrm, np.array([frontal, tilted]), depth, K


def write_case(path, pts, nrm, poses, depth, K, gate_mm, iters, min_pairs, damping, stop):
    """the binary case file tests/c_abi/pose_align_check.cpp reads"""
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    H, W = depth.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", 0x5041, len(pts), len(poses), H, W, gate_mm, iters, min_pairs))
        f.write(np.array([damping, stop, *np.asarray(K, np.float64).reshape(9)], np.float64).tobytes())
        for a in (pts, nrm, poses):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(np.ascontiguousarray(depth, np.uint16).tobytes())


def read_result(path, n):
    """(poses [n,4,4], records [n], sums [n,28]) as the program wrote them"""
    raw = open(path, "rb").read()
    assert len(raw) == n * (128 + 40 + 224), len(raw)
    poses = np.frombuffer(raw, np.float64, n * 16).reshape(n, 4, 4)
    rec = np.frombuffer(raw, PAO.REC_DTYPE, n, offset=n * 128)
    sums = np.frombuffer(raw, np.int64, n * 28, offset=n * 168).reshape(n, 28)
    return poses, rec, sums


def facing_fit(pts, nrm, poses, depth, K, tol_mm):
    """the facing records of m poses (the diagonal of the m x m grid of their factors)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    m = len(poses)
    return PGO.score(pts, nrm, poses[:, :3, :3], poses[:, :3, 3], depth, K, tol_mm, 1)[np.arange(m) * (m + 1)]


def local_stage(pts, nrm, hyps, depth, K, tol_mm, lattice_factors):
    """step 2 of Tracker.acquire on the oracle: the best candidate of each hypothesis's own lattice -> (poses, records)"""
    local, fit = [], []
    for h in hyps:
        lr, lt = lattice_factors(h)
        w = PGO.score(pts, nrm, lr, lt, depth, K, tol_mm, 1)
        b = int(PSO.rank(w, 1)[0])
        local.append(PGO.compose(lr, lt)[b])
        fit.append(w[b])
    return np.array(local), np.array(fit, PSO.DTYPE)


@functools.lru_cache(maxsize=None)
def acquire_chain(top=8):
    """rotation_grid(40, 6) x depth_seeds(stride 8), top `top`, the local lattice, alignment -- all on the oracle ->
    dict(local, local_fit, aligned, align_rec, aligned_fit)"""
    import se3tracknet_amd as se3
    pts, nrm, depth = l_scene()
    rots, seeds = se3.recover.rotation_grid(40, 6), se3.recover.depth_seeds(depth, SC.K, 8, 0.03)
    stage1 = PGO.score(pts, nrm, rots, seeds, depth, SC.K, SC.TOL, 1)
    hyps = PGO.compose(rots, seeds)[PSO.rank(stage1, top)]
    local, local_fit = local_stage(pts, nrm, hyps, depth, SC.K, SC.TOL, se3.recover.lattice_factors)
    aligned, rec, _ = PAO.align(pts, nrm, local, depth, SC.K, **DEFAULTS)
    return dict(local=local, local_fit=local_fit, aligned=aligned, align_rec=rec,
                aligned_fit=facing_fit(pts, nrm, aligned, depth, SC.K, SC.TOL))
