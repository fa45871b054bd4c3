"""The scenes of the scene-aware alignment tests (a helper module: numpy and the oracles, no device), shared by
tests/test_scene_align_host.py and tests/test_gpu_scene_align.py so that each reference is computed once.

  the stacked scene   a tracked slab S lies ON the lost slab L of tests/scene_search_scene.py: its near face is 20 mm in front of
                      L's, inside the default gate, turned by 30 degrees about the table's normal, and it covers a good third of L.
                      Plain alignment pairs L's covered points with S's face and tilts L up; under the scene rule they are hidden.
                      perturbed(40): 40 seeded perturbations of L's true pose, up to 8 degrees and 8 mm per axis.
  the existing scene  scene_search_scene's T, L, O with the place L was last seen moved OFF the lattice: `last` + (4, -3, 5) mm,
                      with or without a further turn of 5 degrees about the camera's z axis.  pool(...) walks
                      MultiTracker.recover(align=20, refine=0) on the oracles: the scene-aware facing search, the top 8 nodes,
                      their alignment under either rule, the pool [aligned, unrefined] rescored under the scene rule.

The bound is that of tests/pose_align_cases.py: one pixel's footprint at 0.5 m plus the 1 mm depth quantum, 2.9 mm, and that length
over the slab's 90 mm, 1.85 degrees."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import color_fit_scene as CS
import pose_align_cases as PAC
import pose_align_oracle as PAO
import scene_align_oracle as SAO
import scene_fit_scene as SF
import scene_search_oracle as SSO
import scene_search_scene as SS

K, TOL = SS.K, SS.TOL
BOUND_M = PAC.BOUND_M
BOUND_DEG = float(np.degrees(BOUND_M / 0.090))
DEFAULTS = PAC.DEFAULTS
LAST_SHIFT = np.array([0.004, -0.003, 0.005])
LAST_TURN_DEG = 5.0


# ---- the stacked scene -------------------------------------------------------------------------------------------------------------------
def stacked_poses():
    """dict L, S -> 4x4 poses"""
    L = SS._on_table((0.0, 0.0, 0.0))
    S = SS._on_table((0.030, 0.020, 2 * CS.HALF))
    S[:3, :3] = S[:3, :3] @ Rotation.from_euler("z", 30.0, degrees=True).as_matrix()
    return dict(L=L, S=S)


@functools.lru_cache(maxsize=None)
def stacked_renders():
    P = stacked_poses()
    return dict(table=SF.oracle_depth(SS.table_mesh(), SS.table_pose()), L=SF.oracle_depth(SS.slab_mesh(), P["L"]),
                S=SF.oracle_depth(SS.slab_mesh(), P["S"]))


def stacked_frame(seed=0):
    """the observed depth, uint16 [H,W] mm"""
    r = stacked_renders()
    return SF.observe(SS.compose([r["table"], r["L"], r["S"]]), seed)


def stacked_scene():
    """the composed depth of the tracked slab S, uint16 [H,W] mm, 0 elsewhere"""
    return SS.compose([stacked_renders()["S"]])


def stacked_covered_share():
    """the share of L's rendered pixels at which S is nearer"""
    r = stacked_renders()
    on = r["L"] > 0
    return float(((r["S"] > 0) & (r["S"] < r["L"]) & on).sum()) / float(on.sum())


def perturbed(count=40, seed=1):
    """for each trial, in this order: axis = normal(3) normalised, angle = uniform(0, 8) degrees applied on the left,
    translation += uniform(-0.008, 0.008, 3)"""
    rng = np.random.default_rng(seed)
    G = stacked_poses()["L"]
    out = []
    for _ in range(count):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(0, 8)
        T = G.copy()
        T[:3, :3] = Rotation.from_rotvec(np.deg2rad(angle) * axis).as_matrix() @ G[:3, :3]
        T[:3, 3] += rng.uniform(-0.008, 0.008, 3)
        out.append(T)
    return np.array(out)


def within(poses, truth):
    """(bool [n]: inside the bound, errors [n,2] in metres / degrees)"""
    errs = np.array([PAO.pose_error(o, truth) for o in poses])
    return (errs[:, 0] <= BOUND_M) & (errs[:, 1] <= BOUND_DEG), errs


@functools.lru_cache(maxsize=None)
def stacked_aligned(seed=0):
    """dict plain, scene -> (poses, records, sums) of the 40 perturbations on the oracles, computed once per observation seed"""
    pts, nrm = SS.slab_model()
    depth, poses = stacked_frame(seed), perturbed(40)
    return dict(plain=PAO.align(pts, nrm, poses, depth, K, **DEFAULTS),
                scene=SAO.align(pts, nrm, poses, depth, stacked_scene(), K, TOL, **DEFAULTS))


# ---- the existing scene, off the lattice ---------------------------------------------------------------------------------------------------
def off_node_last(turn=True):
    """where L was last seen, moved off the lattice: + LAST_SHIFT, and with `turn` a rotation of LAST_TURN_DEG about the camera's z
    axis applied on the left of its rotation"""
    last = SS.poses()["last"].copy()
    last[:3, 3] += LAST_SHIFT
    if turn:
        last[:3, :3] = Rotation.from_euler("z", LAST_TURN_DEG, degrees=True).as_matrix() @ last[:3, :3]
    return last


def diagonal_fit(pts, nrm, poses, depth, scene, tol):
    """the scene-aware facing records of m poses (the diagonal of the m x m grid of their factors)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    m = len(poses)
    return SSO.score(pts, nrm, poses[:, :3, :3], poses[:, :3, 3], depth, scene, K, tol, 1)[np.arange(m) * (m + 1)]


def pool_from(pts, nrm, unrefined, aligned, depth, scene, tol=TOL):
    """step (4) of MultiTracker.recover(refine=0): the pool [aligned, unrefined] rescored under the scene rule -> (pool, records,
    chosen): the largest key wins, ties prefer the lower index"""
    import se3tracknet_amd as se3
    final = np.concatenate([aligned, unrefined])
    fit = diagonal_fit(pts, nrm, final, depth, scene, tol)
    return final, fit, int(np.argmax(se3.recover.pose_key(fit)))


@functools.lru_cache(maxsize=None)
def pool(turn=True, scene_rule=True, top=8, iters=20):
    """MultiTracker.recover(align=iters, refine=0[, scene_align=scene_rule]) around off_node_last(turn), on the oracles alone ->
    dict(unrefined, top_idx, top_fit, aligned, align_rec, final, final_fit, chosen, pose)"""
    import se3tracknet_amd as se3
    pts, nrm = SS.slab_model()
    depth, scene = SS.frame(0), SS.scene()
    rots, trans = se3.recover.lattice_factors(off_node_last(turn), 0.05, SS.TRANS_STEP, (15.0,))
    fit = SSO.score(pts, nrm, rots, trans, depth, scene, K, TOL, 1)
    idx = SSO.rank(fit, top)
    unrefined = np.tile(np.eye(4), (len(idx), 1, 1))
    unrefined[:, :3, :3], unrefined[:, :3, 3] = rots[idx // len(trans)], trans[idx % len(trans)]
    prm = dict(DEFAULTS, iters=iters)
    if scene_rule:
        aligned, rec, _ = SAO.align(pts, nrm, unrefined, depth, scene, K, TOL, **prm)
    else:
        aligned, rec, _ = PAO.align(pts, nrm, unrefined, depth, K, **prm)
    final, final_fit, chosen = pool_from(pts, nrm, unrefined, aligned, depth, scene)
    return dict(unrefined=unrefined, top_idx=idx, top_fit=fit[idx], aligned=aligned, align_rec=rec, final=final, final_fit=final_fit,
                chosen=chosen, pose=final[chosen])


# ---- the case files of tests/c_abi/pose_align_scene_check.cpp ------------------------------------------------------------------------------
def write_case(path, pts, nrm, poses, depth, scene, K, scene_tol_mm, gate_mm, iters, min_pairs, damping, stop):
    """int32 {magic 0x5053, P, n, H, W, gate_mm, iters, min_pairs, scene_tol_mm}, float64 {damping, stop, K[9]}, float64 points [P,3],
    normals [P,3], poses [n,16], uint16 depth [H,W], uint16 scene [H,W]"""
    import struct
    poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    H, W = depth.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", 0x5053, len(pts), len(poses), H, W, gate_mm, iters, min_pairs, scene_tol_mm))
        f.write(np.array([damping, stop, *np.asarray(K, np.float64).reshape(9)], np.float64).tobytes())
        for a in (pts, nrm, poses):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(np.ascontiguousarray(depth, np.uint16).tobytes())
        f.write(np.ascontiguousarray(scene, np.uint16).tobytes())


def read_result(path, n):
    """(poses [n,4,4], records [n], sums [n,28]) as the program wrote them"""
    raw = open(path, "rb").read()
    assert len(raw) == n * (128 + 40 + 224), len(raw)
    poses = np.frombuffer(raw, np.float64, n * 16).reshape(n, 4, 4)
    rec = np.frombuffer(raw, SAO.REC_DTYPE, n, offset=n * 128)
    sums = np.frombuffer(raw, np.int64, n * 28, offset=n * 168).reshape(n, 28)
    return poses, rec, sums


# ---- the small device case -----------------------------------------------------------------------------------------------------------------
def device_poses(case):
    """the poses composed from SS.device_case()'s rotations and translations: every rotation with translations 0, 1, 2 and 3 (behind
    the camera) -- 12 poses, the NaN rotation's among them; pose 0 is (rotation 0, translation 0), the candidate
    SS.boundary_scene marks"""
    _, _, rots, trans, _, _ = case
    out = []
    for r in rots:
        for t in trans[:4]:
            G = np.eye(4)
            G[:3, :3], G[:3, 3] = r, t
            out.append(G)
    return np.array(out)
