"""The yardstick of the scene-aware pose grid tests (a helper module, as tests/pose_grid_oracle.py): the rule of
se3tn_score_pose_grid_scene stated in numpy float64, vectorised, in the operation order include/se3tracknet.h states -- so that every
counter of the library must EQUAL it -- and a plain per-point Python loop of the same rule (the vectorised form is checked against
it).  Candidate r * n_trans + t is the pose [R_r | t_t]; `scene` is the composed depth of the tracked objects, uint16 [H,W], 0 = none.

    q, c, facing, in front, uf, vf, in frame, m = rint(c.z * 1000.0)            exactly as tests/pose_grid_oracle.py
    s = scene[vf, uf]
    hidden     in frame and 100 < s < 2000 and s <= m + tol                      enters hidden_pts and nothing else past in_frame_pts
    otherwise  d = depth[vf, uf]; seen, inlier, front, behind                    exactly as tests/pose_grid_oracle.py
"""
import numpy as np

FIELDS = ("points", "in_frame_pts", "seen_pts", "inlier_pts", "front_pts", "behind_pts", "tol_mm", "hidden_pts")
DTYPE = np.dtype([(k, "<u4") for k in FIELDS])


def score(points, normals, rots, trans, depth, scene, K, tol_mm, facing, chunk=64):
    """n_rot * n_trans records (DTYPE); vectorised over translations and points per rotation, numpy float64 elementwise (no fused
    multiply-add); `chunk` translations at a time to bound the memory of a wide grid"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    x, y, z = (pts[:, i][None, :] for i in range(3))
    R = np.asarray(rots, np.float64).reshape(-1, 3, 3)
    T = np.asarray(trans, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(9)
    depth = np.asarray(depth)
    scene = np.asarray(scene)
    H, W = depth.shape
    assert scene.shape == depth.shape
    tol = float(tol_mm)
    if facing:
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        nx, ny, nz = (nrm[:, i][None, :] for i in range(3))
    out = np.zeros(len(R) * len(T), DTYPE)
    out["tol_mm"] = tol_mm
    with np.errstate(all="ignore"):
        for r, M in enumerate(R):
            q = [(M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z for a in range(3)]
            if facing:
                n = [(M[a, 0] * nx + M[a, 1] * ny) + M[a, 2] * nz for a in range(3)]
            for t0 in range(0, len(T), chunk):
                t = T[t0:t0 + chunk]
                cx, cy, cz = (q[a] + t[:, a][:, None] for a in range(3))
                if facing:
                    use = ((n[0] * cx + n[1] * cy) + n[2] * cz) < 0
                else:
                    use = np.ones(cx.shape, bool)
                front = cz > 0
                uf = np.rint(cx * K[0] / cz + K[2])
                vf = np.rint(cy * K[4] / cz + K[5])
                inf = use & front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
                u = np.where(inf, uf, 0.0).astype(np.int64)
                v = np.where(inf, vf, 0.0).astype(np.int64)
                m = np.rint(cz * 1000.0)
                s = scene[v, u].astype(np.float64)
                hidden = inf & (s > 100) & (s < 2000) & (s <= m + tol)
                d = depth[v, u].astype(np.float64)
                seen = inf & ~hidden & (d > 100) & (d < 2000)
                o = out[r * len(T) + t0:r * len(T) + t0 + len(t)]
                o["points"] = use.sum(1)
                o["in_frame_pts"] = inf.sum(1)
                o["hidden_pts"] = hidden.sum(1)
                o["seen_pts"] = seen.sum(1)
                o["inlier_pts"] = (seen & (np.abs(d - m) <= tol)).sum(1)
                o["front_pts"] = (seen & (d < m - tol)).sum(1)
                o["behind_pts"] = (seen & (d > m + tol)).sum(1)
    return out


def score_loop(points, normals, rots, trans, depth, scene, K, tol_mm, facing):
    """the same rule one point at a time in numpy float64 scalars: what score() is checked against"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3) if facing else np.zeros_like(pts)
    R = np.asarray(rots, np.float64).reshape(-1, 3, 3)
    T = np.asarray(trans, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(9)
    H, W = depth.shape
    tol = np.float64(tol_mm)
    out = np.zeros(len(R) * len(T), DTYPE)
    with np.errstate(all="ignore"):
        for r, M in enumerate(R):
            for ti, t in enumerate(T):
                cnt = dict.fromkeys(FIELDS, 0)
                cnt["tol_mm"] = tol_mm
                for (x, y, z), (nx, ny, nz) in zip(pts, nrm):
                    c = [((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + t[a] for a in range(3)]
                    if facing:
                        n = [(M[a, 0] * nx + M[a, 1] * ny) + M[a, 2] * nz for a in range(3)]
                        if not ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) < 0:
                            continue
                    cnt["points"] += 1
                    if not c[2] > 0:
                        continue
                    uf = np.rint(c[0] * K[0] / c[2] + K[2])
                    vf = np.rint(c[1] * K[4] / c[2] + K[5])
                    if not (uf >= 0 and uf < W and vf >= 0 and vf < H):
                        continue
                    cnt["in_frame_pts"] += 1
                    m = np.rint(c[2] * 1000.0)
                    s = np.float64(scene[int(vf), int(uf)])
                    if s > 100 and s < 2000 and s <= m + tol:
                        cnt["hidden_pts"] += 1
                        continue
                    d = np.float64(depth[int(vf), int(uf)])
                    if not (d > 100 and d < 2000):
                        continue
                    cnt["seen_pts"] += 1
                    cnt["inlier_pts"] += int(abs(d - m) <= tol)
                    cnt["front_pts"] += int(d < m - tol)
                    cnt["behind_pts"] += int(d > m + tol)
                out[r * len(T) + ti] = tuple(cnt[k] for k in FIELDS)
    return out


def rank(fit, k):
    """the k best indices in se3tn_rank_poses' order: more inliers, then fewer seen-through points, then the lower index"""
    order = np.lexsort((np.arange(len(fit)), fit["behind_pts"].astype(np.int64), -fit["inlier_pts"].astype(np.int64)))
    return order[:k].astype(np.int32)


def check_invariants(fit, P, tol_mm, facing):
    f = {k: fit[k].astype(np.int64) for k in FIELDS}
    assert (f["tol_mm"] == tol_mm).all()
    assert (f["points"] <= P).all() if facing else (f["points"] == P).all()
    assert (f["seen_pts"] == f["inlier_pts"] + f["front_pts"] + f["behind_pts"]).all()
    assert (f["hidden_pts"] + f["seen_pts"] <= f["in_frame_pts"]).all() and (f["in_frame_pts"] <= f["points"]).all()
