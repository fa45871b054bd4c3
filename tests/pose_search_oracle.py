"""The yardstick of the pose search tests (a helper module, as tests/route_model.py): the rule of se3tn_score_poses stated in numpy
float64, vectorised, in the operation order include/se3tracknet.h states -- so that every counter of the library must EQUAL it -- a
plain per-point Python loop of the same rule (the vectorised form is checked against it), the rank key, and the candidate lattice
recomputed independently of the package's pose_lattice.

    c = R x + t              row r: ((r_r0 x + r_r1 y) + r_r2 z) + t_r
    in front   c.z > 0
    uf = rint(c.x * K[0] / c.z + K[2]),  vf = rint(c.y * K[4] / c.z + K[5])        (np.rint: half to even)
    in frame   in front and 0 <= uf < W and 0 <= vf < H                            (on the doubles)
    d = depth[vf, uf],  m = rint(c.z * 1000.0)
    seen       in frame and 100 < d < 2000
    inlier |d - m| <= tol,  front d < m - tol,  behind d > m + tol                 (of the seen ones)
"""
import numpy as np

FIELDS = ("points", "in_frame_pts", "seen_pts", "inlier_pts", "front_pts", "behind_pts", "tol_mm", "_reserved")
DTYPE = np.dtype([(k, "<u4") for k in FIELDS])
FIELD_MAX = (1 << 20) - 1


def score(points, poses, depth, K, tol_mm):
    """n records (DTYPE) of n poses [n,4,4]; vectorised over poses and points, numpy float64 elementwise (no fused multiply-add)"""
    x, y, z = (np.asarray(points, np.float64).reshape(-1, 3)[:, i][None, :] for i in range(3))
    T = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    K = np.asarray(K, np.float64).reshape(9)
    depth = np.asarray(depth)
    H, W = depth.shape
    tol = float(tol_mm)
    r = lambda i, j: T[:, i, j][:, None]   # noqa: E731
    with np.errstate(all="ignore"):
        cx = ((r(0, 0) * x + r(0, 1) * y) + r(0, 2) * z) + r(0, 3)
        cy = ((r(1, 0) * x + r(1, 1) * y) + r(1, 2) * z) + r(1, 3)
        cz = ((r(2, 0) * x + r(2, 1) * y) + r(2, 2) * z) + r(2, 3)
        front = cz > 0
        uf = np.rint(cx * K[0] / cz + K[2])
        vf = np.rint(cy * K[4] / cz + K[5])
        inf = front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        u = np.where(inf, uf, 0.0).astype(np.int64)
        v = np.where(inf, vf, 0.0).astype(np.int64)
        d = depth[v, u].astype(np.float64)
        m = np.rint(cz * 1000.0)
        seen = inf & (d > 100) & (d < 2000)
        inl = seen & (np.abs(d - m) <= tol)
        fro = seen & (d < m - tol)
        beh = seen & (d > m + tol)
    out = np.zeros(len(T), DTYPE)
    out["points"] = x.shape[1]
    out["in_frame_pts"] = inf.sum(1)
    out["seen_pts"] = seen.sum(1)
    out["inlier_pts"] = inl.sum(1)
    out["front_pts"] = fro.sum(1)
    out["behind_pts"] = beh.sum(1)
    out["tol_mm"] = tol_mm
    return out


def score_loop(points, poses, depth, K, tol_mm):
    """the same rule one point at a time in numpy float64 scalars: what score() is checked against"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    K = np.asarray(K, np.float64).reshape(9)
    H, W = depth.shape
    tol = np.float64(tol_mm)
    out = np.zeros(len(T), DTYPE)
    with np.errstate(all="ignore"):
        for i, P in enumerate(T):
            cnt = dict.fromkeys(FIELDS, 0)
            for x, y, z in pts:
                c = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
                if not c[2] > 0:
                    continue
                uf = np.rint(c[0] * K[0] / c[2] + K[2])
                vf = np.rint(c[1] * K[4] / c[2] + K[5])
                if not (uf >= 0 and uf < W and vf >= 0 and vf < H):
                    continue
                cnt["in_frame_pts"] += 1
                d = np.float64(depth[int(vf), int(uf)])
                if not (d > 100 and d < 2000):
                    continue
                m = np.rint(c[2] * 1000.0)
                cnt["seen_pts"] += 1
                cnt["inlier_pts"] += int(abs(d - m) <= tol)
                cnt["front_pts"] += int(d < m - tol)
                cnt["behind_pts"] += int(d > m + tol)
            cnt["points"], cnt["tol_mm"] = len(pts), tol_mm
            out[i] = tuple(cnt[k] for k in FIELDS)
    return out


def key(inlier, behind, index):
    """inlier * 2^40 + (2^20 - 1 - min(behind, 2^20 - 1)) * 2^20 + (2^20 - 1 - index), a Python int"""
    return int(inlier) * (1 << 40) + (FIELD_MAX - min(int(behind), FIELD_MAX)) * (1 << 20) + (FIELD_MAX - int(index))


def keys(fit):
    return [key(f["inlier_pts"], f["behind_pts"], i) for i, f in enumerate(fit)]


def rank(fit, k):
    """indices of the k best records, best first: a sort by the TUPLE (inliers descending, behind (clamped) ascending, index
    ascending) -- not by the key, which the plan check holds to this order"""
    order = sorted(range(len(fit)), key=lambda i: (-int(fit["inlier_pts"][i]), min(int(fit["behind_pts"][i]), FIELD_MAX), i))
    return np.array(order[:k], np.int32)


def check_invariants(fit, P, tol_mm):
    f = {k: fit[k].astype(np.int64) for k in FIELDS}
    assert (f["points"] == P).all() and (f["tol_mm"] == tol_mm).all() and (f["_reserved"] == 0).all()
    assert (f["seen_pts"] == f["inlier_pts"] + f["front_pts"] + f["behind_pts"]).all()
    assert (f["seen_pts"] <= f["in_frame_pts"]).all() and (f["in_frame_pts"] <= f["points"]).all()


def axis_rotation(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    R = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def lattice(base, radius_steps, step, rot_deg):
    """the candidates in the order the issue fixes: rotations outermost (identity, then +a, -a about camera x, y, z per angle),
    translations x outermost .. z innermost ascending; R = dR . R_base, t = t_base + dt"""
    base = np.asarray(base, np.float64)
    rots = [np.eye(3)]
    for a in rot_deg:
        for ax in range(3):
            rots += [axis_rotation(ax, a), axis_rotation(ax, -a)]
    out = []
    rng = range(-radius_steps, radius_steps + 1)
    for dR in rots:
        for ix in rng:
            for iy in rng:
                for iz in rng:
                    T = np.eye(4)
                    T[:3, :3] = dR @ base[:3, :3]
                    T[:3, 3] = base[:3, 3] + np.array([ix * step, iy * step, iz * step])
                    out.append(T)
    return np.array(out)
