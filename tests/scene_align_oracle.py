"""The yardstick of the scene-aware pose alignment tests (a helper module, as tests/pose_align_oracle.py, whose walk, solves and Cayley
update it reuses): the rule of se3tn_align_poses_scene stated in numpy float64 in the operation order include/se3tracknet.h states --
vectorised over the points of a pose (align) and as a plain per-point loop on Python floats (align_loop).  The rule of
se3tn_align_poses with ONE step more, for a FACING point whose pixel is in frame, before d is looked at:

    s = scene[vf, uf],  m = rint(c.z * 1000.0)
    hidden   100 < s < 2000 and s <= m + scene_tol_mm      on doubles: the predicate of tests/scene_search_oracle.py
             a hidden point enters hidden_pts and nothing else past facing_pts: it is not paired whatever d is, it adds to no sum
    otherwise  d, seen, paired, o, r, J, fx exactly as tests/pose_align_oracle.py

Every sum is an integer, so the two, the stand-alone host program (tests/c_abi/pose_align_scene_check.cpp) and the device must agree
WORD FOR WORD.  The record is REC_DTYPE: pose_align_oracle.REC_DTYPE with hidden_pts, the hidden points at the last evaluated pose, in
the place of _reserved."""
import numpy as np

import pose_align_oracle as PAO

ITERS, CONVERGED, FEW, SINGULAR, SUMS = PAO.ITERS, PAO.CONVERGED, PAO.FEW, PAO.SINGULAR, PAO.SUMS
REC_DTYPE = np.dtype([(k if k != "_reserved" else "hidden_pts", PAO.REC_DTYPE.fields[k][0]) for k in PAO.REC_DTYPE.names])
assert REC_DTYPE.itemsize == 40 and REC_DTYPE.fields["hidden_pts"][1] == 28


def sums_of_scene(pts, nrm, R, t, depth, scene, K, gate_mm, scene_tol_mm):
    """(sums int64 [28], pairs, facing points, hidden points) of one pose, vectorised over the points"""
    K = np.asarray(K, np.float64).reshape(9)
    H, W = depth.shape
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    with np.errstate(all="ignore"):
        q = [(R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z for a in range(3)]
        c = [q[a] + t[a] for a in range(3)]
        n = [(R[a, 0] * nx + R[a, 1] * ny) + R[a, 2] * nz for a in range(3)]
        facing = ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) < 0
        uf = np.rint(c[0] * K[0] / c[2] + K[2])
        vf = np.rint(c[1] * K[4] / c[2] + K[5])
        inf = facing & (c[2] > 0) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        u = np.where(inf, uf, 0.0).astype(np.int64)
        v = np.where(inf, vf, 0.0).astype(np.int64)
        d = depth[v, u].astype(np.float64)
        s = scene[v, u].astype(np.float64)
        m = np.rint(c[2] * 1000.0)
        hidden = inf & (s > 100) & (s < 2000) & (s <= m + float(scene_tol_mm))
        paired = inf & ~hidden & (d > 100) & (d < 2000) & (np.abs(d - m) <= float(gate_mm))
        k = np.nonzero(paired)[0]
        q, c, n, uf, vf, d = [a[k] for a in q], [a[k] for a in c], [a[k] for a in n], uf[k], vf[k], d[k]
        oz = d / 1000.0
        ox = ((uf - K[2]) * oz) / K[0]
        oy = ((vf - K[5]) * oz) / K[4]
        r = (n[0] * (ox - c[0]) + n[1] * (oy - c[1])) + n[2] * (oz - c[2])
        J = np.stack([q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]])
        S = np.empty(SUMS, np.int64)
        S[:21] = PAO.fx(J[PAO._PI] * J[PAO._PJ]).sum(1)
        S[21:27] = PAO.fx(J * r).sum(1)
        S[27] = PAO.fx(r * r).sum()
    return S, len(k), int(facing.sum()), int(hidden.sum())


def sums_of_scene_loop(pts, nrm, R, t, depth, scene, K, gate_mm, scene_tol_mm):
    """the same one point at a time on Python floats and ints"""
    K = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    H, W = depth.shape
    R = [[float(R[a, b]) for b in range(3)] for a in range(3)]
    t = [float(v) for v in t]
    S, pairs, facing, hidden = [0] * SUMS, 0, 0, 0

    def fx1(v):
        v = -256.0 if not v >= -256.0 else v             # fmax(v, -256): a NaN gives -256
        v = 256.0 if v > 256.0 else v
        return int(np.rint(v * PAO.TWO32))

    with np.errstate(all="ignore"):
        for (x, y, z), (nx, ny, nz) in zip(pts.tolist(), nrm.tolist()):
            q = [(R[a][0] * x + R[a][1] * y) + R[a][2] * z for a in range(3)]
            c = [q[a] + t[a] for a in range(3)]
            n = [(R[a][0] * nx + R[a][1] * ny) + R[a][2] * nz for a in range(3)]
            if not ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) < 0:
                continue
            facing += 1
            if not c[2] > 0:
                continue
            uf = float(np.rint(np.float64(c[0]) * K[0] / np.float64(c[2]) + K[2]))
            vf = float(np.rint(np.float64(c[1]) * K[4] / np.float64(c[2]) + K[5]))
            if not (uf >= 0 and uf < W and vf >= 0 and vf < H):
                continue
            m = float(np.rint(c[2] * 1000.0))
            s = float(scene[int(vf), int(uf)])
            if s > 100 and s < 2000 and s <= m + float(scene_tol_mm):
                hidden += 1
                continue
            d = float(depth[int(vf), int(uf)])
            if not (d > 100 and d < 2000 and abs(d - m) <= float(gate_mm)):
                continue
            pairs += 1
            oz = d / 1000.0
            ox = ((uf - K[2]) * oz) / K[0]
            oy = ((vf - K[5]) * oz) / K[4]
            r = (n[0] * (ox - c[0]) + n[1] * (oy - c[1])) + n[2] * (oz - c[2])
            J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]]
            for w, (i, j) in enumerate(PAO.PAIRS):
                S[w] += fx1(J[i] * J[j])
            for i in range(6):
                S[21 + i] += fx1(J[i] * r)
            S[27] += fx1(r * r)
    return np.array(S, np.int64), pairs, facing, hidden


def _align(points, normals, poses, depth, scene, K, scene_tol_mm, gate_mm, iters, min_pairs, damping, stop, sums_fn, solve_fn):
    """pose_align_oracle._align pose by pose (a pose's output does not depend on the others) with the scene rule's sums; the hidden
    count of a pose's LAST evaluation -- the one its record describes -- goes into the record's word at offset 28"""
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    scene = np.asarray(scene)
    assert scene.shape == np.asarray(depth).shape
    out, rec, sums = P.copy(), np.zeros(len(P), REC_DTYPE), np.zeros((len(P), SUMS), np.int64)
    for p in range(len(P)):
        last = []

        def fn(pts, nrm, R, t, dep, k, gate):
            S, pairs, facing, hidden = sums_fn(pts, nrm, R, t, dep, scene, k, gate, scene_tol_mm)
            last[:] = [hidden]
            return S, pairs, facing

        o, r, s = PAO._align(points, normals, P[p:p + 1], depth, K, gate_mm, [iters], min_pairs, damping, stop, fn, solve_fn)[int(iters)]
        out[p], sums[p] = o[0], s[0]
        rec[p] = r.view(REC_DTYPE)[0]
        rec["hidden_pts"][p] = last[0]
    return out, rec, sums


def align(points, normals, poses, depth, scene, K, scene_tol_mm=10, gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6):
    """-> (poses [n,4,4], records [n] REC_DTYPE, sums int64 [n,28]), vectorised over the points, the solve on Python floats"""
    return _align(points, normals, poses, depth, scene, K, scene_tol_mm, gate_mm, iters, min_pairs, damping, stop, sums_of_scene,
                  PAO.solve_floats)


def align_loop(points, normals, poses, depth, scene, K, scene_tol_mm=10, gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6):
    """the same rule one point at a time on Python floats, the solve on numpy scalars: what align() is checked against"""
    return _align(points, normals, poses, depth, scene, K, scene_tol_mm, gate_mm, iters, min_pairs, damping, stop, sums_of_scene_loop,
                  PAO.solve_arrays)


def hidden_of(rec):
    """hidden_pts per pose"""
    return np.asarray(rec["hidden_pts"])
