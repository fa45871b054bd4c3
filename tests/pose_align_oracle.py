"""The yardstick of the pose alignment tests (a helper module, as tests/pose_grid_oracle.py): the rule of se3tn_align_poses stated in
numpy float64 in the operation order include/se3tracknet.h states -- vectorised over the points of a pose (align) and as a plain
per-point loop on Python floats (align_loop), each with a scalar LDL^T of its own.  Every sum is an integer (each term is quantised to 2^-32 before it
is added), so the two, the stand-alone host program (tests/c_abi/pose_align_check.cpp) and the device must agree WORD FOR WORD.

    q  = (R0 x + R1 y) + R2 z  per row,   c = q + t,   n' = (R0 nx + R1 ny) + R2 nz  per row
    f  = (n'x c.x + n'y c.y) + n'z c.z,   facing: f < 0
    in front, uf, vf, in frame, d, m, seen     as tests/pose_grid_oracle.py
    paired   seen and |d - m| <= gate
    o.z = d / 1000.0,  o.x = ((uf - K[2]) * o.z) / K[0],  o.y = ((vf - K[5]) * o.z) / K[4]
    r  = (n'x (o.x - c.x) + n'y (o.y - c.y)) + n'z (o.z - c.z)
    J  = (q x n', n')
    fx(v) = int64(rint(fmin(fmax(v, -256.0), 256.0) * 2^32))        (fmax / fmin: a NaN gives -256)
    sums: 21 x fx(J_i J_j) (i <= j, row-major) | 6 x fx(J_i r) | fx(r r);  counts: pairs, facing points
    pairs < min_pairs: FEW.  A = S_A 2^-32 (+ damping * pairs on the diagonal), b = S_b 2^-32, LDL^T without pivoting, every inner sum
    left to right from 0.0 over ascending k; a pivot that is not > 0 or a step that is not finite: SINGULAR, the pose unchanged.
    Cayley update about the object's origin: a = 0.5 w, R <- C R, t <- t + v.  max |delta| <= stop: CONVERGED (after the update).
"""
import numpy as np

ITERS, CONVERGED, FEW, SINGULAR = 0, 1, 2, 3
SUMS = 28
REC_DTYPE = np.dtype([("iterations", "<u4"), ("status", "<u4"), ("pairs", "<u4"), ("facing_pts", "<u4"), ("sum_r2", "<i8"),
                      ("pairs0", "<u4"), ("_reserved", "<u4"), ("sum_r2_0", "<i8")])
assert REC_DTYPE.itemsize == 40
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 words of S_A, row-major
TWO32 = 4294967296.0
_PI, _PJ = np.array([i for i, _ in PAIRS]), np.array([j for _, j in PAIRS])


def fx(v):
    return np.rint(np.fmin(np.fmax(v, -256.0), 256.0) * TWO32).astype(np.int64)


def sums_of(pts, nrm, R, t, depth, K, gate_mm):
    """(sums int64 [28], pairs, facing points) of one pose, vectorised over the points"""
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
        m = np.rint(c[2] * 1000.0)
        paired = inf & (d > 100) & (d < 2000) & (np.abs(d - m) <= float(gate_mm))
        k = np.nonzero(paired)[0]
        q, c, n, uf, vf, d = [a[k] for a in q], [a[k] for a in c], [a[k] for a in n], uf[k], vf[k], d[k]
        oz = d / 1000.0
        ox = ((uf - K[2]) * oz) / K[0]
        oy = ((vf - K[5]) * oz) / K[4]
        r = (n[0] * (ox - c[0]) + n[1] * (oy - c[1])) + n[2] * (oz - c[2])
        J = np.stack([q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]])
        S = np.empty(SUMS, np.int64)
        S[:21] = fx(J[_PI] * J[_PJ]).sum(1)            # one product per word and point, quantised, then added: integer sums
        S[21:27] = fx(J * r).sum(1)
        S[27] = fx(r * r).sum()
    return S, len(k), int(facing.sum())


def sums_of_loop(pts, nrm, R, t, depth, K, gate_mm):
    """the same one point at a time on Python floats and ints"""
    K = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    H, W = depth.shape
    R = [[float(R[a, b]) for b in range(3)] for a in range(3)]
    t = [float(v) for v in t]
    S, pairs, facing = [0] * SUMS, 0, 0

    def fx1(v):
        v = -256.0 if not v >= -256.0 else v             # fmax(v, -256): a NaN gives -256
        v = 256.0 if v > 256.0 else v
        return int(np.rint(v * TWO32))

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
            d = float(depth[int(vf), int(uf)])
            m = float(np.rint(c[2] * 1000.0))
            if not (d > 100 and d < 2000 and abs(d - m) <= float(gate_mm)):
                continue
            pairs += 1
            oz = d / 1000.0
            ox = ((uf - K[2]) * oz) / K[0]
            oy = ((vf - K[5]) * oz) / K[4]
            r = (n[0] * (ox - c[0]) + n[1] * (oy - c[1])) + n[2] * (oz - c[2])
            J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]]
            for w, (i, j) in enumerate(PAIRS):
                S[w] += fx1(J[i] * J[j])
            for i in range(6):
                S[21 + i] += fx1(J[i] * r)
            S[27] += fx1(r * r)
    return np.array(S, np.int64), pairs, facing


def solve_arrays(S, pairs, damping):
    """the step delta[6] of the normal equations, or None: a pivot that is not > 0 or a component that is not finite -- on numpy
    float64 scalars in arrays"""
    A = np.zeros((6, 6))
    for w, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = float(S[w]) * (1.0 / TWO32)
    b = np.array([float(S[21 + i]) * (1.0 / TWO32) for i in range(6)])
    for i in range(6):
        A[i, i] = A[i, i] + float(damping) * float(pairs)
    L, D = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = np.float64(0.0)
            for k in range(j):
                s = s + (L[j, k] * L[j, k]) * D[k]
            D[j] = A[j, j] - s
            if not D[j] > 0:
                return None
            for i in range(j + 1, 6):
                s = np.float64(0.0)
                for k in range(j):
                    s = s + (L[i, k] * L[j, k]) * D[k]
                L[i, j] = (A[j, i] - s) / D[j]
        yv = np.zeros(6)
        for i in range(6):
            s = np.float64(0.0)
            for k in range(i):
                s = s + L[i, k] * yv[k]
            yv[i] = b[i] - s
        for i in range(6):
            yv[i] = yv[i] / D[i]
        xv = np.zeros(6)
        for i in range(5, -1, -1):
            s = np.float64(0.0)
            for k in range(i + 1, 6):
                s = s + L[k, i] * xv[k]
            xv[i] = yv[i] - s
    return xv if np.isfinite(xv).all() else None


def solve_floats(S, pairs, damping):
    """the same on Python floats in lists"""
    import math
    inv = 1.0 / TWO32
    A = [[0.0] * 6 for _ in range(6)]
    for w, (i, j) in enumerate(PAIRS):
        A[i][j] = A[j][i] = float(int(S[w])) * inv
    b = [float(int(S[21 + i])) * inv for i in range(6)]
    for i in range(6):
        A[i][i] += float(damping) * float(int(pairs))
    L, D = [[0.0] * 6 for _ in range(6)], [0.0] * 6

    def div(a, c):
        return float(np.float64(a) / np.float64(c))      # IEEE division (inf / NaN instead of ZeroDivisionError)

    for j in range(6):
        s = 0.0
        for k in range(j):
            s = s + (L[j][k] * L[j][k]) * D[k]
        D[j] = A[j][j] - s
        if not D[j] > 0:
            return None
        for i in range(j + 1, 6):
            s = 0.0
            for k in range(j):
                s = s + (L[i][k] * L[j][k]) * D[k]
            L[i][j] = div(A[j][i] - s, D[j])
    yv = [0.0] * 6
    for i in range(6):
        s = 0.0
        for k in range(i):
            s = s + L[i][k] * yv[k]
        yv[i] = b[i] - s
    for i in range(6):
        yv[i] = div(yv[i], D[i])
    xv = [0.0] * 6
    for i in range(5, -1, -1):
        s = 0.0
        for k in range(i + 1, 6):
            s = s + L[k][i] * xv[k]
        xv[i] = yv[i] - s
    return np.array(xv) if all(math.isfinite(v) for v in xv) else None


def cayley(R, t, delta):
    """R <- C R, t <- t + v with C = ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s), a = 0.5 w -- each entry in the header's order"""
    a0, a1, a2 = 0.5 * delta[0], 0.5 * delta[1], 0.5 * delta[2]
    s = (a0 * a0 + a1 * a1) + a2 * a2
    den = 1.0 + s
    C = np.array([[((1.0 - s) + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den],
                  [(2.0 * (a1 * a0) + 2.0 * a2) / den, ((1.0 - s) + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) - 2.0 * a0) / den],
                  [(2.0 * (a2 * a0) - 2.0 * a1) / den, (2.0 * (a2 * a1) + 2.0 * a0) / den, ((1.0 - s) + 2.0 * (a2 * a2)) / den]])
    Rn = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (C[i, 0] * R[0, j] + C[i, 1] * R[1, j]) + C[i, 2] * R[2, j]
    return Rn, np.array([t[0] + delta[3], t[1] + delta[4], t[2] + delta[5]])


def _align(points, normals, poses, depth, K, gate_mm, marks, min_pairs, damping, stop, sums_fn, solve_fn):
    """{iters: (poses, records, sums)} for every iteration limit of `marks` from ONE walk per pose: a pose still running after c
    iterations is what a call with iters = c returns (status ITERS); one that stopped at or before c is the same under every limit"""
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    nrm = np.ascontiguousarray(np.asarray(normals, np.float64).reshape(-1, 3))
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    depth = np.asarray(depth)
    marks = sorted(int(m) for m in marks)
    res = {m: (P.copy(), np.zeros(len(P), REC_DTYPE), np.zeros((len(P), SUMS), np.int64)) for m in marks}
    for out, _, _ in res.values():
        out[:, 3] = (0.0, 0.0, 0.0, 1.0)
    with np.errstate(all="ignore"):
        for p in range(len(P)):
            R, t = P[p, :3, :3].copy(), P[p, :3, 3].copy()
            rec = np.zeros((), REC_DTYPE)
            left = list(marks)
            for it in range(marks[-1]):
                S, pairs, facing = sums_fn(pts, nrm, R, t, depth, K, gate_mm)
                rec["iterations"], rec["pairs"], rec["facing_pts"], rec["sum_r2"] = it + 1, pairs, facing, S[27]
                if it == 0:
                    rec["pairs0"], rec["sum_r2_0"] = pairs, S[27]
                status = ITERS
                if pairs < int(min_pairs):
                    status = FEW
                else:
                    delta = solve_fn(S, pairs, damping)
                    if delta is None:
                        status = SINGULAR
                    else:
                        R, t = cayley(R, t, delta)
                        if np.abs(delta).max() <= float(stop):
                            status = CONVERGED
                rec["status"] = status
                done = [m for m in left if status != ITERS or m == it + 1]
                for m in done:
                    out, recs, sums = res[m]
                    out[p, :3, :3], out[p, :3, 3], recs[p], sums[p] = R, t, rec, S
                    left.remove(m)
                if not left:
                    break
    return res


def align(points, normals, poses, depth, K, gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6):
    """-> (poses [n,4,4], records [n] REC_DTYPE, sums int64 [n,28]), vectorised over the points, the solve on Python floats"""
    return _align(points, normals, poses, depth, K, gate_mm, [iters], min_pairs, damping, stop, sums_of, solve_floats)[int(iters)]


def align_limits(points, normals, poses, depth, K, limits, gate_mm=20, min_pairs=12, damping=1e-6, stop=1e-6):
    """{iters: align(..., iters=iters)} for every iteration limit of `limits`, from one walk per pose (the limits share their start)"""
    return _align(points, normals, poses, depth, K, gate_mm, limits, min_pairs, damping, stop, sums_of, solve_floats)


def align_loop(points, normals, poses, depth, K, gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6):
    """the same rule one point at a time on Python floats, the solve on numpy scalars: what align() is checked against"""
    return _align(points, normals, poses, depth, K, gate_mm, [iters], min_pairs, damping, stop, sums_of_loop, solve_arrays)[int(iters)]


def pose_error(pose, truth):
    """(translation error in metres, rotation error in degrees)"""
    dR = pose[:3, :3] @ truth[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(pose[:3, 3] - truth[:3, 3])), float(ang)
