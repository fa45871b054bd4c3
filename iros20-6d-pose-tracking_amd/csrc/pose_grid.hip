// Searching a product lattice of poses (se3tn_score_pose_grid): n_rot rotations x n_trans translations scored against ONE observed
// depth frame, candidate r * n_trans + t being the pose [R_r | t_t].  The candidates are never materialised: the factors travel
// (72 + 24 bytes per rotation / translation instead of 128 per pose), and the part of a point's transform that depends on the
// rotation alone is computed once per rotation.
//
// The rule of a point x_j with normal n_j under candidate (r, t), float64, in this operation order (include/se3tracknet.h states it
// in full):
//     q  = (R0 x + R1 y) + R2 z  per row              the rotated part of transform() (pose_transform.h), its first three roundings
//     c  = q + t                                      its last rounding: c has the bits transform() gives for the composed pose
//     with facing:  n' = (R0 nx + R1 ny) + R2 nz per row,  f = (n'x c.x + n'y c.y) + n'z c.z,  the point counts only if f < 0
//     in front / uf, vf / in frame / d, m / seen / inlier, front, behind     exactly as pose_search.hip
// The file is compiled with -ffp-contract=off (csrc/Makefile) like pose_search.hip: every counter must EQUAL the numpy oracle's.
//
// One workgroup of PG_THREADS threads per (rotation, tile of PG_TT translations) -- pose_grid_plan.h has the index arithmetic.  Per
// tile of PG_PT model points: all threads rotate the tile into LDS (three planes of doubles, six with the normals); then wave w
// walks the translations w, w + 4, ... of its tile, its lanes stride over the tile's points reading LDS, the counters go through
// wave64 xor shuffles and lane 0 adds them to the translation's row of LDS words -- a row has one owner wave, so no atomics.  After
// the last point tile the records are written once with plain vector stores.  Integer sums only, nothing allocated: a record
// depends on (points, normals, R_r, t_t, depth, K, tol, facing) alone.
#include "pose_grid_plan.h"
#include "se3tn_internal.h"

namespace se3tn {

template <bool FACING>
__global__ __launch_bounds__(PG_THREADS) void pose_grid_kernel(const PoseGridArgs a) {
  extern __shared__ double pg_lds[];   // [3 | 6][PG_PT] rotated points (and normals), then PG_TT rows of PG_ROW_WORDS counters
  constexpr int NC = FACING ? 6 : 5;   // counters of a row in use: [points |] in frame, seen, inlier, front, behind
  double* const qx = pg_lds;
  double* const qy = pg_lds + PG_PT;
  double* const qz = pg_lds + 2 * PG_PT;
  unsigned* const rows = reinterpret_cast<unsigned*>(pg_lds + (FACING ? 6 : 3) * PG_PT);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = pg_rot_of((int)blockIdx.x, a.n_trans);
  const int t0 = pg_trans0_of((int)blockIdx.x, a.n_trans);
  const int nt = pg_trans_count(t0, a.n_trans);
  if (t < PG_TT * PG_ROW_WORDS) rows[t] = 0u;   // (the first tile's barrier below orders this before any wave's first sum)
  const double* sr = a.rots + (size_t)r * 9;    // the rotation: nine uniform loads, kept in registers
  const double r00 = sr[0], r01 = sr[1], r02 = sr[2], r10 = sr[3], r11 = sr[4], r12 = sr[5], r20 = sr[6], r21 = sr[7], r22 = sr[8];
  const double W = (double)a.W, H = (double)a.H, tol = (double)a.tol;
  const double fx = a.K[0], cx0 = a.K[2], fy = a.K[4], cy0 = a.K[5];
  for (int p0 = 0; p0 < a.P; p0 += PG_PT) {
    const int np = pg_point_count(p0, a.P);
    if (p0 > 0) __syncthreads();   // the previous tile's readers are done
    for (int j = t; j < np; j += PG_THREADS) {
      const double* x = a.pts + 3 * (size_t)(p0 + j);
      qx[j] = (r00 * x[0] + r01 * x[1]) + r02 * x[2];
      qy[j] = (r10 * x[0] + r11 * x[1]) + r12 * x[2];
      qz[j] = (r20 * x[0] + r21 * x[1]) + r22 * x[2];
      if (FACING) {
        const double* n = a.nrm + 3 * (size_t)(p0 + j);
        qx[3 * PG_PT + j] = (r00 * n[0] + r01 * n[1]) + r02 * n[2];
        qy[3 * PG_PT + j] = (r10 * n[0] + r11 * n[1]) + r12 * n[2];
        qz[3 * PG_PT + j] = (r20 * n[0] + r21 * n[1]) + r22 * n[2];
      }
    }
    __syncthreads();
    for (int k = wave; k < nt; k += PG_WAVES) {   // pg_wave_of(k) == wave: this wave's translations of the tile
      const double* tr = a.trans + 3 * (size_t)(t0 + k);
      const double tx = tr[0], ty = tr[1], tz = tr[2];
      unsigned v[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // points (facing), in frame, seen, inlier, front, behind
#pragma unroll 2
      for (int j = lane; j < np; j += 64) {
        const double cx = qx[j] + tx, cy = qy[j] + ty, cz = qz[j] + tz;
        if (FACING) {
          const double f = (qx[3 * PG_PT + j] * cx + qy[3 * PG_PT + j] * cy) + qz[3 * PG_PT + j] * cz;
          if (!(f < 0.0)) continue;   // turned away, grazing (f == 0) or NaN: the point enters no counter
          v[0] += 1u;
        }
        const bool front = cz > 0.0;
        const double uf = rint(cx * fx / cz + cx0);
        const double vf = rint(cy * fy / cz + cy0);
        // every comparison is false for NaN; +-inf and anything beyond the frame fail one of them: only an index reaches the cast
        if (front && uf >= 0.0 && uf < W && vf >= 0.0 && vf < H) {
          v[1] += 1u;
          const size_t q = (size_t)(int)vf * (size_t)a.W + (size_t)(int)uf;
          const double d = (double)a.depth[q];
          if (d > 100.0 && d < 2000.0) {
            const double m = rint(cz * 1000.0);
            v[2] += 1u;
            if (fabs(d - m) <= tol) v[3] += 1u;
            if (d < m - tol) v[4] += 1u;
            if (d > m + tol) v[5] += 1u;
          }
        }
      }
#pragma unroll
      for (int c = 6 - NC; c < 6; ++c) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[c] += __shfl_xor(v[c], s, 64);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 6 - NC; c < 6; ++c) rows[k * PG_ROW_WORDS + c] += v[c];
      }
    }
  }
  __syncthreads();
  if (t < nt * PS_FIT_WORDS) {   // the records' eight words, one lane each: points | in frame, seen, inlier, front, behind | tol | 0
    const int k = t / PS_FIT_WORDS, w = t % PS_FIT_WORDS;
    unsigned val = 0u;
    if (w == 0) val = FACING ? rows[k * PG_ROW_WORDS] : (unsigned)a.P;
    else if (w < 6) val = rows[k * PG_ROW_WORDS + w];
    else if (w == 6) val = (unsigned)a.tol;
    reinterpret_cast<unsigned*>(a.out + pg_candidate(r, t0 + k, a.n_trans))[w] = val;
    __threadfence_system();   // (the record may live in mapped host memory)
  }
}

hipError_t launch_pose_grid(const PoseGridArgs& a, int n_rot, hipStream_t st) {
  if (n_rot < 1 || a.n_trans < 1 || (long long)n_rot * a.n_trans > PS_MAX_POSES || a.P < 1 || a.P > SE3TN_POSE_ERRORS_MAX_POINTS ||
      a.H < 1 || a.W < 1 || a.tol < 1 || a.tol > 65535 || (a.facing && a.nrm == nullptr))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)pg_grid(n_rot, a.n_trans));
  if (a.facing) hipLaunchKernelGGL(pose_grid_kernel<true>, grid, dim3(PG_THREADS), pg_lds_bytes(1), st, a);
  else hipLaunchKernelGGL(pose_grid_kernel<false>, grid, dim3(PG_THREADS), pg_lds_bytes(0), st, a);
  return hipGetLastError();
}

}  // namespace se3tn
