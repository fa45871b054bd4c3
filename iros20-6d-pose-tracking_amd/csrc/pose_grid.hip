// Searching a product lattice of poses (se3tn_score_pose_grid): n_rot rotations x n_trans translations scored against ONE observed
// depth frame, candidate r * n_trans + t being the pose [R_r | t_t].  The candidates are never materialised: the factors travel
// (72 + 24 bytes per rotation / translation instead of 128 per pose), and the part of a point's transform that depends on the
// rotation alone is computed once per rotation.
//
// The rule of a point under candidate (r, t) lives in pose_point_rule.h: q = rotate(x) by R_r, c = q + t_t -- the bits transform()
// gives for the composed pose, its five roundings cut after the third -- then faces() with the rotated normal where `facing` asks
// for it, and count_point(); include/se3tracknet.h states it in full.  The file is compiled with -ffp-contract=off (csrc/Makefile):
// every counter must EQUAL the numpy oracle's.
//
// One workgroup of PG_THREADS threads per (rotation, tile of PG_TT translations) -- pose_grid_plan.h has the index arithmetic.  Per
// tile of PG_PT model points: all threads rotate the tile into LDS (three planes of doubles, six with the normals); then wave w
// walks the translations w, w + 4, ... of its tile, its lanes stride over the tile's points reading LDS, the counters go through
// wave64 xor shuffles and lane 0 adds them to the translation's row of LDS words -- a row has one owner wave, so no atomics.  After
// the last point tile the records are written once with plain vector stores.  Integer sums only, nothing allocated: a record
// depends on (points, normals, R_r, t_t, depth, K, tol, facing) alone.
//
// SCENE (se3tn_score_pose_grid_scene) is the same kernel with count_point_scene() in the point loop: a second 2-byte gather, from
// a.scene at the pixel index the depth gather computed, and a seventh counter, hidden, in a row of PG_SCENE_ROW_WORDS words.  The
// planes keep their layout (each contiguous, lane l reads double l of a run of 64: conflict-free); only the rows behind them grow,
// by 64 bytes per workgroup, so six / three workgroups share a CU as before.  Compiled for gfx950 the four instantiations take
// <facing, scene> = <0,0> 58, <1,0> 64, <0,1> 62, <1,1> 64 VGPRs, none spills, all at 8 waves per SIMD by registers -- LDS, not
// registers, bounds the residency (3 workgroups = 12 waves per CU with facing), for both rules alike.  The <., false> instantiations
// compile to the instructions they had before SCENE existed.  count_point_scene adds to every counter by name, without a branch
// that picks one: with `hidden: add and return` the compiler addressed the counters through a pointer and kept them in scratch.
#include "pose_grid_plan.h"
#include "pose_point_rule.h"
#include "se3tn_internal.h"

namespace se3tn {

template <bool FACING, bool SCENE>
__global__ __launch_bounds__(PG_THREADS) void pose_grid_kernel(const PoseGridArgs a) {
  extern __shared__ double pg_lds[];   // [3 | 6][PG_PT] rotated points (and normals), then PG_TT rows of RW counters
  constexpr int RW = SCENE ? PG_SCENE_ROW_WORDS : PG_ROW_WORDS;
  constexpr int C0 = FACING ? 0 : 1;   // counters of a row in use, [C0, RW): [points |] in frame, seen, inlier, front, behind [| hidden]
  double* const qx = pg_lds;
  double* const qy = pg_lds + PG_PT;
  double* const qz = pg_lds + 2 * PG_PT;
  unsigned* const rows = reinterpret_cast<unsigned*>(pg_lds + (FACING ? 6 : 3) * PG_PT);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = pg_rot_of((int)blockIdx.x, a.n_trans);
  const int t0 = pg_trans0_of((int)blockIdx.x, a.n_trans);
  const int nt = pg_trans_count(t0, a.n_trans);
  if (t < PG_TT * RW) rows[t] = 0u;   // (the first tile's barrier below orders this before any wave's first sum)
  const double* sr = a.rots + (size_t)r * 9;    // the rotation: nine uniform loads, kept in registers
  const double R[3][3] = {{sr[0], sr[1], sr[2]}, {sr[3], sr[4], sr[5]}, {sr[6], sr[7], sr[8]}};
  const DepthFrame f = depth_frame(a.depth, a.H, a.W, a.K);
  const double tol = (double)a.tol;
  for (int p0 = 0; p0 < a.P; p0 += PG_PT) {
    const int np = pg_point_count(p0, a.P);
    if (p0 > 0) __syncthreads();   // the previous tile's readers are done
    for (int j = t; j < np; j += PG_THREADS) {
      const double* x = a.pts + 3 * (size_t)(p0 + j);
      rotate(R, x[0], x[1], x[2], qx[j], qy[j], qz[j]);
      if (FACING) {
        const double* n = a.nrm + 3 * (size_t)(p0 + j);
        rotate(R, n[0], n[1], n[2], qx[3 * PG_PT + j], qy[3 * PG_PT + j], qz[3 * PG_PT + j]);
      }
    }
    __syncthreads();
    for (int k = wave; k < nt; k += PG_WAVES) {   // pg_wave_of(k) == wave: this wave's translations of the tile
      const double* tr = a.trans + 3 * (size_t)(t0 + k);
      const double tx = tr[0], ty = tr[1], tz = tr[2];
      unsigned v[RW] = {};   // points (facing), in frame, seen, inlier, front, behind (, hidden)
#pragma unroll 2
      for (int j = lane; j < np; j += 64) {
        const double cx = qx[j] + tx, cy = qy[j] + ty, cz = qz[j] + tz;
        if (FACING) {   // turned away, grazing (f == 0) or NaN: the point enters no counter
          if (!faces(qx[3 * PG_PT + j], qy[3 * PG_PT + j], qz[3 * PG_PT + j], cx, cy, cz)) continue;
          v[0] += 1u;
        }
        if (SCENE) count_point_scene(f, a.scene, tol, cx, cy, cz, v + 1);
        else count_point(f, tol, cx, cy, cz, v + 1);
      }
#pragma unroll
      for (int c = C0; c < RW; ++c) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[c] += __shfl_xor(v[c], s, 64);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = C0; c < RW; ++c) rows[k * RW + c] += v[c];
      }
    }
  }
  __syncthreads();
  if (t < nt * PS_FIT_WORDS) {   // the records' eight words, one lane each: points | in frame, seen, inlier, front, behind | tol | 0 or hidden
    const int k = t / PS_FIT_WORDS, w = t % PS_FIT_WORDS;
    unsigned val = 0u;
    if (w == 0) val = FACING ? rows[k * RW] : (unsigned)a.P;
    else if (w < 6) val = rows[k * RW + w];
    else if (w == 6) val = (unsigned)a.tol;
    else if (SCENE) val = rows[k * RW + PG_SCENE_HIDDEN];
    reinterpret_cast<unsigned*>(a.out + pg_candidate(r, t0 + k, a.n_trans))[w] = val;
    __threadfence_system();   // (the record may live in mapped host memory)
  }
}

hipError_t launch_pose_grid(const PoseGridArgs& a, int n_rot, hipStream_t st) {
  if (n_rot < 1 || a.n_trans < 1 || (long long)n_rot * a.n_trans > PS_MAX_POSES || a.P < 1 || a.P > SE3TN_POSE_ERRORS_MAX_POINTS ||
      a.H < 1 || a.W < 1 || a.tol < 1 || a.tol > 65535 || (a.facing && a.nrm == nullptr))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)pg_grid(n_rot, a.n_trans));
  if (a.scene) {   // the scene-aware rule: a.out holds se3tn_scene_point_fit records
    if (a.facing) hipLaunchKernelGGL((pose_grid_kernel<true, true>), grid, dim3(PG_THREADS), pg_scene_lds_bytes(1), st, a);
    else hipLaunchKernelGGL((pose_grid_kernel<false, true>), grid, dim3(PG_THREADS), pg_scene_lds_bytes(0), st, a);
  } else if (a.facing) hipLaunchKernelGGL((pose_grid_kernel<true, false>), grid, dim3(PG_THREADS), pg_lds_bytes(1), st, a);
  else hipLaunchKernelGGL((pose_grid_kernel<false, false>), grid, dim3(PG_THREADS), pg_lds_bytes(0), st, a);
  return hipGetLastError();
}

}  // namespace se3tn
