// ADD / ADD-S of n pose pairs (se3tn_pose_errors; Utils.py:72-98 `add` / `adi` of the reference, which builds a KD-tree per frame).
// For pair i, with the model points x_j (j < P), a_j = R_pred x_j + t_pred and b_j = R_gt x_j + t_gt:
//     add[i]  = mean_j |a_j - b_j|
//     adds[i] = mean_j min_k |b_j - a_k|        (the PRED cloud is the reference set, the GT cloud queries it: Utils.py:92-97)
// float64 throughout, all pairs of points, no tree: n P^2 distance evaluations of 9 float64 operations each.  What bounds it is the
// float64 vector rate (one wave instruction per four clocks and SIMD): the reference point of the inner loop is one LDS address for
// the whole wave (a broadcast, no bank conflict) and serves PE_QPT query points a thread holds in registers, so LDS carries
// 24 bytes per 36 vector instructions of a wave.
//
// Guarantees (include/se3tracknet.h)
//  (a) equal poses give exactly 0.0 twice: BOTH clouds go through transform() below -- one function, one operation order -- and the
//      file is compiled with -ffp-contract=off (csrc/Makefile), so x_j has the same bits as a_j and as b_j; |a_j - b_j| = sqrt(0) and the
//      minimum over k meets k = j.
//  (b) a pair's results depend on (points, pred_i, gt_i) only.  The minimum is order-free.  Sums: a thread adds its PE_QPT slots in
//      slot order, a wave adds by xor shuffles 32, 16, .. 1 (both partners of a step form the same commutative sum), the four waves are
//      added in index order through LDS, a workgroup stores its two sums at [pair][tile] with plain vector stores, and the finish
//      launch adds a pair's tiles in index order and divides by P.  No floating-point atomics; the tiling depends on P alone.
//  (c) nothing is allocated: the scratch [PE_CHUNK][tiles][2] belongs to the points handle.
// The inner loop keeps the minimum SQUARED distance; one sqrt per query point at the end (sqrt is monotone).
#include "pose_errors_plan.h"
#include "pose_transform.h"
#include "record_reduce.h"
#include "se3tn_internal.h"

namespace se3tn {

// Rigid, load_pose and THE transform of both clouds (pose_transform.h: shared with pose_search.hip, one operation order)

template <bool ADDS>
__global__ __launch_bounds__(PE_THREADS) void pose_errors_kernel(const PoseErrArgs a) {
  __shared__ __attribute__((aligned(16))) double sx[PE_REF_TILE];
  __shared__ __attribute__((aligned(16))) double sy[PE_REF_TILE];
  __shared__ __attribute__((aligned(16))) double sz[PE_REF_TILE];
  __shared__ double red[2][PE_THREADS / 64];
  const int t = threadIdx.x;
  const int tile = blockIdx.x, pair = blockIdx.y, tiles = gridDim.x;
  const int P = a.P;
  const Rigid Tp = load_pose(a.pred + (size_t)pair * 16);
  const Rigid Tg = load_pose(a.gt + (size_t)pair * 16);

  double bx[PE_QPT], by[PE_QPT], bz[PE_QPT], m[PE_QPT];
  bool live[PE_QPT];
  double s_add = 0.0;
#pragma unroll
  for (int s = 0; s < PE_QPT; ++s) {
    const long long j = pe_query_index(tile, s, t);
    live[s] = j < P;
    const size_t jj = live[s] ? (size_t)j : (size_t)(P - 1);   // an empty slot reads the last point and its result is dropped
    const double x = a.pts[3 * jj], y = a.pts[3 * jj + 1], z = a.pts[3 * jj + 2];
    transform(Tg, x, y, z, bx[s], by[s], bz[s]);
    double ax, ay, az;
    transform(Tp, x, y, z, ax, ay, az);
    const double dx = ax - bx[s], dy = ay - by[s], dz = az - bz[s];
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    s_add += live[s] ? d : 0.0;
    m[s] = __builtin_inf();
  }

  double s_adds = 0.0;
  if (ADDS) {
    for (int r0 = 0; r0 < P; r0 += PE_REF_TILE) {
      const int cnt = P - r0 < PE_REF_TILE ? P - r0 : PE_REF_TILE;
      __syncthreads();   // the previous tile has been read by every wave
      for (int k = t; k < cnt; k += PE_THREADS) {
        const size_t j = (size_t)r0 + k;
        transform(Tp, a.pts[3 * j], a.pts[3 * j + 1], a.pts[3 * j + 2], sx[k], sy[k], sz[k]);
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < cnt; ++k) {
        const double rx = sx[k], ry = sy[k], rz = sz[k];   // one address for the whole wave
#pragma unroll
        for (int s = 0; s < PE_QPT; ++s) {
          const double dx = bx[s] - rx, dy = by[s] - ry, dz = bz[s] - rz;
          m[s] = __builtin_fmin(m[s], (dx * dx + dy * dy) + dz * dz);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < PE_QPT; ++s) s_adds += live[s] ? sqrt(m[s]) : 0.0;
  }

  s_add = wave_sum(s_add);
  if (ADDS) s_adds = wave_sum(s_adds);
  if ((t & 63) == 0) {
    red[0][t >> 6] = s_add;
    red[1][t >> 6] = s_adds;
  }
  __syncthreads();
  if (t < 2) {   // lane 0: the |a - b| sum, lane 1: the closest-distance sum; the four waves in index order
    const double v = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
    a.part[pe_partial_index(pair, tile, tiles) + t] = v;
  }
}

// one thread per pair of the chunk: the tiles in index order, then the mean
__global__ __launch_bounds__(PE_THREADS) void pose_errors_finish_kernel(const PoseErrArgs a, int count, int tiles) {
  const int pair = blockIdx.x * PE_THREADS + threadIdx.x;
  if (pair >= count) return;
  double s0 = 0.0, s1 = 0.0;
  for (int tile = 0; tile < tiles; ++tile) {
    const size_t q = pe_partial_index(pair, tile, tiles);
    s0 += a.part[q];
    if (a.adds) s1 += a.part[q + 1];
  }
  const double P = (double)a.P;
  if (a.add) a.add[pair] = s0 / P;
  if (a.adds) a.adds[pair] = s1 / P;
}

hipError_t launch_pose_errors(const PoseErrArgs& a, int count, hipStream_t st) {
  if (count < 1 || count > PE_CHUNK || a.P < 1 || a.P > PE_MAX_POINTS) return hipErrorInvalidValue;
  const int tiles = pe_query_tiles(a.P);
  if (a.adds) hipLaunchKernelGGL(pose_errors_kernel<true>, dim3(tiles, count), dim3(PE_THREADS), 0, st, a);
  else hipLaunchKernelGGL(pose_errors_kernel<false>, dim3(tiles, count), dim3(PE_THREADS), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pose_errors_finish_kernel, dim3((count + PE_THREADS - 1) / PE_THREADS), dim3(PE_THREADS), 0, st, a, count, tiles);
  return hipGetLastError();
}

}  // namespace se3tn
