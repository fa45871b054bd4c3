// Re-acquiring a lost object (se3tn_score_poses, se3tn_rank_poses): n candidate poses scored against ONE observed depth frame by
// projecting the model's points, and the k best picked.  The reference's answer to a lost track is an external detector
// (predict.py:539-541: PoseCNN at the frames --reinit_frames lists); a render per candidate would cost a rasteriser pass each.
//
// The rule of a point under a candidate lives in pose_point_rule.h (count_point(), after transform() of pose_transform.h);
// include/se3tracknet.h states it in full.  The file is compiled with -ffp-contract=off (csrc/Makefile): every counter must EQUAL
// the numpy oracle's.
//
// Scoring: one workgroup of PS_THREADS threads per pose.  The pose's twelve doubles are loaded once (twelve lanes, through LDS);
// thread t takes the points t, t + 256, ... and keeps five counters in registers; wave64 xor shuffles, the four waves through LDS,
// then lanes 0-7 store the record's eight words once with plain vector stores.  Integer sums only, no atomics, nothing allocated: a
// record depends on (points, pose, depth, K, tol) alone.
// Ranking: ONE workgroup; round r finds the largest key (pose_search_plan.h: ps_key) below round r - 1's winner -- k passes over
// the n records, no scratch, the same result on every run because keys are unique.
#include "pose_point_rule.h"
#include "pose_search_plan.h"
#include "record_reduce.h"
#include "se3tn_internal.h"

namespace se3tn {

__global__ __launch_bounds__(PS_THREADS) void pose_score_kernel(const PoseScoreArgs a) {
  __shared__ double sp[12];
  __shared__ unsigned part[PS_WAVES][5];
  const int t = threadIdx.x;
  const size_t pose = blockIdx.x;
  if (t < 12) sp[t] = a.poses[pose * 16 + t];   // rows 0-2 of the pose: loaded once per workgroup
  __syncthreads();
  const Rigid T = load_pose(sp);
  const DepthFrame f = depth_frame(a.depth, a.H, a.W, a.K);
  const double tol = (double)a.tol;
  unsigned v[5] = {0u, 0u, 0u, 0u, 0u};   // in frame, seen, inlier, front, behind
  for (int j = t; j < a.P; j += PS_THREADS) {
    double cx, cy, cz;
    transform(T, a.pts[3 * (size_t)j], a.pts[3 * (size_t)j + 1], a.pts[3 * (size_t)j + 2], cx, cy, cz);
    count_point(f, tol, cx, cy, cz, v);
  }
  wave_sums_to_lds(v, part);
  __syncthreads();
  if (t < PS_FIT_WORDS) {   // the record's eight words, one lane each: points | in frame, seen, inlier, front, behind | tol | 0
    unsigned r = 0u;
    if (t == 0) r = (unsigned)a.P;
    else if (t < 6) r = ((part[0][t - 1] + part[1][t - 1]) + part[2][t - 1]) + part[3][t - 1];
    else if (t == 6) r = (unsigned)a.tol;
    reinterpret_cast<unsigned*>(a.out + pose)[t] = r;
    __threadfence_system();   // (the record may live in mapped host memory)
  }
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_xor(v, s, 64);
    v = o > v ? o : v;
  }
  return v;
}

// keys travel as key + 1 inside the kernel: 0 is "none yet" (a key itself may be 0: no inliers, index 2^20 - 1)
__global__ __launch_bounds__(PS_THREADS) void pose_rank_kernel(const se3tn_point_fit* fit, int n, int k, int32_t* idx,
                                                               se3tn_point_fit* top_fit) {
  __shared__ unsigned long long red[PS_WAVES];
  __shared__ unsigned long long win;
  const int t = threadIdx.x;
  unsigned long long bound = ~0ull;
  for (int r = 0; r < k; ++r) {
    unsigned long long best = 0ull;
    for (int i = t; i < n; i += PS_THREADS) {
      const unsigned long long q = ps_key(fit[i].inlier_pts, fit[i].behind_pts, (uint32_t)i) + 1ull;
      if (q < bound && q > best) best = q;
    }
    best = wave_max(best);
    if ((t & 63) == 0) red[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
      unsigned long long b = red[0];
#pragma unroll
      for (int w = 1; w < PS_WAVES; ++w) b = red[w] > b ? red[w] : b;
      win = b;
    }
    __syncthreads();   // (red is rewritten only after the next round's scan, win only after the next round's first barrier)
    bound = win;       // k <= n: a key below the bound exists in every round, so win >= 1
    const uint32_t w = ps_key_index(bound - 1ull);
    if (t == 0) idx[r] = (int32_t)w;
    if (top_fit != nullptr && t < PS_FIT_WORDS)
      reinterpret_cast<unsigned*>(top_fit + r)[t] = reinterpret_cast<const unsigned*>(fit + w)[t];
  }
  if (t < PS_FIT_WORDS) __threadfence_system();   // (idx / top_fit may live in mapped host memory)
}

hipError_t launch_pose_score(const PoseScoreArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > PS_MAX_POSES || a.P < 1 || a.P > SE3TN_POSE_ERRORS_MAX_POINTS || a.H < 1 || a.W < 1 || a.tol < 1 || a.tol > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pose_score_kernel, dim3(n), dim3(PS_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pose_rank(const se3tn_point_fit* fit, int n, int k, int32_t* idx, se3tn_point_fit* top_fit, hipStream_t st) {
  if (n < 1 || n > PS_MAX_POSES || k < 1 || k > PS_RANK_MAX || k > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pose_rank_kernel, dim3(1), dim3(PS_THREADS), 0, st, fit, n, k, idx, top_fit);
  return hipGetLastError();
}

}  // namespace se3tn
