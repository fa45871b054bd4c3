// Aligning pose hypotheses to the depth frame (se3tn_align_poses): a few damped point-to-plane Gauss-Newton steps of the model's
// facing points against ONE observed depth frame, for n poses in ONE launch -- the link between a node of the search lattices
// (pose_search.hip, pose_grid.hip: 10 mm, 15 degrees) and a pose the network can take over.
//
// The rule (include/se3tracknet.h states it in full) lives in pose_align_math.h, host and device: the terms of a point, their
// quantisation fx(), the LDL^T solve and the Cayley update.  This file is the walk and the reduction around those statements; it is
// compiled with -ffp-contract=off (csrc/Makefile) like its neighbours: every word must EQUAL the numpy oracle's.
//
// One workgroup of PA_THREADS threads per pose, all iterations inside the launch (pose_align_plan.h).  Per iteration: thread t walks
// the points t, t + PA_THREADS, ... reading the handle's points and normals from global memory (the same few KB every iteration:
// they stay in L2), and keeps the 28 int64 sums and the two counts in registers; wave64 xor shuffles; the waves' rows through LDS;
// thread 0 solves and publishes the new pose through LDS; a barrier, and the next iteration starts.  Integer sums only: the result
// does not depend on the order of the reduction, so not on the thread count either.  No atomics, no grid-wide synchronisation,
// nothing allocated, no traffic between workgroups: a pose's output depends on (points, normals, pose, depth, K, params) alone.
//
// SCENE (se3tn_align_poses_scene) is the same kernel with pa_point_scene() in the point loop: a second 2-byte gather, from a.scene at
// the pixel index the depth gather computed, issued beside it; a third count, hidden; rows of PA_SCENE_ROW_WORDS words; and thread 0
// keeps the hidden points of the pose pa_step last evaluated for the record's word at offset 28.  The <false> instantiation keeps
// its arithmetic, its LDS layout and its launch geometry.
#include "pose_align_math.h"
#include "pose_align_plan.h"
#include "record_reduce.h"
#include "se3tn_internal.h"

namespace se3tn {

template <bool SCENE>
__global__ __launch_bounds__(PA_THREADS) void pose_align_kernel(const PoseAlignArgs a) {
  constexpr int RW = SCENE ? PA_SCENE_ROW_WORDS : PA_ROW_WORDS;
  constexpr int TOTAL = PA_WAVES * RW;        // pa_lds_total() / pa_scene_lds_total(); wave w's row starts at w * RW
  __shared__ long long red[TOTAL + RW];       // pa_lds_words() / pa_scene_lds_words(): the waves' rows, then the totals
  __shared__ double sp[12];                                  // rows 0-2 of the pose, as thread 0 last left it
  __shared__ int done;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t pose = blockIdx.x;
  if (t < 12) sp[t] = a.poses[pose * 16 + t];   // rows 0-2: read before anything is written, so poses_out may be poses
  if (t == 0) done = 0;
  __syncthreads();
  const DepthFrame f = depth_frame(a.depth, a.H, a.W, a.K);
  const double gate = (double)a.p.gate_mm;
  const double scene_tol = (double)a.scene_tol;
  uint32_t hidden_pts = 0u;   // thread 0's: the hidden points of the last evaluated pose
  se3tn_align_rec rec;   // thread 0's
  rec.iterations = 0u; rec.status = SE3TN_ALIGN_ITERS; rec.pairs = 0u; rec.facing_pts = 0u; rec.sum_r2 = 0;
  rec.pairs0 = 0u; rec._reserved = 0u; rec.sum_r2_0 = 0;
  for (int it = 0; it < a.p.iters; ++it) {
    Rigid T = load_pose(sp);
    int64_t S[PA_SUMS];
#pragma unroll
    for (int w = 0; w < PA_SUMS; ++w) S[w] = 0;
    long long pairs = 0, facing = 0;
    int hidden = 0;   // (32 bits: at most P <= 2^20 points)
    for (int j = pa_first(t); j < a.P; j += pa_stride()) {
      const double* x = a.pts + 3 * (size_t)j;
      const double* n = a.nrm + 3 * (size_t)j;
      double J[6], r;
      const int k = SCENE ? pa_point_scene(T, f, a.scene, scene_tol, gate, x[0], x[1], x[2], n[0], n[1], n[2], J, r)
                          : pa_point(T, f, gate, x[0], x[1], x[2], n[0], n[1], n[2], J, r);
      facing += k & 1;
      if (SCENE) hidden += (k >> 2) & 1;
      if (k & 2) {
        pairs += 1;
        pa_accumulate(J, r, S);
      }
    }
#pragma unroll
    for (int w = 0; w < PA_SUMS; ++w) S[w] = wave_sum(S[w]);
    pairs = wave_sum(pairs);
    facing = wave_sum(facing);
    if (SCENE) hidden = wave_sum(hidden);
    if (lane == 0) {
      long long* row = red + wave * RW;
#pragma unroll
      for (int w = 0; w < PA_SUMS; ++w) row[w] = S[w];
      row[PA_W_PAIRS] = pairs;
      row[PA_W_FACING] = facing;
      if (SCENE) row[PA_W_HIDDEN] = hidden;
    }
    __syncthreads();
    if (t < RW) {
      long long s = 0;
#pragma unroll
      for (int w = 0; w < PA_WAVES; ++w) s += red[w * RW + t];
      red[TOTAL + t] = s;
    }
    __syncthreads();
    if (t == 0) {
      const long long* tot = red + TOTAL;
      int64_t St[PA_SUMS];
#pragma unroll
      for (int w = 0; w < PA_SUMS; ++w) St[w] = tot[w];
      const bool fin = pa_step(T, St, (uint32_t)tot[PA_W_PAIRS], (uint32_t)tot[PA_W_FACING], it, a.p, rec);
      if (SCENE) hidden_pts = (uint32_t)tot[PA_W_HIDDEN];
      // a pose that stopped FEW or SINGULAR was not touched: its doubles stay in LDS with the bits they came in with
      if (rec.status == SE3TN_ALIGN_ITERS || rec.status == SE3TN_ALIGN_CONVERGED) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          sp[4 * i] = T.r[i][0]; sp[4 * i + 1] = T.r[i][1]; sp[4 * i + 2] = T.r[i][2]; sp[4 * i + 3] = T.t[i];
        }
      }
      done = fin ? 1 : 0;
    }
    __syncthreads();   // the new pose and `done` are published; red is rewritten only after the next iteration's walk
    if (done) break;   // uniform: every thread reads the same word
  }
  // the pose (row 3 is 0 0 0 1), the record's ten words and the last sums: plain vector stores, every word once
  if (t < 16) a.poses_out[pose * 16 + t] = t < 12 ? sp[t] : (t == 15 ? 1.0 : 0.0);
  if (a.sums != nullptr && t < PA_SUMS) a.sums[pose * PA_SUMS + t] = red[TOTAL + t];
  if (t == 0) {
    if (SCENE) reinterpret_cast<se3tn_scene_align_rec*>(a.rec)[pose] = pa_scene_rec(rec, hidden_pts);
    else a.rec[pose] = rec;
  }
}

hipError_t launch_pose_align(const PoseAlignArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > PA_MAX_POSES || a.P < 1 || a.P > SE3TN_POSE_ERRORS_MAX_POINTS || a.H < 1 || a.W < 1 || a.nrm == nullptr ||
      a.p.gate_mm < 1 || a.p.gate_mm > 65535 || a.p.iters < 1 || a.p.iters > PA_MAX_ITERS || a.p.min_pairs < 6)
    return hipErrorInvalidValue;
  if (a.scene != nullptr) {   // the scene-aware rule: a.rec holds se3tn_scene_align_rec records
    if (a.scene_tol < 1 || a.scene_tol > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_align_kernel<true>, dim3(n), dim3(PA_THREADS), 0, st, a);
  } else hipLaunchKernelGGL(pose_align_kernel<false>, dim3(n), dim3(PA_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace se3tn
