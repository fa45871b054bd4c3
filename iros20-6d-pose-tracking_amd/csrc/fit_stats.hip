// Fit record of a pose estimate (se3tn_fit_stats, the check stage of the one-call tracking bodies): the model rendered at the
// estimate against the depth the sensor observed, both seen through a se3tn_crop descriptor as 176 x 176 crops (crop_rule.h).
// With m(p) / o(p) the model / observed depth in millimetres at crop pixel p and valid(d) = 100 < d < 2000 (the network's own
// rule: `invalid` in preprocess_kernel, maskA = depthA > 100 of predict.py:247), a pair's record counts
//   model   valid(m)                     seen    valid(m) && valid(o)
//   inlier  seen && |o - m| <= tol       front   seen && o < m - tol       behind  seen && o > m + tol
// and sums |o - m| over the inliers.  All integers: the record does not depend on the order the workgroups arrive in.
//
// One thread per crop pixel, grid = (121, pairs) as the crop kernels.  Six partial counts per thread -> wave64 shuffle reduction
// -> LDS across the four waves -> ONE vector atomic add per counter and workgroup into the pair's uint32 counters (device scope:
// the 121 workgroups of a pair run on several XCDs).  The last of the 121 to arrive (a counter per pair, re-armed by that workgroup,
// as tail_kernel does) reads the sums, stores the finished record once and zeroes the counters for the next launch.
#include "crop_rule.h"

namespace se3tn {

__device__ __forceinline__ bool depth_valid(int d) { return d > 100 && d < 2000; }

__global__ __launch_bounds__(256) void fit_stats_kernel(const FitArgs a) {
  __shared__ unsigned part[4][6];
  __shared__ int last;
  const int i = blockIdx.y, t = threadIdx.x;
  const int p = blockIdx.x * 256 + t;
  unsigned v[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // model, seen, inlier, front, behind, sum |o - m| of the inliers
  if (p < RES * RES) {
    const int y = p / RES, x = p - y * RES;
    const se3tn_crop& cm = a.m[i];
    const se3tn_crop& co = a.o[i];
    size_t q;
    int m = 0, o = 0;
    const bool in_m = crop_source(cm, x, y, q);
    if (in_m) m = cm.depth[q];
    if (a.raw_depth != nullptr) {   // (uniform over the launch)
      uint8_t r = 0, g = 0, b = 0;
      if (in_m) { r = cm.rgb[q * 3]; g = cm.rgb[q * 3 + 1]; b = cm.rgb[q * 3 + 2]; }
      uint8_t* rr = a.raw_rgb + ((size_t)i * RES * RES + p) * 3;
      rr[0] = r; rr[1] = g; rr[2] = b;
      a.raw_depth[(size_t)i * RES * RES + p] = (uint16_t)m;
    }
    if (crop_source(co, x, y, q)) o = co.depth[q];
    if (depth_valid(m)) {
      v[0] = 1u;
      if (depth_valid(o)) {
        const int d = o - m;
        const int ad = d < 0 ? -d : d;
        v[1] = 1u;
        if (ad <= a.tol) { v[2] = 1u; v[5] = (unsigned)ad; }
        else if (d < 0) v[3] = 1u;
        else v[4] = 1u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) part[t >> 6][k] = v[k];
  }
  __syncthreads();
  unsigned* cnt = a.counters + (size_t)i * FitArgs::WORDS;
  if (t < 64) {   // wave 0: lanes 0-5 add one counter each (ONE vector atomic), then lane 0 takes the pair's ticket
    if (t < 6) {
      const unsigned s = part[0][t] + part[1][t] + part[2][t] + part[3][t];
      const unsigned old = __hip_atomic_fetch_add(cnt + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("" ::"v"(old));   // (the returning form: the add has been performed where the other XCDs' adds are)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) {
      last = __hip_atomic_fetch_add(cnt + 6, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
  }
  __syncthreads();
  if (!last) return;                                   // (uniform: `last` is a shared word)
  if (t < FitArgs::WORDS) {                            // the record's eight words, one lane each: stored once, plain vector stores
    unsigned r = 0u;
    if (t < 6) r = __hip_atomic_load(cnt + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (t == 6) r = (unsigned)a.tol;
    reinterpret_cast<unsigned*>(a.out + i)[t] = r;
    if (t < 7) __hip_atomic_store(cnt + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm: sums and ticket
    __threadfence_system();                            // (the record may live in mapped host memory)
  }
}

hipError_t launch_fit_stats(const FitArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > FitArgs::MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_stats_kernel, dim3((RES * RES + 255) / 256, n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace se3tn
