// Depth AND colour record of a pose hypothesis (se3tn_color_stats, the compare stage of se3tn_verify_poses_host): the model rendered
// at the hypothesis against the frame the sensor observed, both seen through a se3tn_crop descriptor as 176 x 176 crops (crop_rule.h).
// The depth part is fit_stats.hip's record, bit for bit (the same loads, the same rule).  A crop pixel is COMPARED exactly when it is
// an inlier of that record: valid(m) && valid(o) && |o - m| <= tol; over the compared pixels the colour record sums, per channel
// c = R, G, B with m_c / o_c the model / observed byte read at the SAME source index as the depth,
//   m_c   o_c   m_c^2   o_c^2   m_c o_c   |o_c - m_c|
// 176 * 176 * 255^2 < 2^32: no word overflows.  All integers: the records do not depend on the order the workgroups arrive in.
//
// The shape of fit_stats_kernel: one thread per crop pixel, grid = (121, pairs).  24 partial sums per thread -> wave64 shuffle
// reduction -> LDS across the four waves -> ONE vector atomic add per sum and workgroup into the pair's uint32 counters (device scope:
// the 121 workgroups of a pair run on several XCDs; every access to a counter is an agent-scope atomic, so no L1 holds a stale copy).
// The last of the 121 to arrive (a ticket per pair) reads the sums, stores both finished records once with plain vector stores and
// zeroes the counters for the next launch.
#include "crop_rule.h"

namespace se3tn {

namespace {
constexpr int NS = ColorFitArgs::SUMS;
__device__ __forceinline__ bool depth_ok(int d) { return d > 100 && d < 2000; }
}  // namespace

__global__ __launch_bounds__(256) void color_fit_kernel(const ColorFitArgs a) {
  __shared__ unsigned part[4][NS];
  __shared__ int last;
  const int i = blockIdx.y, t = threadIdx.x;
  const int p = blockIdx.x * 256 + t;
  // 0 model, 1 seen, 2 inlier, 3 front, 4 behind, 5 sum |o - m| of the inliers; 6 + 3 k + c: sum k of channel c (k as listed above)
  unsigned v[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0u;
  if (p < RES * RES) {
    const int y = p / RES, x = p - y * RES;
    const se3tn_crop& cm = a.m[i];
    const se3tn_crop& co = a.o[i];
    size_t qm = 0, qo = 0;
    int m = 0, o = 0;
    const bool in_m = crop_source(cm, x, y, qm);
    if (in_m) m = cm.depth[qm];
    const bool in_o = crop_source(co, x, y, qo);
    if (in_o) o = co.depth[qo];
    if (depth_ok(m)) {
      v[0] = 1u;
      if (depth_ok(o)) {
        const int d = o - m;
        const int ad = d < 0 ? -d : d;
        v[1] = 1u;
        if (ad <= a.tol) {   // compared: both depths are valid, so both indices lie inside their images
          v[2] = 1u; v[5] = (unsigned)ad;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int mc = cm.rgb[qm * 3 + c], oc = co.rgb[qo * 3 + c];
            const int dc = oc - mc;
            v[6 + c] = (unsigned)mc;
            v[9 + c] = (unsigned)oc;
            v[12 + c] = (unsigned)(mc * mc);
            v[15 + c] = (unsigned)(oc * oc);
            v[18 + c] = (unsigned)(mc * oc);
            v[21 + c] = (unsigned)(dc < 0 ? -dc : dc);
          }
        }
        else if (d < 0) v[3] = 1u;
        else v[4] = 1u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) part[t >> 6][k] = v[k];
  }
  __syncthreads();
  unsigned* cnt = a.counters + (size_t)i * ColorFitArgs::WORDS;
  if (t < 64) {   // wave 0: lanes 0-23 add one counter each (ONE vector atomic), then lane 0 takes the pair's ticket
    if (t < NS) {
      const unsigned s = part[0][t] + part[1][t] + part[2][t] + part[3][t];
      const unsigned old = __hip_atomic_fetch_add(cnt + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("" ::"v"(old));   // (the returning form: the add has been performed where the other XCDs' adds are)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) {
      last = __hip_atomic_fetch_add(cnt + NS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
  }
  __syncthreads();
  if (!last) return;                                   // (uniform: `last` is a shared word)
  if (t < 32) {                                        // one lane per sum: every record word stored once, plain vector stores
    unsigned* fit = reinterpret_cast<unsigned*>(a.fit_out ? a.fit_out + i : nullptr);
    unsigned* col = reinterpret_cast<unsigned*>(a.out + i);
    if (t < NS) {
      const unsigned r = __hip_atomic_load(cnt + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t < 6) { if (fit) fit[t] = r; }
      else col[t - 4] = r;                             // sums 6 .. 23 -> words 2 .. 19
      if (t == 2) col[0] = r;                          // px = the inliers
    } else if (t == NS) {
      if (fit) fit[6] = (unsigned)a.tol;
      col[1] = (unsigned)a.tol;
    } else if (t == NS + 1) {
      if (fit) fit[7] = 0u;
    }
    if (t <= NS) __hip_atomic_store(cnt + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm: sums and ticket
    __threadfence_system();                            // (the records may live in mapped host memory)
  }
}

hipError_t launch_color_fit(const ColorFitArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > ColorFitArgs::MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(color_fit_kernel, dim3((RES * RES + 255) / 256, n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace se3tn
