// The crop records of a pose estimate: the model rendered at the estimate against the frame the sensor observed, both seen through a
// se3tn_crop descriptor as 176 x 176 crops (crop_rule.h).
//   depth record   (se3tn_fit_stats, the check stage of the one-call tracking bodies): the counts of fit_rule.h over the crop's
//                  pixels, and the sum of |o - m| over the inliers;
//   colour record  (se3tn_color_stats, the compare stage of se3tn_verify_poses_host; COLOUR): a pixel is COMPARED exactly when it is
//                  an inlier of the depth record; over the compared pixels, per channel c = R, G, B with m_c / o_c the model /
//                  observed byte read at the SAME source index as the depth:  m_c   o_c   m_c^2   o_c^2   m_c o_c   |o_c - m_c|
//   scene rule     (se3tn_color_stats_scene, the compare stage of se3tn_verify_poses_scene_host; COLOUR and SCENE): a third descriptor
//                  per pair shows the composed depth of the tracked objects; a pixel they hide (fit_classify_scene of fit_rule.h) is
//                  model_px and hidden_px and nothing else, so it is no inlier and its colours are not compared.
// 176 * 176 * 255^2 < 2^32: no word overflows.  All integers: the records do not depend on the order the workgroups arrive in.
//
// One thread per crop pixel, grid = (121, pairs) as the crop kernels.  6 (COLOUR: 24, SCENE: 25) partial sums per thread, reduced and
// published by the protocol of record_reduce.h into the pair's counters: wave 0 adds the words, lane 0 takes the pair's ticket, and
// the last of the 121 workgroups stores the finished record(s).
#include "crop_rule.h"
#include "fit_rule.h"
#include "record_reduce.h"

namespace se3tn {

// the kernel arguments of an instantiation: FitArgs, or (SCENE) FitSceneArgs with its third descriptor per pair
template <bool SCENE> struct FitArgsOf { using type = FitArgs; };
template <> struct FitArgsOf<true> { using type = FitSceneArgs; };

template <bool COLOUR, bool SCENE>
__global__ __launch_bounds__(256) void fit_stats_kernel(const typename FitArgsOf<SCENE>::type a) {
  static_assert(COLOUR || !SCENE, "the scene rule is built for the colour records only");
  constexpr int CS = FitArgs::COLOUR_SUMS;                                      // where the colour sums end (and `hidden` stands)
  constexpr int NS = SCENE ? FitSceneArgs::SUMS : COLOUR ? CS : FitArgs::SUMS;
  constexpr int WORDS = COLOUR ? FitArgs::COLOUR_WORDS : FitArgs::WORDS;
  static_assert(NS + 1 <= WORDS, "the sums and the ticket fit the pair's counter words");
  __shared__ unsigned part[4][NS];
  __shared__ int last;
  const int i = blockIdx.y, t = threadIdx.x;
  const int p = blockIdx.x * 256 + t;
  // 0 model, 1 seen, 2 inlier, 3 front, 4 behind, 5 sum |o - m| of the inliers; 6 + 3 k + c: sum k of channel c (k as listed above);
  // 24 (SCENE): hidden
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
    if constexpr (!COLOUR) {
      if (a.raw_depth != nullptr) {   // (uniform over the launch)
        uint8_t r = 0, g = 0, b = 0;
        if (in_m) { r = cm.rgb[qm * 3]; g = cm.rgb[qm * 3 + 1]; b = cm.rgb[qm * 3 + 2]; }
        uint8_t* rr = a.raw_rgb + ((size_t)i * RES * RES + p) * 3;
        rr[0] = r; rr[1] = g; rr[2] = b;
        a.raw_depth[(size_t)i * RES * RES + p] = (uint16_t)m;
      }
    }
    if (crop_source(co, x, y, qo)) o = co.depth[qo];
    unsigned bits;
    if constexpr (SCENE) {   // the third gather, beside the other two and not behind a verdict on them
      const se3tn_crop& cs = a.s[i];
      size_t qs = 0;
      int s = 0;
      if (crop_source(cs, x, y, qs)) s = cs.depth[qs];
      bits = fit_classify_scene(m, o, s, a.tol, v[FC_COUNTS]);
      v[CS] = (bits >> FC_HIDDEN) & 1u;
    } else {
      bits = fit_classify(m, o, a.tol, v[FC_COUNTS]);
    }
#pragma unroll
    for (int k = 0; k < FC_COUNTS; ++k) v[k] = (bits >> k) & 1u;
    if (COLOUR && v[FC_INLIER]) {   // compared: both depths are valid, so both indices lie inside their images
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
  }
  wave_sums_to_lds(v, part);
  __syncthreads();
  unsigned* cnt = a.counters + (size_t)i * WORDS;
  if (t < 64) {   // wave 0: lanes 0 .. NS - 1 add one counter each, then lane 0 takes the pair's ticket
    if (t < NS) counter_add(cnt + t, part[0][t] + part[1][t] + part[2][t] + part[3][t]);
    counters_returned();
    if (t == 0) last = take_ticket(cnt + NS);
  }
  __syncthreads();
  if (!last) return;                                   // (uniform: `last` is a shared word)
  if (t < WORDS) {   // lane t's word -- sum t, tol behind the sums, else 0 -- stored once per record, plain vector stores
    constexpr int SUMS = FitArgs::SUMS;
    const unsigned r = t < NS ? counter_read(cnt + t) : t == NS ? (unsigned)a.tol : 0u;
    // se3tn_fit: sums 0 .. 5 | tol | 0 (SCENE: hidden), from lanes 0 .. 5, NS and NS + 1 (SCENE: CS, the lane of the hidden sum)
    constexpr int LAST = SCENE ? CS : NS + 1;
    if ((!COLOUR || a.fit) && (t < SUMS || t == NS || t == LAST)) reinterpret_cast<unsigned*>(a.fit + i)[t < SUMS ? t : t == NS ? SUMS : SUMS + 1] = r;
    // se3tn_color_fit: px = the inliers (sum 2) | tol | sums 6 .. 23 as words 2 .. 19
    if (COLOUR && (t >= SUMS ? (t < CS || t == NS) : t == FC_INLIER)) reinterpret_cast<unsigned*>(a.colour + i)[t == FC_INLIER ? 0 : t == NS ? 1 : t - 4] = r;
    if (t <= NS) counter_rearm(cnt + t);               // sums and ticket
    __threadfence_system();                            // (the records may live in mapped host memory)
  }
}

hipError_t launch_fit_stats(const FitArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > FitArgs::MAX || (a.colour ? a.raw_depth != nullptr : a.fit == nullptr)) return hipErrorInvalidValue;
  const dim3 grid((RES * RES + 255) / 256, n);
  if (a.colour) hipLaunchKernelGGL((fit_stats_kernel<true, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((fit_stats_kernel<false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fit_stats(const FitSceneArgs& a, int n, hipStream_t st) {
  if (n < 1 || n > FitSceneArgs::MAX || a.colour == nullptr) return hipErrorInvalidValue;
  const dim3 grid((RES * RES + 255) / 256, n);
  hipLaunchKernelGGL((fit_stats_kernel<true, true>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace se3tn
