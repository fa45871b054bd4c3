// Device helpers shared by depth_fill.hip (one launch per step over the frame) and depth_fill_fused.hip (the tiled chain and the
// rectangle pass): border rule of the two blurs, the order-preserving keys of the min / max words, the bilateral table's size.
#pragma once
#include <hip/hip_runtime.h>

namespace se3tn {

struct BilateralTaps { float w[12]; };

// cv::borderInterpolate(p, n, BORDER_REFLECT_101) for the taps of a 5-wide kernel (-2 <= p <= n + 1): one fold at each end, which is
// the rule for every n >= 3; n = 1 ends in the clamp (every tap is pixel 0).  On n = 2 the rule folds p = 3 a second time, to 1,
// where the clamp gives 0: no difference to the blurs, which get an image that is constant along every axis of 3 pixels or fewer
// (every window of the 5 x 5 dilation in front of them holds the whole axis; tests/test_fill_depth_hard_frames_oracle.py).
__device__ __forceinline__ int reflect101(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * n - 2 - p;
  return p < 0 ? 0 : (p >= n ? n - 1 : p);
}

// min / max of the image as order-preserving unsigned keys (any sign), mm[0] = min key, mm[1] = max key
__device__ __forceinline__ unsigned f32_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int BIL_BINS = 1 << 12;

}  // namespace se3tn
