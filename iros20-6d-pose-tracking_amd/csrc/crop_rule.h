// crop_bbox's index rule (Utils.py:320-359), stated once for device code: which pixel of a se3tn_crop's image the crop pixel
// (x, y) of the 176 x 176 crop shows.  cv2.resize(INTER_NEAREST) (OpenCV resizeNN):
//   sx = min(floor(x * (1.0 / ((double)dst / src))), src - 1)      evaluated in float64,
// and the crop canvas is zero outside the image (Utils.py:327-342): false = that zero.  The same arithmetic, operation by
// operation, as preprocess_kernel / crop_raw_kernel (kernels_misc.hip), which keep their own copy.
#pragma once
#include "se3tn_internal.h"

namespace se3tn {

__device__ __forceinline__ bool crop_source(const se3tn_crop& c, int x, int y, size_t& q) {
  const int cw = c.right - c.left, chh = c.bottom - c.top;
  const double ifx = 1.0 / ((double)RES / (double)cw);
  const double ify = 1.0 / ((double)RES / (double)chh);
  int sx = (int)floor((double)x * ifx); sx = sx < cw - 1 ? sx : cw - 1;
  int sy = (int)floor((double)y * ify); sy = sy < chh - 1 ? sy : chh - 1;
  const int fx = c.left + sx, fy = c.top + sy;
  if ((unsigned)fx >= (unsigned)c.W || (unsigned)fy >= (unsigned)c.H) return false;
  q = (size_t)fy * c.W + fx;
  return true;
}

}  // namespace se3tn
