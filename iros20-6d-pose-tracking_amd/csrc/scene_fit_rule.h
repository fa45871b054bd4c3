// THE rule of se3tn_scene_stats / se3tn_scene_fit: n depth layers of one frame composed through a shared depth test, and per layer
// the fit record over the pixels where that layer is the nearest one.  Host and device; no HIP header is needed to read it
// (scene_fit.hip compiles these statements into the kernel, tests/c_abi/scene_fit_check.cpp runs them on the host under sanitizers);
// include/se3tracknet.h keeps the public statement, utils.scene_stats the NumPy one.  Integers only: there is no float in here.
//
// Layer i (i < n) is a uint16 millimetre sub-image of the rectangle {x0, y0, x1, y1} of the frame, tightly packed [y1 - y0, x1 - x0];
// x1 <= x0 or y1 <= y0: a layer with no pixels.  For a frame pixel p = (x, y), with o(p) the observed depth:
//     m_i(p)     the layer's value if p is inside its rectangle, else 0
//     valid(d)   100 < d < 2000                                      depth_valid() of fit_rule.h
//     owner(p)   the i with the smallest valid m_i(p), ties to the lowest i; none if no layer is valid at p
//     ids(p)     owner + 1, or 0;        scene(p) = m_owner(p), or 0
// and layer i counts, over the frame,
//     model    valid(m_i)                        visible  model && owner == i           hidden  model && owner != i
//     seen     visible && valid(o)               inlier   seen && |o - m_i| <= tol
//     front    seen && o < m_i - tol             behind   seen && o > m_i + tol
// sums |o - m_i| over its inliers, and sets bit j of hidden_by for every j that owns a pixel where the layer is hidden.
//
// No word overflows: two valid depths differ by at most 1999 - 101 = 1,898, a frame holds at most SCENE_MAX_PIXELS = 2^21 pixels, and
// 2^21 x 1,898 = 3,980,394,496 < 2^32 = 4,294,967,296 (every count is at most 2^21).  A frame with H * W > 2^21 is refused;
// 1920 x 1080 = 2,073,600 fits.  hidden_by is one word and ids one byte: at most SE3TN_SCENE_MAX_OBJECTS = 32 layers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fit_rule.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_SC_HD __host__ __device__
#else
#define SE3TN_SC_HD
#endif

namespace se3tn {

constexpr int SCENE_MAX_LAYERS = 32;                 // == SE3TN_SCENE_MAX_OBJECTS
constexpr unsigned SCENE_MAX_PIXELS = 1u << 21;      // H * W of the largest frame
constexpr unsigned SCENE_MAX_DIFF = 1999u - 101u;    // the largest |o - m| of two valid depths
static_assert((unsigned long long)SCENE_MAX_PIXELS * SCENE_MAX_DIFF < (1ull << 32), "sum_abs_mm cannot overflow");

// what a pixel adds to layer i's counters, in the order the kernel's counter words have
enum SceneCount { SC_MODEL = 0, SC_VISIBLE, SC_SEEN, SC_INLIER, SC_FRONT, SC_BEHIND, SC_COUNTS };

struct SceneLayer {   // one layer as the kernel reads it
  const uint16_t* depth;
  int x0, y0, x1, y1;
};

// m_i(p)
SE3TN_SC_HD inline int scene_layer_at(const SceneLayer& l, int x, int y) {
  if (x < l.x0 || x >= l.x1 || y < l.y0 || y >= l.y1) return 0;
  return (int)l.depth[(size_t)(y - l.y0) * (size_t)(l.x1 - l.x0) + (size_t)(x - l.x0)];
}

// the depth test: layers are offered in ascending i, a later one wins only when strictly nearer (ties to the lowest i).
// owner = -1 and best = 0 before the first offer
SE3TN_SC_HD inline void scene_offer(int i, int m, int& owner, int& best) {
  if (depth_valid(m) && (owner < 0 || m < best)) { owner = i; best = m; }
}

// layer i at a pixel whose owner is known: the bits (1 << SC_*) of the counters the pixel enters, |o - m| of an inlier in `ad` (else 0)
// and the hidden_by bit it sets in `by` (else 0)
SE3TN_SC_HD inline unsigned scene_classify(int i, int m, int owner, int o, int tol, unsigned& ad, unsigned& by) {
  static_assert(SC_MODEL == 0 && SC_VISIBLE == 1 && (int)SC_SEEN == (int)FC_SEEN + 1 && (int)SC_BEHIND == (int)FC_BEHIND + 1,
                "the SC_* bits are the FC_* bits with visible inserted after model");
  ad = 0u; by = 0u;
  if (!depth_valid(m)) return 0u;
  if (owner != i) { by = 1u << owner; return 1u << SC_MODEL; }
  const unsigned f = fit_classify(m, o, tol, ad);   // a visible pixel: exactly se3tn_fit's counts, model set
  return (1u << SC_MODEL) | (1u << SC_VISIBLE) | ((f >> FC_SEEN) << SC_SEEN);
}

}  // namespace se3tn
