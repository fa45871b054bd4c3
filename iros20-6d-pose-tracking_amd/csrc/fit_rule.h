// THE depth rule of a pixel, shared by se3tn_fit_stats / se3tn_color_stats (fit_stats.hip) and se3tn_scene_stats (scene_fit_rule.h
// builds its visible branch from it).  Host and device; no HIP header is needed to read it (tests/c_abi/scene_fit_check.cpp runs it
// on the host under sanitizers); include/se3tracknet.h keeps the public statement, utils.fit_stats the NumPy one.  Integers only.
// With m / o the model / observed depth of the pixel in millimetres:
//     valid(d)  100 < d < 2000        the network's own rule: `invalid` in preprocess_kernel, maskA = depthA > 100 of predict.py:247
//     model   valid(m)                     seen    valid(m) && valid(o)
//     inlier  seen && |o - m| <= tol       front   seen && o < m - tol       behind  seen && o > m + tol
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_FR_HD __host__ __device__
#else
#define SE3TN_FR_HD
#endif

namespace se3tn {

// the counts a pixel can enter, in the order of se3tn_fit's fields
enum FitCount { FC_MODEL = 0, FC_SEEN, FC_INLIER, FC_FRONT, FC_BEHIND, FC_COUNTS };

SE3TN_FR_HD inline bool depth_valid(int d) { return d > 100 && d < 2000; }

// the bits (1 << FC_*) of the counts the pixel enters, and |o - m| of an inlier in `ad` (else 0)
SE3TN_FR_HD inline unsigned fit_classify(int m, int o, int tol, unsigned& ad) {
  ad = 0u;
  if (!depth_valid(m)) return 0u;
  if (!depth_valid(o)) return 1u << FC_MODEL;
  const unsigned seen = (1u << FC_MODEL) | (1u << FC_SEEN);
  const int d = o - m;
  const int a = d < 0 ? -d : d;
  if (a <= tol) { ad = (unsigned)a; return seen | (1u << FC_INLIER); }
  return seen | (d < 0 ? 1u << FC_FRONT : 1u << FC_BEHIND);
}

}  // namespace se3tn
