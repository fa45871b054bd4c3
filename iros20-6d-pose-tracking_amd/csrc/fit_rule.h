// THE depth rule of a pixel, shared by se3tn_fit_stats / se3tn_color_stats (fit_stats.hip) and se3tn_scene_stats (scene_fit_rule.h
// builds its visible branch from it).  Host and device; no HIP header is needed to read it (tests/c_abi/scene_fit_check.cpp runs it
// on the host under sanitizers); include/se3tracknet.h keeps the public statement, utils.fit_stats the NumPy one.  Integers only.
// With m / o the model / observed depth of the pixel in millimetres:
//     valid(d)  100 < d < 2000        the network's own rule: `invalid` in preprocess_kernel, maskA = depthA > 100 of predict.py:247
//     model   valid(m)                     seen    valid(m) && valid(o)
//     inlier  seen && |o - m| <= tol       front   seen && o < m - tol       behind  seen && o > m + tol
// The scene-aware rule (se3tn_color_stats_scene / se3tn_verify_poses_scene_host) puts one verdict in front of `seen`.  With s the
// scene depth of the pixel -- the composed depth of the tracked objects, what se3tn_scene_fit writes as `scene`, 0 where there is none:
//     hidden  valid(m) && valid(s) && s <= m + tol     a tracked surface at or in front of the pixel: occluded by it, or claimed by it
// A hidden pixel enters model and hidden and nothing else; every other pixel is classified exactly as above.  This is hidden() of
// pose_point_rule.h (the verdict of the scene-aware pose search and alignment on a model POINT) on integers, for a crop PIXEL
// (tests/c_abi/scene_verify_check.cpp runs it on the host under sanitizers; utils.fit_stats(scene=) is the NumPy statement).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_FR_HD __host__ __device__
#else
#define SE3TN_FR_HD
#endif

namespace se3tn {

// the counts a pixel can enter, in the order of se3tn_fit's fields
enum FitCount { FC_MODEL = 0, FC_SEEN, FC_INLIER, FC_FRONT, FC_BEHIND, FC_COUNTS };
// the scene-aware rule's one more count: its bit follows the five above (its word is se3tn_fit's last, where the plain rule leaves 0)
enum { FC_HIDDEN = FC_COUNTS };

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

// hidden by a tracked surface: hidden() of pose_point_rule.h on integers (m < 2000 and tol <= 65535: m + tol cannot overflow)
SE3TN_FR_HD inline bool fit_hidden(int m, int s, int tol) { return depth_valid(m) && depth_valid(s) && s <= m + tol; }

// the scene-aware classifier: the bits of fit_classify plus 1 << FC_HIDDEN; a hidden pixel carries FC_MODEL and FC_HIDDEN only.  With
// s = 0 (no scene) it is fit_classify
SE3TN_FR_HD inline unsigned fit_classify_scene(int m, int o, int s, int tol, unsigned& ad) {
  if (fit_hidden(m, s, tol)) { ad = 0u; return (1u << FC_MODEL) | (1u << FC_HIDDEN); }
  return fit_classify(m, o, tol, ad);
}

}  // namespace se3tn
