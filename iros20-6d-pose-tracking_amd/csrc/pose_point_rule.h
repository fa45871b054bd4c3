// THE rule of a model point against the observed depth frame, shared by se3tn_score_poses (pose_search.hip), se3tn_score_pose_grid
// (pose_grid.hip) and se3tn_align_poses (pose_align_math.h); include/se3tracknet.h keeps the public statement.  Host and device; no
// HIP header is needed to read it (tests/c_abi/pose_point_rule_check.cpp runs it on the host under sanitizers and holds it to the
// numpy oracles word for word).  Float64, every operation rounded once in the order written: whoever includes this compiles with
// -ffp-contract=off (csrc/Makefile).
//     c = R x + t                                   transform() of pose_transform.h, or rotate() + t where the rotated part is kept
//     facing     n' = rotate(n),  f = (n'x c.x + n'y c.y) + n'z c.z < 0               (where the caller asks for it)
//     in front   c.z > 0
//     uf = rint(c.x * K[0] / c.z + K[2]),  vf = rint(c.y * K[4] / c.z + K[5])          half to even, the rule of track_plan.h
//     in frame   in front && 0 <= uf < W && 0 <= vf < H                                on the doubles: nothing that is not an index is cast
//     d = depth[vf, uf],  m = rint(c.z * 1000.0)
//     seen       in frame && 100 < d < 2000
//     inlier |d - m| <= tol      front d < m - tol      behind d > m + tol             (of the seen ones; exact: integers in doubles)
// count_point_scene (below, se3tn_score_pose_grid_scene) and pa_point_scene (pose_align_math.h, se3tn_align_poses_scene) put one verdict
// in front of `seen`: hidden by a tracked surface -- hidden() below, stated once for both.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pose_transform.h"

namespace se3tn {

struct DepthFrame {   // the observed frame and the camera
  const uint16_t* depth;   // [H,W] millimetres
  int H, W;
  double k0, k2, k4, k5;   // K[0], K[2], K[4], K[5]
};
SE3TN_PS_HD inline DepthFrame depth_frame(const uint16_t* depth, int H, int W, const double K[9]) {
  DepthFrame f;
  f.depth = depth; f.H = H; f.W = W;
  f.k0 = K[0]; f.k2 = K[2]; f.k4 = K[4]; f.k5 = K[5];
  return f;
}

// the rotated normal (nx, ny, nz) of a point at c faces the camera: false when turned away, grazing (f == 0) or NaN
SE3TN_PS_HD inline bool faces(double nx, double ny, double nz, double cx, double cy, double cz) {
  const double f = (nx * cx + ny * cy) + nz * cz;
  return f < 0.0;
}

SE3TN_PS_HD inline double project(double c, double k, double cz, double k0) { return rint(c * k / cz + k0); }

// The pixel of the camera-space point c: false when it is not in frame; otherwise (uf, vf) are its column and row and q its index
// into depth.  Every comparison is false for NaN; +-inf and anything beyond the frame fail one of them: only an index reaches the cast.
SE3TN_PS_HD inline bool pixel_of(const DepthFrame& f, double cx, double cy, double cz, double& uf, double& vf, size_t& q) {
  uf = project(cx, f.k0, cz, f.k2);
  vf = project(cy, f.k4, cz, f.k5);
  if (!(cz > 0.0 && uf >= 0.0 && uf < (double)f.W && vf >= 0.0 && vf < (double)f.H)) return false;
  q = (size_t)(int)vf * (size_t)f.W + (size_t)(int)uf;
  return true;
}

SE3TN_PS_HD inline bool seen(double d) { return d > 100.0 && d < 2000.0; }       // a depth the sensor measured, millimetres
SE3TN_PS_HD inline double model_mm(double cz) { return rint(cz * 1000.0); }       // m: the model's depth at the point

// the hidden verdict of the scene-aware rules on an in-frame point: s = scene[vf, uf], m = model_mm(c.z), tol in millimetres --
// a tracked surface the sensor could have measured, at or in front of the point.  fit_hidden() of fit_rule.h is the same verdict on
// integers, for a crop pixel (se3tn_color_stats_scene)
SE3TN_PS_HD inline bool hidden(double s, double m, double tol) { return seen(s) && s <= m + tol; }

// the point c added to the five counters v: in frame, seen, inlier, front, behind
SE3TN_PS_HD inline void count_point(const DepthFrame& f, double tol, double cx, double cy, double cz, unsigned v[5]) {
  double uf, vf;
  size_t q;
  if (!pixel_of(f, cx, cy, cz, uf, vf, q)) return;
  v[0] += 1u;
  const double d = (double)f.depth[q];
  if (!seen(d)) return;
  const double m = model_mm(cz);
  v[1] += 1u;
  if (fabs(d - m) <= tol) v[2] += 1u;
  if (d < m - tol) v[3] += 1u;
  if (d > m + tol) v[4] += 1u;
}

// The scene-aware rule (se3tn_score_pose_grid_scene): `scene` [H,W] is the composed depth of the tracked objects in millimetres, 0
// where there is none.
//     s = scene[vf, uf]
//     hidden     in frame && 100 < s < 2000 && s <= m + tol       a tracked surface at or in front of the point: occluded by it, or
//                                                                 claimed by it.  The point enters hidden and nothing else past in frame
//     otherwise  d = depth[vf, uf]; seen, inlier, front, behind exactly as count_point
// the point c added to the six counters v: in frame, seen, inlier, front, behind, hidden
SE3TN_PS_HD inline void count_point_scene(const DepthFrame& f, const uint16_t* scene, double tol, double cx, double cy, double cz,
                                          unsigned v[6]) {
  double uf, vf;
  size_t q;
  if (!pixel_of(f, cx, cy, cz, uf, vf, q)) return;
  v[0] += 1u;
  const double s = (double)scene[q];
  const double d = (double)f.depth[q];   // (read beside s, not after the verdict on it: on the device the two gathers travel together)
  const double m = model_mm(cz);
  // every counter is added to by name, without a branch that picks one: the device keeps the seven sums in registers only then
  const bool hid = hidden(s, m, tol);
  const bool sn = !hid && seen(d);
  v[5] += hid ? 1u : 0u;
  v[1] += sn ? 1u : 0u;
  v[2] += (sn && fabs(d - m) <= tol) ? 1u : 0u;
  v[3] += (sn && d < m - tol) ? 1u : 0u;
  v[4] += (sn && d > m + tol) ? 1u : 0u;
}

}  // namespace se3tn
