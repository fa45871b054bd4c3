// The arithmetic of se3tn_align_poses (include/se3tracknet.h states the rule), host and device: the terms of one model point (which
// pixel it pairs with is the rule of pose_point_rule.h), their quantisation, the 6 x 6 solve and the Cayley update.  pose_align.hip
// runs these statements on the device and
// tests/c_abi/pose_align_check.cpp (and pose_align_scene_check.cpp for the scene-aware rule of se3tn_align_poses_scene) runs the very
// same ones on the host, so the two can be held to each other and to the numpy oracles (tests/pose_align_oracle.py,
// tests/scene_align_oracle.py) word for word.  Whoever includes this compiles with -ffp-contract=off: every operation below is
// rounded once, in the order written.  No HIP header is needed to read it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pose_point_rule.h"
#include "pose_search_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_PA_UNROLL _Pragma("unroll")   // the sums and the 6 x 6 systems stay in registers on the device
#else
#define SE3TN_PA_UNROLL
#endif

namespace se3tn {

constexpr int PA_SUMS = SE3TN_POSE_ALIGN_SUMS;   // 21 words of S_A (i <= j, row-major) | 6 of S_b | S_e
constexpr int PA_B0 = 21, PA_E = 27;
static_assert(PA_SUMS == 28, "21 + 6 + 1");

// fx(v) = (int64) rint(min(max(v, -256), 256) * 2^32); fmax / fmin ignore a NaN, which therefore gives -256 * 2^32
SE3TN_PS_HD inline int64_t pa_fx(double v) { return (int64_t)rint(fmin(fmax(v, -256.0), 256.0) * 4294967296.0); }

// One model point x with normal n under pose T, paired when it faces, its pixel is seen and |d - m| <= gate (millimetres).  Returns
// bit 0: facing, bit 1: paired; with bit 1 set J[6] and r are the point's row of the Jacobian and its residual (metres), otherwise
// they are not written.
//
// The scene-aware rule (SCENE, se3tn_align_poses_scene) puts one verdict in front of `seen`: with s = scene[vf, uf] (read beside d,
// not after the verdict on d: on the device the two gathers travel together) a point that is hidden(s, m, scene_tol) of
// pose_point_rule.h returns bits 0 and 2 and is not paired whatever d is.  The statements are written once for both rules; without
// SCENE `scene` and `scene_tol` are not read.
template <bool SCENE>
SE3TN_PS_HD inline int pa_point_rule(const Rigid& T, const DepthFrame& f, const uint16_t* scene, double scene_tol, double gate, double x,
                                     double y, double z, double nx, double ny, double nz, double J[6], double& r) {
  double qx, qy, qz, mx, my, mz, uf, vf;
  size_t q;
  rotate(T.r, x, y, z, qx, qy, qz);
  const double cx = qx + T.t[0], cy = qy + T.t[1], cz = qz + T.t[2];
  rotate(T.r, nx, ny, nz, mx, my, mz);
  if (!faces(mx, my, mz, cx, cy, cz)) return 0;
  if (!pixel_of(f, cx, cy, cz, uf, vf, q)) return 1;
  const double d = (double)f.depth[q];
  if (SCENE) {
    const double s = (double)scene[q];
    if (hidden(s, model_mm(cz), scene_tol)) return 5;
  }
  if (!(seen(d) && fabs(d - model_mm(cz)) <= gate)) return 1;
  const double oz = d / 1000.0;
  const double ox = ((uf - f.k2) * oz) / f.k0;
  const double oy = ((vf - f.k5) * oz) / f.k4;
  r = (mx * (ox - cx) + my * (oy - cy)) + mz * (oz - cz);
  J[0] = qy * mz - qz * my;
  J[1] = qz * mx - qx * mz;
  J[2] = qx * my - qy * mx;
  J[3] = mx; J[4] = my; J[5] = mz;
  return 3;
}
SE3TN_PS_HD inline int pa_point(const Rigid& T, const DepthFrame& f, double gate, double x, double y, double z, double nx, double ny,
                                double nz, double J[6], double& r) {
  return pa_point_rule<false>(T, f, nullptr, 0.0, gate, x, y, z, nx, ny, nz, J, r);
}
// bit 0: facing, bit 1: paired, bit 2: hidden (never with bit 1)
SE3TN_PS_HD inline int pa_point_scene(const Rigid& T, const DepthFrame& f, const uint16_t* scene, double scene_tol, double gate, double x,
                                      double y, double z, double nx, double ny, double nz, double J[6], double& r) {
  return pa_point_rule<true>(T, f, scene, scene_tol, gate, x, y, z, nx, ny, nz, J, r);
}

// the 28 quantised terms of a paired point added to S
SE3TN_PS_HD inline void pa_accumulate(const double J[6], double r, int64_t S[PA_SUMS]) {
  int w = 0;
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i)
    SE3TN_PA_UNROLL
    for (int j = i; j < 6; ++j) S[w++] += pa_fx(J[i] * J[j]);
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i) S[PA_B0 + i] += pa_fx(J[i] * r);
  S[PA_E] += pa_fx(r * r);
}

// (A + damping * pairs * I) delta = b by LDL^T without pivoting and without a square root; every inner sum starts from 0.0 and adds
// left to right over ascending k.  Returns 0, or 1 (delta not to be used): a pivot that is not > 0 (NaN included) or a component of
// delta that is not finite.
SE3TN_PS_HD inline int pa_solve(const int64_t S[PA_SUMS], uint32_t pairs, double damping, double delta[6]) {
  const double inv = 1.0 / 4294967296.0;
  double A[6][6], b[6], L[6][6], D[6];
  int w = 0;
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i)
    SE3TN_PA_UNROLL
    for (int j = i; j < 6; ++j) { A[i][j] = (double)S[w++] * inv; A[j][i] = A[i][j]; }
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i) b[i] = (double)S[PA_B0 + i] * inv;
  const double lift = damping * (double)pairs;
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lift;
  SE3TN_PA_UNROLL
  for (int j = 0; j < 6; ++j) {
    double s = 0.0;
    SE3TN_PA_UNROLL
    for (int k = 0; k < j; ++k) s = s + (L[j][k] * L[j][k]) * D[k];
    D[j] = A[j][j] - s;
    if (!(D[j] > 0.0)) return 1;
    SE3TN_PA_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      s = 0.0;
      SE3TN_PA_UNROLL
      for (int k = 0; k < j; ++k) s = s + (L[i][k] * L[j][k]) * D[k];
      L[i][j] = (A[j][i] - s) / D[j];
    }
  }
  double y[6];
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
    SE3TN_PA_UNROLL
    for (int k = 0; k < i; ++k) s = s + L[i][k] * y[k];
    y[i] = b[i] - s;
  }
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
  SE3TN_PA_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = 0.0;
    SE3TN_PA_UNROLL
    for (int k = i + 1; k < 6; ++k) s = s + L[k][i] * delta[k];
    delta[i] = y[i] - s;
  }
  SE3TN_PA_UNROLL
  for (int i = 0; i < 6; ++i)
    if (!(fabs(delta[i]) <= 1.7976931348623157e308)) return 1;
  return 0;
}

// R <- C R, t <- t + v with the Cayley rotation of w about the object's origin: a = 0.5 w, s = (a0 a0 + a1 a1) + a2 a2,
// C = ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s) -- orthogonal for every w, no trigonometry
SE3TN_PS_HD inline void pa_update(Rigid& T, const double delta[6]) {
  const double a0 = 0.5 * delta[0], a1 = 0.5 * delta[1], a2 = 0.5 * delta[2];
  const double s = (a0 * a0 + a1 * a1) + a2 * a2;
  const double den = 1.0 + s;
  double C[3][3];
  C[0][0] = ((1.0 - s) + 2.0 * (a0 * a0)) / den;
  C[0][1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;
  C[0][2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  C[1][0] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
  C[1][1] = ((1.0 - s) + 2.0 * (a1 * a1)) / den;
  C[1][2] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  C[2][0] = (2.0 * (a2 * a0) - 2.0 * a1) / den;
  C[2][1] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
  C[2][2] = ((1.0 - s) + 2.0 * (a2 * a2)) / den;
  double R[3][3];
  SE3TN_PA_UNROLL
  for (int i = 0; i < 3; ++i)
    SE3TN_PA_UNROLL
    for (int j = 0; j < 3; ++j) R[i][j] = (C[i][0] * T.r[0][j] + C[i][1] * T.r[1][j]) + C[i][2] * T.r[2][j];
  SE3TN_PA_UNROLL
  for (int i = 0; i < 3; ++i) {
    SE3TN_PA_UNROLL
    for (int j = 0; j < 3; ++j) T.r[i][j] = R[i][j];
    T.t[i] = T.t[i] + delta[3 + i];
  }
}

// max_k |delta_k| <= stop
SE3TN_PS_HD inline bool pa_small(const double delta[6], double stop) {
  double m = fabs(delta[0]);
  SE3TN_PA_UNROLL
  for (int i = 1; i < 6; ++i) m = fabs(delta[i]) > m ? fabs(delta[i]) : m;
  return m <= stop;
}

// What one thread does after the sums of iteration `it` (0-based) are known: the record, the solve, the update.  Returns true when
// the pose is finished (rec.status is then final); rec.iterations / pairs / facing_pts / sum_r2 describe the pose just evaluated.
SE3TN_PS_HD inline bool pa_step(Rigid& T, const int64_t S[PA_SUMS], uint32_t pairs, uint32_t facing, int it,
                                const se3tn_align_params& p, se3tn_align_rec& rec) {
  rec.iterations = (uint32_t)(it + 1);
  rec.pairs = pairs; rec.facing_pts = facing; rec.sum_r2 = S[PA_E];
  if (it == 0) { rec.pairs0 = pairs; rec.sum_r2_0 = S[PA_E]; rec._reserved = 0u; }
  rec.status = SE3TN_ALIGN_ITERS;
  if (pairs < (uint32_t)p.min_pairs) { rec.status = SE3TN_ALIGN_FEW; return true; }
  double delta[6];
  if (pa_solve(S, pairs, p.damping, delta)) { rec.status = SE3TN_ALIGN_SINGULAR; return true; }
  pa_update(T, delta);
  if (pa_small(delta, p.stop)) { rec.status = SE3TN_ALIGN_CONVERGED; return true; }
  return it + 1 >= p.iters;
}

// The scene-aware record: the fields pa_step left, and the hidden points of the pose it last evaluated in the place of _reserved
static_assert(sizeof(se3tn_scene_align_rec) == sizeof(se3tn_align_rec) && offsetof(se3tn_scene_align_rec, hidden_pts) == 28 &&
                  offsetof(se3tn_align_rec, _reserved) == 28 && offsetof(se3tn_scene_align_rec, sum_r2_0) == offsetof(se3tn_align_rec, sum_r2_0),
              "se3tn_scene_align_rec is se3tn_align_rec with the word at offset 28 in use");
SE3TN_PS_HD inline se3tn_scene_align_rec pa_scene_rec(const se3tn_align_rec& rec, uint32_t hidden_pts) {
  se3tn_scene_align_rec s;
  s.iterations = rec.iterations; s.status = rec.status; s.pairs = rec.pairs; s.facing_pts = rec.facing_pts; s.sum_r2 = rec.sum_r2;
  s.pairs0 = rec.pairs0; s.hidden_pts = hidden_pts; s.sum_r2_0 = rec.sum_r2_0;
  return s;
}

}  // namespace se3tn
