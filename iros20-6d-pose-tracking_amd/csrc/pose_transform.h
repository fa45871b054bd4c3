// THE rigid transform of a model point, shared by every float64 kernel that promises bits (pose_errors.hip, and through
// pose_point_rule.h pose_search.hip, pose_grid.hip and pose_align_math.h): one struct, one function, one operation order.  Host and
// device; no HIP header is needed to read it (tests/c_abi/pose_point_rule_check.cpp and pose_align_check.cpp run it on the host).  A
// file that includes this is compiled with -ffp-contract=off (csrc/Makefile): a fused multiply-add formed in one place and not in
// another would give one point two sets of bits.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_PS_HD __host__ __device__
#else
#define SE3TN_PS_HD
#endif

namespace se3tn {

struct Rigid {   // rows 0-2 of a row-major 4 x 4 pose
  double r[3][3], t[3];
};

SE3TN_PS_HD inline Rigid load_pose(const double* p) {
  Rigid T;
  for (int i = 0; i < 3; ++i) {
    T.r[i][0] = p[4 * i]; T.r[i][1] = p[4 * i + 1]; T.r[i][2] = p[4 * i + 2]; T.t[i] = p[4 * i + 3];
  }
  return T;
}

// row i is (r_i0 x + r_i1 y) + r_i2 z, three roundings in this order (no contraction): the part of a transform that depends on
// the rotation alone (pose_grid.hip computes it once per rotation), and the whole of a normal's
SE3TN_PS_HD inline void rotate(const double r[3][3], double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = (r[0][0] * x + r[0][1] * y) + r[0][2] * z;
  oy = (r[1][0] * x + r[1][1] * y) + r[1][2] * z;
  oz = (r[2][0] * x + r[2][1] * y) + r[2][2] * z;
}

// row i is ((r_i0 x + r_i1 y) + r_i2 z) + t_i: rotate(), then the translation -- five roundings in this order
SE3TN_PS_HD inline void transform(const Rigid& T, double x, double y, double z, double& ox, double& oy, double& oz) {
  rotate(T.r, x, y, z, ox, oy, oz);
  ox = ox + T.t[0];
  oy = oy + T.t[1];
  oz = oz + T.t[2];
}

}  // namespace se3tn
