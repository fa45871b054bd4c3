// THE rigid transform of a model point, shared by every float64 kernel that promises bits (pose_errors.hip, pose_search.hip): one
// function, one operation order.  A file that includes this is compiled with -ffp-contract=off (csrc/Makefile): a fused multiply-add
// formed in one place and not in another would give one point two sets of bits.  (pose_grid.hip states the same five roundings cut
// after the third: the rotated part once per rotation, the translation added per candidate.)
#pragma once
#include <hip/hip_runtime.h>

namespace se3tn {

struct Rigid {   // rows 0-2 of a row-major 4 x 4 pose
  double r[3][3], t[3];
};

__device__ __forceinline__ Rigid load_pose(const double* p) {
  Rigid T;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T.r[i][0] = p[4 * i]; T.r[i][1] = p[4 * i + 1]; T.r[i][2] = p[4 * i + 2]; T.t[i] = p[4 * i + 3];
  }
  return T;
}

// row i is ((r_i0 x + r_i1 y) + r_i2 z) + t_i, five roundings in this order (no contraction)
__device__ __forceinline__ void transform(const Rigid& T, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = ((T.r[0][0] * x + T.r[0][1] * y) + T.r[0][2] * z) + T.t[0];
  oy = ((T.r[1][0] * x + T.r[1][1] * y) + T.r[1][2] * z) + T.t[1];
  oz = ((T.r[2][0] * x + T.r[2][1] * y) + T.r[2][2] * z) + T.t[2];
}

}  // namespace se3tn
