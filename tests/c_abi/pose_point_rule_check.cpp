// Stand-alone host check of csrc/pose_point_rule.h and csrc/pose_transform.h (built with -ffp-contract=off and
// -fsanitize=address,undefined by tests/test_pose_point_rule_host.py): the statements pose_search.hip and pose_grid.hip run per
// point, run on the host.
//   pose_point_rule_check CASE OUT       reads a case and writes, per depth frame, the eight-word record of every pose -- transform(),
//                                        then count_point(), as pose_score_kernel does -- and then of every lattice candidate
//                                        r * n_trans + t -- rotate() once per rotation, + t, faces() with the rotated normal when the
//                                        case asks for it, then count_point(), as pose_grid_kernel does.
// CASE: int32 {magic 0x5052, P, n_poses, n_rot, n_trans, frames, H, W, tol_mm, facing}, float64 K[9], points [P,3], normals [P,3],
// poses [n_poses,16], rots [n_rot,9], trans [n_trans,3], uint16 depth [frames,H,W].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pose_point_rule.h"
#include "pose_search_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// points | in frame, seen, inlier, front, behind | tol | 0
static void put_record(std::vector<uint32_t>& out, uint32_t points, const unsigned v[5], int tol) {
  out.push_back(points);
  for (int k = 0; k < 5; ++k) out.push_back(v[k]);
  out.push_back((uint32_t)tol);
  out.push_back(0u);
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: pose_point_rule_check CASE OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f != nullptr);
  std::vector<int32_t> hd;
  std::vector<double> K, pts, nrm, poses, rots, trans;
  std::vector<uint16_t> depth;
  CHECK(read_n(f, hd, 10) && hd[0] == 0x5052);
  const int P = hd[1], n_poses = hd[2], n_rot = hd[3], n_trans = hd[4], frames = hd[5], H = hd[6], W = hd[7], tol_mm = hd[8], facing = hd[9];
  CHECK(P >= 1 && n_poses >= 0 && n_rot >= 0 && n_trans >= 0 && frames >= 1 && H >= 1 && W >= 1 && tol_mm >= 1 && (facing == 0 || facing == 1));
  CHECK(read_n(f, K, 9) && read_n(f, pts, (size_t)P * 3) && read_n(f, nrm, (size_t)P * 3) && read_n(f, poses, (size_t)n_poses * 16));
  CHECK(read_n(f, rots, (size_t)n_rot * 9) && read_n(f, trans, (size_t)n_trans * 3));
  CHECK(read_n(f, depth, (size_t)frames * (size_t)H * (size_t)W));
  std::fclose(f);
  const double tol = (double)tol_mm;
  std::vector<uint32_t> out;
  std::vector<double> q((size_t)P * 3), m((size_t)P * 3);   // the rotated points and normals of one rotation
  for (int fr = 0; fr < frames; ++fr) {
    const DepthFrame d = depth_frame(depth.data() + (size_t)fr * (size_t)H * (size_t)W, H, W, K.data());
    for (int i = 0; i < n_poses; ++i) {
      const Rigid T = load_pose(poses.data() + (size_t)i * 16);
      unsigned v[5] = {0u, 0u, 0u, 0u, 0u};
      for (int j = 0; j < P; ++j) {
        double cx, cy, cz;
        transform(T, pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2], cx, cy, cz);
        count_point(d, tol, cx, cy, cz, v);
      }
      put_record(out, (uint32_t)P, v, tol_mm);
    }
    for (int r = 0; r < n_rot; ++r) {
      const double* sr = rots.data() + (size_t)r * 9;
      const double R[3][3] = {{sr[0], sr[1], sr[2]}, {sr[3], sr[4], sr[5]}, {sr[6], sr[7], sr[8]}};
      for (size_t j = 0; j < (size_t)P; ++j) {
        rotate(R, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], q[3 * j], q[3 * j + 1], q[3 * j + 2]);
        rotate(R, nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2], m[3 * j], m[3 * j + 1], m[3 * j + 2]);
      }
      for (int t = 0; t < n_trans; ++t) {
        const double* tr = trans.data() + (size_t)t * 3;
        unsigned v[5] = {0u, 0u, 0u, 0u, 0u};
        uint32_t points = 0;
        for (size_t j = 0; j < (size_t)P; ++j) {
          const double cx = q[3 * j] + tr[0], cy = q[3 * j + 1] + tr[1], cz = q[3 * j + 2] + tr[2];
          if (facing && !faces(m[3 * j], m[3 * j + 1], m[3 * j + 2], cx, cy, cz)) continue;
          points += 1;
          count_point(d, tol, cx, cy, cz, v);
        }
        put_record(out, points, v, tol_mm);
      }
    }
  }
  CHECK(out.size() == (size_t)frames * ((size_t)n_poses + (size_t)n_rot * (size_t)n_trans) * PS_FIT_WORDS);
  std::FILE* g = std::fopen(argv[2], "wb");
  CHECK(g != nullptr);
  CHECK(std::fwrite(out.data(), sizeof(uint32_t), out.size(), g) == out.size());
  CHECK(std::fclose(g) == 0);
  std::puts("pose_point_rule_check: case done");
  return 0;
}
