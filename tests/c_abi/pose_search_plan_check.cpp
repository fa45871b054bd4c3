// Stand-alone host check of csrc/pose_search_plan.h (built with -fsanitize=address,undefined by tests/test_pose_search_host.py): the
// rank key of se3tn_rank_poses and the staging layout of se3tn_search_poses_host.
//   * the order of the keys is the order of the tuples (inliers descending, behind ascending, index ascending) over edge values
//     -- 0, 1, 2^20 - 1, a behind count above the clamp -- and a key gives its inlier count, clamped behind count and index back;
//   * the staging regions [poses | depth | pad | fit | top_fit | idx | pad] are walked over host and device buffers malloc'ed with
//     EXACTLY the planned bytes, the way api.cpp walks them (upload run, launches' pointers, read-back run), for n, frame sizes and
//     k at the edges: an index past the end is a sanitizer report, an overlap is a mismatch.
// Exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>

#include "pose_search_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static int check_keys() {
  const uint32_t M = PS_FIELD_MAX;   // 2^20 - 1
  const uint32_t inl[] = {0u, 1u, 2u, 107u, M - 1, M, M + 1};                      // M + 1 = 2^20: every point of the largest model
  const uint32_t beh[] = {0u, 1u, 2u, M - 1, M, M + 1, 3000000u, 0xffffffffu};     // from M on: the clamp
  const uint32_t idx[] = {0u, 1u, 2u, M - 1, M};
  struct Rec { uint32_t in, be, ix; uint64_t key; };
  std::vector<Rec> all;
  for (uint32_t a : inl)
    for (uint32_t b : beh)
      for (uint32_t i : idx) {
        const uint64_t k = ps_key(a, b, i);
        const uint32_t bc = b > M ? M : b;
        CHECK(ps_key_inliers(k) == a && ps_key_behind(k) == bc && ps_key_index(k) == i);      // the key inverts
        CHECK(k == ((uint64_t)a << 40) + ((uint64_t)(M - bc) << 20) + (uint64_t)(M - i));       // the header's formula
        all.push_back({a, bc, i, k});
      }
  // key order == tuple order, for every pair
  for (const Rec& p : all)
    for (const Rec& q : all) {
      // "p ranks before q": more inliers, then fewer behind, then the lower index
      const bool before = std::make_tuple(-(int64_t)p.in, p.be, p.ix) < std::make_tuple(-(int64_t)q.in, q.be, q.ix);
      CHECK(before == (p.key > q.key));
      CHECK((p.key == q.key) == (p.in == q.in && p.be == q.be && p.ix == q.ix));
    }
  // the largest and the smallest key a call can hold; key + 1 (the kernel's "0 is none") does not wrap
  CHECK(ps_key(M + 1, 0, 0) == ((uint64_t)1 << 60) + ((uint64_t)M << 20) + M);
  CHECK(ps_key(0, M, M) == 0 && ps_key(0, 0xffffffffu, M) == 0);
  CHECK(ps_key(0xffffffffu, 0, 0) == ps_key(M + 1, 0, 0));   // a foreign record: taken as 2^20, no overflow
  CHECK(ps_key(M + 1, 0, 0) + 1 > ps_key(M + 1, 0, 0));
  return 0;
}

static int check_stage(int n, int H, int W, int k) {
  const PsStage s = ps_stage(n, H, W, k);
  const size_t px = (size_t)H * (size_t)W;
  // the regions in order, without gaps beyond the two pads, without overlap
  CHECK(s.poses == 0 && s.depth == (size_t)n * 128 && s.upload_bytes == s.depth + px * 2);
  CHECK(s.fit >= s.upload_bytes && s.fit - s.upload_bytes < 8 && s.fit % 8 == 0 && s.depth % 8 == 0);
  CHECK(s.top_fit == s.fit + (size_t)n * 32 && s.idx == s.top_fit + (size_t)k * 32 && s.top_fit % 8 == 0 && s.idx % 4 == 0);
  CHECK(s.readback_bytes == (size_t)k * 36 && s.top_fit + s.readback_bytes == s.idx + (size_t)k * 4);
  CHECK(s.bytes >= s.idx + (size_t)k * 4 && s.bytes - (s.idx + (size_t)k * 4) < 8 && s.bytes % 8 == 0);
  unsigned char* h = (unsigned char*)std::malloc(s.bytes);
  unsigned char* d = (unsigned char*)std::malloc(s.bytes);
  CHECK(h != nullptr && d != nullptr);
  std::memset(h, 0xee, s.bytes);
  std::memset(d, 0xdd, s.bytes);
  // the caller's arrays into the pinned staging, then the upload run
  std::vector<double> poses((size_t)n * 16, 1.5);
  std::vector<uint16_t> depth(px, 700);
  std::memcpy(h + s.poses, poses.data(), sizeof(double) * 16 * (size_t)n);
  std::memcpy(h + s.depth, depth.data(), sizeof(uint16_t) * px);
  std::memcpy(d, h, s.upload_bytes);
  // what the score launch reads and writes: every pose, every pixel, every record's eight words
  const double* dp = reinterpret_cast<const double*>(d + s.poses);
  const uint16_t* dd = reinterpret_cast<const uint16_t*>(d + s.depth);
  se3tn_point_fit* fit = reinterpret_cast<se3tn_point_fit*>(d + s.fit);
  double sum = 0.0;
  for (size_t i = 0; i < (size_t)n * 16; ++i) sum += dp[i];
  CHECK(sum == 1.5 * 16 * (double)n);
  unsigned long long dsum = 0;
  for (size_t i = 0; i < px; ++i) dsum += dd[i];
  CHECK(dsum == 700ull * px);
  for (int i = 0; i < n; ++i) {
    uint32_t* w = reinterpret_cast<uint32_t*>(fit + i);
    for (int t = 0; t < PS_FIT_WORDS; ++t) w[t] = (uint32_t)i;
  }
  // what the rank launch writes: k records and k indices (here: the last k candidates)
  se3tn_point_fit* top = reinterpret_cast<se3tn_point_fit*>(d + s.top_fit);
  int32_t* idx = reinterpret_cast<int32_t*>(d + s.idx);
  for (int r = 0; r < k; ++r) { top[r] = fit[n - 1 - r]; idx[r] = n - 1 - r; }
  // nothing reached the poses or the frame
  for (size_t i = 0; i < (size_t)n * 16; ++i) CHECK(dp[i] == 1.5);
  for (size_t i = 0; i < px; ++i) CHECK(dd[i] == 700);
  for (int i = 0; i < n; ++i) CHECK(fit[i].points == (uint32_t)i && fit[i]._reserved == (uint32_t)i);
  // the read-back run, then out of the staging
  std::memcpy(h + s.top_fit, d + s.top_fit, s.readback_bytes);
  std::vector<se3tn_point_fit> fit_out((size_t)k);
  std::vector<int32_t> idx_out((size_t)k);
  std::memcpy(fit_out.data(), h + s.top_fit, sizeof(se3tn_point_fit) * (size_t)k);
  std::memcpy(idx_out.data(), h + s.idx, sizeof(int32_t) * (size_t)k);
  for (int r = 0; r < k; ++r) CHECK(idx_out[(size_t)r] == n - 1 - r && fit_out[(size_t)r].inlier_pts == (uint32_t)(n - 1 - r));
  std::free(h);
  std::free(d);
  return 0;
}

int main() {
  static_assert(PS_MAX_POSES == SE3TN_POSE_SEARCH_MAX_POSES && PS_RANK_MAX == SE3TN_POSE_RANK_MAX, "the header's constants");
  static_assert(PS_THREADS == 64 * PS_WAVES && PS_FIT_WORDS * 4 == sizeof(se3tn_point_fit), "geometry");
  if (check_keys()) return 1;
  const int ns[] = {1, 2, 7, 63, 64, 65, 257, 9317, PS_MAX_POSES};
  const int hw[][2] = {{1, 1}, {1, 3}, {3, 1}, {5, 7}, {120, 160}, {480, 640}, {481, 641}};
  for (int n : ns)
    for (const auto& f : hw) {
      if (n == PS_MAX_POSES && f[1] != 1 && f[0] != 481) continue;   // (160 MB per buffer: three frame sizes are enough there)
      const int ks[] = {1, n < 8 ? n : 8, n < PS_RANK_MAX ? n : PS_RANK_MAX};
      for (int k : ks)
        if (check_stage(n, f[0], f[1], k)) { std::fprintf(stderr, "n = %d, H = %d, W = %d, k = %d\n", n, f[0], f[1], k); return 1; }
    }
  // the largest frame the ABI can express, by arithmetic alone: no overflow in the offsets
  const PsStage big = ps_stage(PS_MAX_POSES, 2147483647, 2147483647, PS_RANK_MAX);
  CHECK(big.upload_bytes == (size_t)PS_MAX_POSES * 128 + (size_t)2147483647 * 2147483647 * 2 && big.bytes > big.idx && big.idx > big.fit);
  std::puts("pose_search_plan_check: ok");
  return 0;
}
