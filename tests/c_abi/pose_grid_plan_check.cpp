// Stand-alone host check of csrc/pose_grid_plan.h (built with -fsanitize=address,undefined by tests/test_pose_grid_host.py): the
// tiling of se3tn_score_pose_grid and the staging layout of se3tn_search_pose_grid_host.
//   * the kernel's loops, walked on the host with the plan's own index functions over the edge sizes of P, n_trans and n_rot: every
//     (rotation, translation, point) triple is visited exactly once, every LDS access of the walk (point planes, counter rows) goes
//     through a buffer malloc'ed with EXACTLY pg_lds_bytes, a translation's row is touched by its owner wave alone, and every
//     record is written once;
//   * the staging regions [rots | trans | depth | pad | fit | top_fit | idx | pad] are ordered, aligned and walked over buffers
//     malloc'ed with exactly the planned bytes, the way api.cpp walks them.
// Exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_grid_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static int check_tiling(int P, int n_trans, int n_rot, int facing) {
  const long long blocks = pg_grid(n_rot, n_trans);
  CHECK(blocks >= 1 && blocks <= (long long)n_rot * n_trans && blocks <= PS_MAX_POSES);
  std::vector<uint8_t> visits((size_t)n_rot * (size_t)n_trans * (size_t)P, 0);
  std::vector<uint8_t> written((size_t)n_rot * (size_t)n_trans, 0);
  const size_t lds_bytes = pg_lds_bytes(facing);
  CHECK(lds_bytes <= 64 * 1024 && 3 * pg_lds_bytes(1) <= 160 * 1024 && 6 * pg_lds_bytes(0) <= 160 * 1024);
  for (long long b = 0; b < blocks; ++b) {
    unsigned char* lds = (unsigned char*)std::malloc(lds_bytes);   // one workgroup's LDS, exactly as planned
    CHECK(lds != nullptr);
    const int r = pg_rot_of((int)b, n_trans), t0 = pg_trans0_of((int)b, n_trans), nt = pg_trans_count(t0, n_trans);
    CHECK(r >= 0 && r < n_rot && t0 >= 0 && t0 < n_trans && nt >= 1 && nt <= PG_TT && t0 + nt <= n_trans);
    CHECK(pg_lds_rows(facing) % 8 == 0);
    uint32_t* rows = reinterpret_cast<uint32_t*>(lds + pg_lds_rows(facing));
    int owner[PG_TT];
    for (int t = 0; t < PG_THREADS; ++t)
      if (t < PG_TT * PG_ROW_WORDS) rows[t] = 0u;
    for (int k = 0; k < PG_TT; ++k) owner[k] = -1;
    int tiles = 0;
    for (int p0 = 0; p0 < P; p0 += PG_PT, ++tiles) {
      const int np = pg_point_count(p0, P);
      CHECK(np >= 1 && np <= PG_PT && p0 + np <= P);
      for (int t = 0; t < PG_THREADS; ++t)   // the rotate pass: plane `pl`, slot j
        for (int j = t; j < np; j += PG_THREADS)
          for (int pl = 0; pl < pg_planes(facing); ++pl) {
            double* plane = reinterpret_cast<double*>(lds + pg_lds_plane(pl));
            plane[j] = (double)(p0 + j);
          }
      for (int wave = 0; wave < PG_WAVES; ++wave)
        for (int k = wave; k < nt; k += PG_WAVES) {
          CHECK(pg_wave_of(k) == wave);
          CHECK(owner[k] == -1 || owner[k] == wave);
          owner[k] = wave;
          uint32_t sum = 0;
          for (int lane = 0; lane < 64; ++lane)
            for (int j = lane; j < np; j += 64) {
              for (int pl = 0; pl < pg_planes(facing); ++pl)
                CHECK(reinterpret_cast<const double*>(lds + pg_lds_plane(pl))[j] == (double)(p0 + j));
              uint8_t& v = visits[(pg_candidate(r, t0 + k, n_trans)) * (size_t)P + (size_t)(p0 + j)];
              CHECK(v == 0);
              v = 1;
              ++sum;
            }
          uint32_t* row = reinterpret_cast<uint32_t*>(lds + pg_lds_row(facing, k));
          CHECK(row == rows + k * PG_ROW_WORDS);
          for (int c = 0; c < PG_ROW_WORDS; ++c) row[c] += sum;
        }
    }
    CHECK(tiles == pg_point_tiles(P));
    for (int t = 0; t < PG_THREADS; ++t)
      if (t < nt * PS_FIT_WORDS) {
        const int k = t / PS_FIT_WORDS, w = t % PS_FIT_WORDS;
        CHECK(k < nt && rows[k * PG_ROW_WORDS + (w < PG_ROW_WORDS ? w : 0)] == (uint32_t)P);
        if (w == 0) {
          const size_t i = pg_candidate(r, t0 + k, n_trans);
          CHECK(i < written.size() && written[i] == 0);
          written[i] = 1;
        }
      }
    std::free(lds);
  }
  for (uint8_t v : visits) CHECK(v == 1);
  for (uint8_t v : written) CHECK(v == 1);
  return 0;
}

static int check_stage(int n_rot, int n_trans, int H, int W, int k) {
  const PgStage s = pg_stage(n_rot, n_trans, H, W, k);
  const size_t n = (size_t)n_rot * (size_t)n_trans, px = (size_t)H * (size_t)W;
  CHECK(s.rots == 0 && s.trans == (size_t)n_rot * 72 && s.depth == s.trans + (size_t)n_trans * 24 && s.upload_bytes == s.depth + px * 2);
  CHECK(s.trans % 8 == 0 && s.depth % 8 == 0);
  CHECK(s.fit >= s.upload_bytes && s.fit - s.upload_bytes < 8 && s.fit % 8 == 0);
  CHECK(s.top_fit == s.fit + n * 32 && s.idx == s.top_fit + (size_t)k * 32 && s.top_fit % 8 == 0 && s.idx % 4 == 0);
  CHECK(s.readback_bytes == (size_t)k * 36 && s.top_fit + s.readback_bytes == s.idx + (size_t)k * 4);
  CHECK(s.bytes >= s.idx + (size_t)k * 4 && s.bytes - (s.idx + (size_t)k * 4) < 8 && s.bytes % 8 == 0);
  unsigned char* h = (unsigned char*)std::malloc(s.bytes);
  unsigned char* d = (unsigned char*)std::malloc(s.bytes);
  CHECK(h != nullptr && d != nullptr);
  std::memset(h, 0xee, s.bytes);
  std::memset(d, 0xdd, s.bytes);
  std::vector<double> rots((size_t)n_rot * 9, 1.5), trans((size_t)n_trans * 3, -2.5);
  std::vector<uint16_t> depth(px, 700);
  std::memcpy(h + s.rots, rots.data(), sizeof(double) * 9 * (size_t)n_rot);
  std::memcpy(h + s.trans, trans.data(), sizeof(double) * 3 * (size_t)n_trans);
  std::memcpy(h + s.depth, depth.data(), sizeof(uint16_t) * px);
  std::memcpy(d, h, s.upload_bytes);
  const double* dr = reinterpret_cast<const double*>(d + s.rots);
  const double* dt = reinterpret_cast<const double*>(d + s.trans);
  const uint16_t* dd = reinterpret_cast<const uint16_t*>(d + s.depth);
  se3tn_point_fit* fit = reinterpret_cast<se3tn_point_fit*>(d + s.fit);
  for (size_t i = 0; i < n; ++i) {
    uint32_t* w = reinterpret_cast<uint32_t*>(fit + i);
    for (int t = 0; t < PS_FIT_WORDS; ++t) w[t] = (uint32_t)i;
  }
  se3tn_point_fit* top = reinterpret_cast<se3tn_point_fit*>(d + s.top_fit);
  int32_t* idx = reinterpret_cast<int32_t*>(d + s.idx);
  for (int r = 0; r < k; ++r) { top[r] = fit[n - 1 - (size_t)r]; idx[r] = (int32_t)(n - 1 - (size_t)r); }
  for (size_t i = 0; i < (size_t)n_rot * 9; ++i) CHECK(dr[i] == 1.5);
  for (size_t i = 0; i < (size_t)n_trans * 3; ++i) CHECK(dt[i] == -2.5);
  for (size_t i = 0; i < px; ++i) CHECK(dd[i] == 700);
  for (size_t i = 0; i < n; ++i) CHECK(fit[i].points == (uint32_t)i && fit[i]._reserved == (uint32_t)i);
  std::memcpy(h + s.top_fit, d + s.top_fit, s.readback_bytes);
  std::vector<se3tn_point_fit> fit_out((size_t)k);
  std::vector<int32_t> idx_out((size_t)k);
  std::memcpy(fit_out.data(), h + s.top_fit, sizeof(se3tn_point_fit) * (size_t)k);
  std::memcpy(idx_out.data(), h + s.idx, sizeof(int32_t) * (size_t)k);
  for (int r = 0; r < k; ++r)
    CHECK(idx_out[(size_t)r] == (int32_t)(n - 1 - (size_t)r) && fit_out[(size_t)r].inlier_pts == (uint32_t)(n - 1 - (size_t)r));
  std::free(h);
  std::free(d);
  return 0;
}

int main() {
  static_assert(PG_THREADS == 64 * PG_WAVES && PG_PT % 64 == 0 && PG_ROW_WORDS == 6, "geometry");
  const int Ps[] = {1, 63, 64, 65, 1023, 1024, 1025, 2049};
  const int nts[] = {1, PG_TT - 1, PG_TT, PG_TT + 1, 3 * PG_TT + 5};
  const int nrs[] = {1, 3};
  for (int P : Ps)
    for (int nt : nts)
      for (int nr : nrs)
        for (int facing = 0; facing < 2; ++facing)
          if (check_tiling(P, nt, nr, facing)) { std::fprintf(stderr, "P = %d, n_trans = %d, n_rot = %d, facing = %d\n", P, nt, nr, facing); return 1; }
  // the grid stays one-dimensional and within the candidate bound at the extremes
  CHECK(pg_grid(PS_MAX_POSES, 1) == PS_MAX_POSES && pg_grid(1, PS_MAX_POSES) == PS_MAX_POSES / PG_TT);
  CHECK(pg_rot_of(PS_MAX_POSES - 1, 1) == PS_MAX_POSES - 1 && pg_trans0_of(PS_MAX_POSES / PG_TT - 1, PS_MAX_POSES) == PS_MAX_POSES - PG_TT);
  const int grids[][2] = {{1, 1}, {1, 17}, {7, 1331}, {240, 281}, {480, 1150}, {PS_MAX_POSES, 1}, {1, PS_MAX_POSES}, {1024, 1024}};
  const int hw[][2] = {{1, 1}, {3, 1}, {5, 7}, {120, 160}, {481, 641}};
  for (const auto& g : grids)
    for (const auto& f : hw) {
      const long long n = (long long)g[0] * g[1];
      if (n == PS_MAX_POSES && f[0] != 1 && f[0] != 481) continue;   // (32 MB of records per buffer: two frame sizes are enough there)
      const int ks[] = {1, n < 8 ? (int)n : 8, n < PS_RANK_MAX ? (int)n : PS_RANK_MAX};
      for (int k : ks)
        if (check_stage(g[0], g[1], f[0], f[1], k)) { std::fprintf(stderr, "n_rot = %d, n_trans = %d, H = %d, W = %d, k = %d\n", g[0], g[1], f[0], f[1], k); return 1; }
    }
  const PgStage big = pg_stage(1024, 1024, 2147483647, 2147483647, PS_RANK_MAX);
  CHECK(big.upload_bytes == (size_t)1024 * 96 + (size_t)2147483647 * 2147483647 * 2 && big.bytes > big.idx && big.idx > big.fit);
  std::puts("pose_grid_plan_check: ok");
  return 0;
}
