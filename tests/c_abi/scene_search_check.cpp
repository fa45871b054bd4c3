// Stand-alone host check of the scene-aware lattice search (built with -ffp-contract=off and -fsanitize=address,undefined by
// tests/test_scene_search_host.py): count_point_scene of csrc/pose_point_rule.h run on the host, and the LDS and staging arithmetic
// csrc/pose_grid_plan.h adds for it.
//   scene_search_check                   the plan alone: the scene rows and the staging of se3tn_search_pose_grid_scene_host.
//   scene_search_check CASE OUT          the plan, then the case: per lattice candidate r * n_trans + t the eight-word record -- rotate()
//                                        once per rotation, + t, faces() with the rotated normal when the case asks for it, then
//                                        count_point_scene(), through rows laid out as the kernel lays them out.
// CASE: int32 {magic 0x5343, P, n_rot, n_trans, H, W, tol_mm, facing}, float64 K[9], points [P,3], normals [P,3], rots [n_rot,9],
// trans [n_trans,3], uint16 depth [H,W], uint16 scene [H,W].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_grid_plan.h"
#include "pose_point_rule.h"

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

// the scene rows: seven words wide, behind the planes where the plain rows start, one LDS buffer of exactly the planned bytes
static int check_rows(int facing) {
  const size_t bytes = pg_scene_lds_bytes(facing);
  CHECK(bytes == pg_lds_bytes(facing) + (size_t)PG_TT * (PG_SCENE_ROW_WORDS - PG_ROW_WORDS) * sizeof(uint32_t));
  CHECK(bytes % 8 == 0 && pg_scene_lds_row(facing, 0) == pg_lds_rows(facing) && pg_row_words(1) == 7 && pg_row_words(0) == PG_ROW_WORDS);
  unsigned char* lds = (unsigned char*)std::malloc(bytes);
  CHECK(lds != nullptr);
  std::memset(lds, 0, bytes);
  for (int k = 0; k < PG_TT; ++k) {
    CHECK(pg_scene_lds_row(facing, k) % sizeof(uint32_t) == 0);
    uint32_t* row = reinterpret_cast<uint32_t*>(lds + pg_scene_lds_row(facing, k));
    for (int c = 0; c < PG_SCENE_ROW_WORDS; ++c) { CHECK(row[c] == 0u); row[c] = (uint32_t)(k * 8 + c + 1); }   // every word once
  }
  CHECK(pg_scene_lds_row(facing, PG_TT - 1) + PG_SCENE_ROW_WORDS * sizeof(uint32_t) == bytes);
  for (size_t b = 0; b < pg_lds_rows(facing); ++b) CHECK(lds[b] == 0);   // the planes were not touched
  std::free(lds);
  // how many workgroups share a CU's 160 KiB: what the header says
  CHECK((160 * 1024) / pg_scene_lds_bytes(0) == 6 && (160 * 1024) / pg_scene_lds_bytes(1) == 3);
  CHECK((160 * 1024) / pg_lds_bytes(0) == 6 && (160 * 1024) / pg_lds_bytes(1) == 3);
  return 0;
}

// the staging: regions ordered, aligned, disjoint; the upload is the head, the read-back one run that holds occ_fit, top_fit and idx
static int check_stage(int n_rot, int n_trans, int H, int W, int k, int n_occ) {
  const PgSceneStage s = pg_scene_stage(n_rot, n_trans, H, W, k, n_occ);
  const PgStage p = pg_stage(n_rot, n_trans, H, W, k);
  const size_t n = (size_t)n_rot * (size_t)n_trans, px = (size_t)H * (size_t)W;
  CHECK(s.rots == p.rots && s.trans == p.trans && s.depth == p.depth && s.upload_bytes == p.upload_bytes);   // the head is the plain call's
  CHECK(s.scene >= s.upload_bytes && s.scene % 8 == 0 && s.fit >= s.scene + px * 2 && s.fit % 8 == 0);
  CHECK(s.occ_fit == s.fit + n * sizeof(se3tn_point_fit) && s.top_fit == s.occ_fit + (size_t)n_occ * PG_OCC_FIT_BYTES);
  CHECK(s.idx == s.top_fit + (size_t)k * sizeof(se3tn_point_fit) && s.bytes >= s.idx + (size_t)k * sizeof(int32_t) && s.bytes % 8 == 0);
  CHECK(s.readback_at == s.occ_fit && s.readback_at + s.readback_bytes == s.idx + (size_t)k * sizeof(int32_t));
  CHECK(s.occ_fit % 8 == 0 && s.top_fit % 8 == 0 && s.idx % 4 == 0);
  // walk it: host and device mirror of exactly s.bytes
  unsigned char* h = (unsigned char*)std::malloc(s.bytes);
  unsigned char* d = (unsigned char*)std::malloc(s.bytes);
  CHECK(h != nullptr && d != nullptr);
  std::memset(h, 0xee, s.bytes);
  std::memset(d, 0xdd, s.bytes);
  std::vector<uint16_t> depth(px, 700);
  std::memcpy(h + s.depth, depth.data(), px * 2);
  std::memcpy(d, h, s.upload_bytes);
  uint16_t* scene = reinterpret_cast<uint16_t*>(d + s.scene);
  for (size_t i = 0; i < px; ++i) scene[i] = 500;
  uint32_t* fit = reinterpret_cast<uint32_t*>(d + s.fit);
  for (size_t i = 0; i < n * PS_FIT_WORDS; ++i) fit[i] = 7u;
  std::memset(d + s.occ_fit, 0x11, (size_t)n_occ * PG_OCC_FIT_BYTES);
  std::memset(d + s.top_fit, 0x22, (size_t)k * sizeof(se3tn_point_fit));
  std::memset(d + s.idx, 0x33, (size_t)k * sizeof(int32_t));
  const uint16_t* dd = reinterpret_cast<const uint16_t*>(d + s.depth);
  for (size_t i = 0; i < px; ++i) CHECK(dd[i] == 700 && scene[i] == 500);
  for (size_t i = 0; i < n * PS_FIT_WORDS; ++i) CHECK(fit[i] == 7u);
  std::memcpy(h + s.readback_at, d + s.readback_at, s.readback_bytes);
  for (size_t b = 0; b < (size_t)n_occ * PG_OCC_FIT_BYTES; ++b) CHECK(h[s.occ_fit + b] == 0x11);
  for (size_t b = 0; b < (size_t)k * sizeof(se3tn_point_fit); ++b) CHECK(h[s.top_fit + b] == 0x22);
  for (size_t b = 0; b < (size_t)k * sizeof(int32_t); ++b) CHECK(h[s.idx + b] == 0x33);
  CHECK(s.readback_at == 0 || h[s.readback_at - 1] != 0x11);   // nothing before the read-back came down
  std::free(h);
  std::free(d);
  return 0;
}

static int check_plan() {
  static_assert(PG_SCENE_ROW_WORDS == PG_ROW_WORDS + 1 && PG_SCENE_HIDDEN == PG_ROW_WORDS && PG_OCC_FIT_BYTES == 48, "the seventh counter");
  static_assert(sizeof(se3tn_scene_point_fit) == sizeof(se3tn_point_fit), "one record size");
  for (int facing = 0; facing < 2; ++facing)
    if (check_rows(facing)) return 1;
  const int grids[][2] = {{1, 1}, {1, 17}, {3, 19}, {7, 1331}, {240, 281}};
  const int hw[][2] = {{1, 1}, {3, 1}, {5, 7}, {24, 32}, {120, 160}, {481, 641}};
  const int occs[] = {1, 2, 31, SE3TN_SCENE_MAX_OBJECTS};
  for (const auto& g : grids)
    for (const auto& f : hw)
      for (int n_occ : occs) {
        const long long n = (long long)g[0] * g[1];
        const int ks[] = {1, n < 8 ? (int)n : 8, n < PS_RANK_MAX ? (int)n : PS_RANK_MAX};
        for (int k : ks)
          if (check_stage(g[0], g[1], f[0], f[1], k, n_occ)) {
            std::fprintf(stderr, "n_rot = %d, n_trans = %d, H = %d, W = %d, k = %d, n_occ = %d\n", g[0], g[1], f[0], f[1], k, n_occ);
            return 1;
          }
      }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 1 && argc != 3) { std::fprintf(stderr, "usage: scene_search_check [CASE OUT]\n"); return 2; }
  if (check_plan()) return 1;
  std::puts("scene_search_check: plan ok");
  if (argc == 1) return 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f != nullptr);
  std::vector<int32_t> hd;
  std::vector<double> K, pts, nrm, rots, trans;
  std::vector<uint16_t> depth, scene;
  CHECK(read_n(f, hd, 8) && hd[0] == 0x5343);
  const int P = hd[1], n_rot = hd[2], n_trans = hd[3], H = hd[4], W = hd[5], tol_mm = hd[6], facing = hd[7];
  CHECK(P >= 1 && n_rot >= 1 && n_trans >= 1 && H >= 1 && W >= 1 && tol_mm >= 1 && (facing == 0 || facing == 1));
  CHECK(read_n(f, K, 9) && read_n(f, pts, (size_t)P * 3) && read_n(f, nrm, (size_t)P * 3));
  CHECK(read_n(f, rots, (size_t)n_rot * 9) && read_n(f, trans, (size_t)n_trans * 3));
  CHECK(read_n(f, depth, (size_t)H * (size_t)W) && read_n(f, scene, (size_t)H * (size_t)W));
  std::fclose(f);
  const double tol = (double)tol_mm;
  const DepthFrame d = depth_frame(depth.data(), H, W, K.data());
  std::vector<uint32_t> out;
  std::vector<double> q((size_t)P * 3), m((size_t)P * 3);   // the rotated points and normals of one rotation
  for (int r = 0; r < n_rot; ++r) {
    const double* sr = rots.data() + (size_t)r * 9;
    const double R[3][3] = {{sr[0], sr[1], sr[2]}, {sr[3], sr[4], sr[5]}, {sr[6], sr[7], sr[8]}};
    for (size_t j = 0; j < (size_t)P; ++j) {
      rotate(R, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], q[3 * j], q[3 * j + 1], q[3 * j + 2]);
      rotate(R, nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2], m[3 * j], m[3 * j + 1], m[3 * j + 2]);
    }
    for (int t = 0; t < n_trans; ++t) {
      const double* tr = trans.data() + (size_t)t * 3;
      unsigned row[PG_SCENE_ROW_WORDS] = {};   // points | in frame, seen, inlier, front, behind | hidden: a row of the kernel
      for (size_t j = 0; j < (size_t)P; ++j) {
        const double cx = q[3 * j] + tr[0], cy = q[3 * j + 1] + tr[1], cz = q[3 * j + 2] + tr[2];
        if (facing && !faces(m[3 * j], m[3 * j + 1], m[3 * j + 2], cx, cy, cz)) continue;
        row[0] += 1u;
        count_point_scene(d, scene.data(), tol, cx, cy, cz, row + 1);
      }
      for (int w = 0; w < 6; ++w) out.push_back(row[w]);   // the record: points | five counters | tol | hidden
      out.push_back((uint32_t)tol_mm);
      out.push_back(row[PG_SCENE_HIDDEN]);
    }
  }
  CHECK(out.size() == (size_t)n_rot * (size_t)n_trans * PS_FIT_WORDS);
  std::FILE* g = std::fopen(argv[2], "wb");
  CHECK(g != nullptr);
  CHECK(std::fwrite(out.data(), sizeof(uint32_t), out.size(), g) == out.size());
  CHECK(std::fclose(g) == 0);
  std::puts("scene_search_check: case done");
  return 0;
}
