// Stand-alone host check of the scene-aware alignment's statements in csrc/pose_point_rule.h, csrc/pose_align_math.h and
// csrc/pose_align_plan.h (built with -ffp-contract=off and -fsanitize=address,undefined by tests/test_scene_align_host.py): what the
// <SCENE> instantiation of the kernel runs, run on the host.
//   pose_align_scene_check               the plan and the predicate alone: hidden() on every edge of its three comparisons, the
//                                        31-word rows beside the 30-word ones, and pa_stage_scene's regions ordered, aligned and
//                                        walked over buffers of exactly the planned bytes;
//   pose_align_scene_check CASE OUT      reads a case, aligns every pose with pa_point_scene -- walking the points in the kernel's
//                                        order: thread by thread, each thread's own partial sums and three counts, then the waves'
//                                        31-word rows -- and writes [poses n x 16 doubles | records n x 40 bytes | sums n x 28 int64].
// CASE: int32 {magic 0x5053, P, n, H, W, gate_mm, iters, min_pairs, scene_tol_mm}, float64 {damping, stop, K[9]}, float64 points [P,3],
// normals [P,3], poses [n,16], uint16 depth [H,W], uint16 scene [H,W].  Exits non-zero at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_align_math.h"
#include "pose_align_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static int check_hidden() {
  // 100 < s < 2000 && s <= m + tol, on doubles
  CHECK(!hidden(0.0, 500.0, 10.0) && !hidden(100.0, 500.0, 10.0) && hidden(101.0, 500.0, 10.0));
  CHECK(hidden(510.0, 500.0, 10.0) && !hidden(511.0, 500.0, 10.0));
  CHECK(hidden(1999.0, 1990.0, 10.0) && !hidden(2000.0, 1990.0, 10.0) && !hidden(2000.0, 3000.0, 10.0));
  CHECK(!hidden(500.0, NAN, 10.0) && !hidden(65535.0, 70000.0, 10.0));
  // count_point_scene reads the same verdict: one in-frame point, a scene pixel on either side of m + tol
  const double K[9] = {10.0, 0.0, 0.5, 0.0, 10.0, 0.5, 0.0, 0.0, 1.0};
  uint16_t depth[1] = {500}, scene[1] = {510};
  const DepthFrame f = depth_frame(depth, 1, 1, K);
  unsigned v[6] = {0, 0, 0, 0, 0, 0};
  count_point_scene(f, scene, 10.0, 0.0, 0.0, 0.5, v);
  CHECK(v[0] == 1 && v[5] == 1 && v[1] == 0);
  scene[0] = 511;
  count_point_scene(f, scene, 10.0, 0.0, 0.0, 0.5, v);
  CHECK(v[0] == 2 && v[5] == 1 && v[1] == 1 && v[2] == 1);
  // pa_point_scene on the same pixel: hidden returns bits 0 and 2 whatever d is; not hidden goes on as pa_point
  Rigid T;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T.r[i][j] = i == j ? 1.0 : 0.0;
  T.t[0] = 0.0; T.t[1] = 0.0; T.t[2] = 0.5;
  double J[6], r = 0.0, J0[6], r0 = 0.0;
  scene[0] = 510;
  CHECK(pa_point_scene(T, f, scene, 10.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, J, r) == 5);
  depth[0] = 0;
  CHECK(pa_point_scene(T, f, scene, 10.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, J, r) == 5);
  depth[0] = 503;
  scene[0] = 511;
  CHECK(pa_point_scene(T, f, scene, 10.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, J, r) == 3);
  CHECK(pa_point(T, f, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, J0, r0) == 3 && std::memcmp(J, J0, sizeof(J)) == 0 && std::memcmp(&r, &r0, 8) == 0);
  CHECK(pa_point_scene(T, f, scene, 10.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, J, r) == 0);   // turned away: not facing, the scene not asked
  return 0;
}

static int check_lds() {
  CHECK(PA_SCENE_ROW_WORDS == PA_SUMS + 3 && PA_W_HIDDEN == PA_SUMS + 2 && PA_W_HIDDEN == PA_W_FACING + 1 && PA_W_FACING == PA_W_PAIRS + 1);
  CHECK(pa_row_words(0) == PA_ROW_WORDS && pa_row_words(1) == PA_SCENE_ROW_WORDS);
  long long* red = (long long*)std::malloc(sizeof(long long) * (size_t)pa_scene_lds_words());   // exactly as the kernel declares it
  CHECK(red != nullptr);
  for (int w = 0; w < PA_WAVES; ++w) {
    CHECK(pa_scene_lds_row(w) == w * PA_SCENE_ROW_WORDS && pa_scene_lds_row(w) + PA_SCENE_ROW_WORDS <= pa_scene_lds_total());
    for (int k = 0; k < PA_SCENE_ROW_WORDS; ++k) red[pa_scene_lds_row(w) + k] = (long long)(w + 1) * 1000 + k;
  }
  CHECK(pa_scene_lds_total() + PA_SCENE_ROW_WORDS == pa_scene_lds_words());
  for (int t = 0; t < PA_THREADS; ++t)
    if (t < PA_SCENE_ROW_WORDS) {
      long long s = 0;
      for (int w = 0; w < PA_WAVES; ++w) s += red[pa_scene_lds_row(w) + t];
      red[pa_scene_lds_total() + t] = s;
    }
  for (int k = 0; k < PA_SCENE_ROW_WORDS; ++k)
    CHECK(red[pa_scene_lds_total() + k] == (long long)PA_WAVES * (PA_WAVES + 1) / 2 * 1000 + (long long)PA_WAVES * k);
  std::free(red);
  return 0;
}

static int check_stage(int n, int H, int W, int with_sums) {
  const PaSceneStage s = pa_stage_scene(n, H, W, with_sums);
  const PaStage plain = pa_stage(n, H, W, with_sums);
  const size_t px = (size_t)H * (size_t)W;
  CHECK(s.poses == 0 && s.depth == (size_t)n * 128 && s.depth == plain.depth);
  CHECK(s.scene >= s.depth + px * 2 && s.scene - (s.depth + px * 2) < 8 && s.scene % 8 == 0 && s.scene == plain.poses_out);
  CHECK(s.upload_bytes == s.scene + px * 2);
  CHECK(s.poses_out >= s.upload_bytes && s.poses_out - s.upload_bytes < 8 && s.poses_out % 8 == 0);
  CHECK(s.rec == s.poses_out + (size_t)n * 128 && s.sums == s.rec + (size_t)n * 40 && s.rec % 8 == 0 && s.sums % 8 == 0);
  CHECK(s.bytes == s.sums + (size_t)n * 224);
  CHECK(s.readback_bytes == (size_t)n * (168 + (with_sums ? 224 : 0)) && s.poses_out + s.readback_bytes <= s.bytes);
  unsigned char* h = (unsigned char*)std::malloc(s.bytes);
  unsigned char* d = (unsigned char*)std::malloc(s.bytes);
  CHECK(h != nullptr && d != nullptr);
  std::memset(h, 0xee, s.bytes);
  std::memset(d, 0xdd, s.bytes);
  std::vector<double> poses((size_t)n * 16, 1.5);
  std::vector<uint16_t> depth(px, 700), scene(px, 650);
  std::memcpy(h + s.poses, poses.data(), sizeof(double) * 16 * (size_t)n);
  std::memcpy(h + s.depth, depth.data(), sizeof(uint16_t) * px);
  std::memcpy(h + s.scene, scene.data(), sizeof(uint16_t) * px);
  std::memcpy(d, h, s.upload_bytes);
  double* po = reinterpret_cast<double*>(d + s.poses_out);
  se3tn_scene_align_rec* rec = reinterpret_cast<se3tn_scene_align_rec*>(d + s.rec);
  int64_t* sums = reinterpret_cast<int64_t*>(d + s.sums);
  for (size_t i = 0; i < (size_t)n; ++i) {
    for (int k = 0; k < 16; ++k) po[i * 16 + (size_t)k] = reinterpret_cast<const double*>(d + s.poses)[i * 16 + (size_t)k] + (double)i;
    rec[i].hidden_pts = (uint32_t)i; rec[i].sum_r2_0 = -(int64_t)i;
    for (int k = 0; k < PA_SUMS; ++k) sums[i * PA_SUMS + (size_t)k] = (int64_t)i * 100 + k;
  }
  for (size_t i = 0; i < px; ++i) {
    CHECK(reinterpret_cast<const uint16_t*>(d + s.depth)[i] == 700);
    CHECK(reinterpret_cast<const uint16_t*>(d + s.scene)[i] == 650);
  }
  std::memcpy(h + s.poses_out, d + s.poses_out, s.readback_bytes);
  for (size_t i = 0; i < (size_t)n; ++i) {
    CHECK(reinterpret_cast<const double*>(h + s.poses_out)[i * 16 + 15] == 1.5 + (double)i);
    CHECK(reinterpret_cast<const se3tn_scene_align_rec*>(h + s.rec)[i].hidden_pts == (uint32_t)i);
    CHECK(reinterpret_cast<const se3tn_scene_align_rec*>(h + s.rec)[i].sum_r2_0 == -(int64_t)i);
    if (with_sums) CHECK(reinterpret_cast<const int64_t*>(h + s.sums)[i * PA_SUMS + 27] == (int64_t)i * 100 + 27);
  }
  std::free(h);
  std::free(d);
  return 0;
}

static int check_plan() {
  if (check_hidden() || check_lds()) return 1;
  const int ns[] = {1, 2, 7, 65, PA_MAX_POSES};
  const int hw[][2] = {{1, 1}, {3, 1}, {5, 7}, {120, 160}, {481, 641}};
  for (int n : ns)
    for (const auto& f : hw)
      for (int ws = 0; ws < 2; ++ws)
        if (check_stage(n, f[0], f[1], ws)) { std::fprintf(stderr, "n = %d, H = %d, W = %d, sums = %d\n", n, f[0], f[1], ws); return 1; }
  // the record: the fields of se3tn_align_rec, the word at offset 28 in use
  se3tn_align_rec a;
  a.iterations = 3; a.status = SE3TN_ALIGN_CONVERGED; a.pairs = 40; a.facing_pts = 140; a.sum_r2 = -5; a.pairs0 = 38; a._reserved = 0; a.sum_r2_0 = 77;
  const se3tn_scene_align_rec b = pa_scene_rec(a, 99u);
  unsigned char ab[40], bb[40];
  std::memcpy(ab, &a, 40);
  std::memcpy(bb, &b, 40);
  const uint32_t ninety_nine = 99u;
  std::memcpy(ab + 28, &ninety_nine, 4);
  CHECK(std::memcmp(ab, bb, 40) == 0);
  std::puts("pose_align_scene_check: ok");
  return 0;
}

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static int run_case(const char* in, const char* out) {
  std::FILE* f = std::fopen(in, "rb");
  CHECK(f != nullptr);
  std::vector<int32_t> hd;
  std::vector<double> dd, pts, nrm, poses;
  std::vector<uint16_t> depth, scene;
  CHECK(read_n(f, hd, 9) && hd[0] == 0x5053);
  const int P = hd[1], n = hd[2], H = hd[3], W = hd[4];
  CHECK(P >= 1 && n >= 1 && H >= 1 && W >= 1);
  se3tn_align_params prm;
  prm.gate_mm = hd[5]; prm.iters = hd[6]; prm.min_pairs = hd[7]; prm._reserved = 0;
  const double scene_tol = (double)hd[8];
  CHECK(read_n(f, dd, 11));
  prm.damping = dd[0]; prm.stop = dd[1];
  CHECK(read_n(f, pts, (size_t)P * 3) && read_n(f, nrm, (size_t)P * 3) && read_n(f, poses, (size_t)n * 16));
  CHECK(read_n(f, depth, (size_t)H * (size_t)W) && read_n(f, scene, (size_t)H * (size_t)W));
  std::fclose(f);
  const DepthFrame fr = depth_frame(depth.data(), H, W, dd.data() + 2);
  const double gate = (double)prm.gate_mm;
  std::vector<double> poses_out((size_t)n * 16);
  std::vector<se3tn_scene_align_rec> recs((size_t)n);
  std::vector<int64_t> sums((size_t)n * PA_SUMS);
  std::vector<long long> red((size_t)pa_scene_lds_words());
  for (int p = 0; p < n; ++p) {
    double sp[12];
    std::memcpy(sp, poses.data() + (size_t)p * 16, sizeof(sp));   // the bits, as the kernel's LDS copy keeps them
    se3tn_align_rec rec;
    std::memset(&rec, 0, sizeof(rec));
    uint32_t hidden_pts = 0u;
    for (int it = 0; it < prm.iters; ++it) {
      Rigid T = load_pose(sp);
      for (int w = 0; w < PA_WAVES; ++w)
        for (int k = 0; k < PA_SCENE_ROW_WORDS; ++k) red[(size_t)(pa_scene_lds_row(w) + k)] = 0;
      for (int t = 0; t < PA_THREADS; ++t) {   // a thread's registers, added to its wave's row (integer sums: any order)
        int64_t S[PA_SUMS] = {0};
        long long pairs = 0, facing = 0, hidden = 0;
        for (int j = pa_first(t); j < P; j += pa_stride()) {
          double J[6], r;
          const int k = pa_point_scene(T, fr, scene.data(), scene_tol, gate, pts[3 * (size_t)j], pts[3 * (size_t)j + 1],
                                       pts[3 * (size_t)j + 2], nrm[3 * (size_t)j], nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2], J, r);
          CHECK(k == 0 || k == 1 || k == 3 || k == 5);
          facing += k & 1;
          hidden += (k >> 2) & 1;
          if (k & 2) { pairs += 1; pa_accumulate(J, r, S); }
        }
        long long* row = red.data() + pa_scene_lds_row(t >> 6);
        for (int w = 0; w < PA_SUMS; ++w) row[w] += S[w];
        row[PA_W_PAIRS] += pairs;
        row[PA_W_FACING] += facing;
        row[PA_W_HIDDEN] += hidden;
      }
      for (int k = 0; k < PA_SCENE_ROW_WORDS; ++k) {
        long long s = 0;
        for (int w = 0; w < PA_WAVES; ++w) s += red[(size_t)(pa_scene_lds_row(w) + k)];
        red[(size_t)(pa_scene_lds_total() + k)] = s;
      }
      const long long* tot = red.data() + pa_scene_lds_total();
      int64_t St[PA_SUMS];
      for (int w = 0; w < PA_SUMS; ++w) St[w] = tot[w];
      const bool fin = pa_step(T, St, (uint32_t)tot[PA_W_PAIRS], (uint32_t)tot[PA_W_FACING], it, prm, rec);
      hidden_pts = (uint32_t)tot[PA_W_HIDDEN];
      CHECK(rec.pairs + hidden_pts <= rec.facing_pts);
      if (rec.status == SE3TN_ALIGN_ITERS || rec.status == SE3TN_ALIGN_CONVERGED)
        for (int i = 0; i < 3; ++i) { sp[4 * i] = T.r[i][0]; sp[4 * i + 1] = T.r[i][1]; sp[4 * i + 2] = T.r[i][2]; sp[4 * i + 3] = T.t[i]; }
      if (fin) break;
    }
    std::memcpy(poses_out.data() + (size_t)p * 16, sp, sizeof(sp));
    const double row3[4] = {0.0, 0.0, 0.0, 1.0};
    std::memcpy(poses_out.data() + (size_t)p * 16 + 12, row3, sizeof(row3));
    recs[(size_t)p] = pa_scene_rec(rec, hidden_pts);
    for (int w = 0; w < PA_SUMS; ++w) sums[(size_t)p * PA_SUMS + (size_t)w] = red[(size_t)(pa_scene_lds_total() + w)];
  }
  std::FILE* g = std::fopen(out, "wb");
  CHECK(g != nullptr);
  CHECK(std::fwrite(poses_out.data(), sizeof(double), poses_out.size(), g) == poses_out.size());
  CHECK(std::fwrite(recs.data(), sizeof(se3tn_scene_align_rec), recs.size(), g) == recs.size());
  CHECK(std::fwrite(sums.data(), sizeof(int64_t), sums.size(), g) == sums.size());
  CHECK(std::fclose(g) == 0);
  std::puts("pose_align_scene_check: case done");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return run_case(argv[1], argv[2]);
  if (argc == 1) return check_plan();
  std::fprintf(stderr, "usage: pose_align_scene_check [CASE OUT]\n");
  return 2;
}
