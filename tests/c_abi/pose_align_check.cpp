// Stand-alone host check of csrc/pose_align_math.h and csrc/pose_align_plan.h (built with -ffp-contract=off and
// -fsanitize=address,undefined by tests/test_pose_align_host.py): the statements the kernel runs, run on the host.
//   pose_align_check                     the plan alone: the thread-to-point walk visits every point exactly once for
//                                        P in {1, 63, 64, 65, T - 1, T, T + 1, 2 T + 1}, the LDS rows do not overlap and the staging
//                                        regions are ordered, aligned and walked over buffers of exactly the planned bytes;
//   pose_align_check CASE OUT            reads a case, aligns every pose with the shared header functions -- walking the points in
//                                        the kernel's order: thread by thread, each thread's own partial sums, then the waves' rows
//                                        -- and writes [poses n x 16 doubles | records n x 40 bytes | sums n x 28 int64] to OUT.
// CASE: int32 {magic 0x5041, P, n, H, W, gate_mm, iters, min_pairs}, float64 {damping, stop, K[9]}, float64 points [P,3], normals [P,3],
// poses [n,16], uint16 depth [H,W].  Exits non-zero at the first mismatch.
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

static int check_walk(int P) {
  std::vector<uint8_t> visits((size_t)P, 0);
  long long total = 0;
  for (int t = 0; t < PA_THREADS; ++t) {
    int mine = 0;
    for (int j = pa_first(t); j < P; j += pa_stride()) {
      CHECK(j >= 0 && j < P && visits[(size_t)j] == 0);
      visits[(size_t)j] = 1;
      ++mine;
    }
    CHECK(mine == pa_count(t, P));
    total += mine;
  }
  CHECK(total == P);
  for (uint8_t v : visits) CHECK(v == 1);
  return 0;
}

static int check_lds() {
  long long* red = (long long*)std::malloc(sizeof(long long) * (size_t)pa_lds_words());   // exactly as the kernel declares it
  CHECK(red != nullptr);
  for (int w = 0; w < PA_WAVES; ++w) {
    CHECK(pa_lds_row(w) == w * PA_ROW_WORDS && pa_lds_row(w) + PA_ROW_WORDS <= pa_lds_total());
    for (int k = 0; k < PA_ROW_WORDS; ++k) red[pa_lds_row(w) + k] = (long long)(w + 1) * 1000 + k;
  }
  CHECK(pa_lds_total() + PA_ROW_WORDS == pa_lds_words());
  for (int t = 0; t < PA_THREADS; ++t)
    if (t < PA_ROW_WORDS) {
      long long s = 0;
      for (int w = 0; w < PA_WAVES; ++w) s += red[pa_lds_row(w) + t];
      red[pa_lds_total() + t] = s;
    }
  for (int k = 0; k < PA_ROW_WORDS; ++k)
    CHECK(red[pa_lds_total() + k] == (long long)PA_WAVES * (PA_WAVES + 1) / 2 * 1000 + (long long)PA_WAVES * k);
  std::free(red);
  CHECK(PA_W_PAIRS == PA_SUMS && PA_W_FACING == PA_SUMS + 1 && PA_ROW_WORDS == PA_SUMS + 2);
  return 0;
}

static int check_stage(int n, int H, int W, int with_sums) {
  const PaStage s = pa_stage(n, H, W, with_sums);
  const size_t px = (size_t)H * (size_t)W;
  CHECK(s.poses == 0 && s.depth == (size_t)n * 128 && s.upload_bytes == s.depth + px * 2);
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
  std::vector<uint16_t> depth(px, 700);
  std::memcpy(h + s.poses, poses.data(), sizeof(double) * 16 * (size_t)n);
  std::memcpy(h + s.depth, depth.data(), sizeof(uint16_t) * px);
  std::memcpy(d, h, s.upload_bytes);
  double* po = reinterpret_cast<double*>(d + s.poses_out);
  se3tn_align_rec* rec = reinterpret_cast<se3tn_align_rec*>(d + s.rec);
  int64_t* sums = reinterpret_cast<int64_t*>(d + s.sums);
  for (size_t i = 0; i < (size_t)n; ++i) {
    for (int k = 0; k < 16; ++k) po[i * 16 + (size_t)k] = reinterpret_cast<const double*>(d + s.poses)[i * 16 + (size_t)k] + (double)i;
    rec[i].iterations = (uint32_t)i; rec[i].sum_r2_0 = -(int64_t)i;
    for (int k = 0; k < PA_SUMS; ++k) sums[i * PA_SUMS + (size_t)k] = (int64_t)i * 100 + k;
  }
  for (size_t i = 0; i < px; ++i) CHECK(reinterpret_cast<const uint16_t*>(d + s.depth)[i] == 700);
  std::memcpy(h + s.poses_out, d + s.poses_out, s.readback_bytes);
  for (size_t i = 0; i < (size_t)n; ++i) {
    CHECK(reinterpret_cast<const double*>(h + s.poses_out)[i * 16 + 15] == 1.5 + (double)i);
    CHECK(reinterpret_cast<const se3tn_align_rec*>(h + s.rec)[i].sum_r2_0 == -(int64_t)i);
    if (with_sums) CHECK(reinterpret_cast<const int64_t*>(h + s.sums)[i * PA_SUMS + 27] == (int64_t)i * 100 + 27);
  }
  std::free(h);
  std::free(d);
  return 0;
}

static int check_plan() {
  const int Ps[] = {1, 63, 64, 65, PA_THREADS - 1, PA_THREADS, PA_THREADS + 1, 2 * PA_THREADS + 1};
  for (int P : Ps)
    if (check_walk(P)) { std::fprintf(stderr, "P = %d\n", P); return 1; }
  if (check_lds()) return 1;
  const int ns[] = {1, 2, 7, 65, PA_MAX_POSES};
  const int hw[][2] = {{1, 1}, {3, 1}, {5, 7}, {120, 160}, {481, 641}};
  for (int n : ns)
    for (const auto& f : hw)
      for (int ws = 0; ws < 2; ++ws)
        if (check_stage(n, f[0], f[1], ws)) { std::fprintf(stderr, "n = %d, H = %d, W = %d, sums = %d\n", n, f[0], f[1], ws); return 1; }
  // the clamp of fx: 2^20 points of the largest term stay below 2^63
  CHECK(pa_fx(1e300) == (int64_t)256 << 32 && pa_fx(-1e300) == -((int64_t)256 << 32) && pa_fx(0.5) == (int64_t)1 << 31);
  CHECK(pa_fx(NAN) == -((int64_t)256 << 32));
  std::puts("pose_align_check: ok");
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
  std::vector<uint16_t> depth;
  CHECK(read_n(f, hd, 8) && hd[0] == 0x5041);
  const int P = hd[1], n = hd[2], H = hd[3], W = hd[4];
  CHECK(P >= 1 && n >= 1 && H >= 1 && W >= 1);
  se3tn_align_params prm;
  prm.gate_mm = hd[5]; prm.iters = hd[6]; prm.min_pairs = hd[7]; prm._reserved = 0;
  CHECK(read_n(f, dd, 11));
  prm.damping = dd[0]; prm.stop = dd[1];
  CHECK(read_n(f, pts, (size_t)P * 3) && read_n(f, nrm, (size_t)P * 3) && read_n(f, poses, (size_t)n * 16));
  CHECK(read_n(f, depth, (size_t)H * (size_t)W));
  std::fclose(f);
  const DepthFrame fr = depth_frame(depth.data(), H, W, dd.data() + 2);
  const double gate = (double)prm.gate_mm;
  std::vector<double> poses_out((size_t)n * 16);
  std::vector<se3tn_align_rec> recs((size_t)n);
  std::vector<int64_t> sums((size_t)n * PA_SUMS);
  std::vector<long long> red((size_t)pa_lds_words());
  for (int p = 0; p < n; ++p) {
    double sp[12];
    std::memcpy(sp, poses.data() + (size_t)p * 16, sizeof(sp));   // the bits, as the kernel's LDS copy keeps them
    se3tn_align_rec rec;
    std::memset(&rec, 0, sizeof(rec));
    for (int it = 0; it < prm.iters; ++it) {
      Rigid T = load_pose(sp);
      for (int w = 0; w < PA_WAVES; ++w)
        for (int k = 0; k < PA_ROW_WORDS; ++k) red[(size_t)(pa_lds_row(w) + k)] = 0;
      for (int t = 0; t < PA_THREADS; ++t) {   // a thread's registers, added to its wave's row (integer sums: any order)
        int64_t S[PA_SUMS] = {0};
        long long pairs = 0, facing = 0;
        for (int j = pa_first(t); j < P; j += pa_stride()) {
          double J[6], r;
          const int k = pa_point(T, fr, gate, pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2], nrm[3 * (size_t)j],
                                 nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2], J, r);
          facing += k & 1;
          if (k & 2) { pairs += 1; pa_accumulate(J, r, S); }
        }
        long long* row = red.data() + pa_lds_row(t >> 6);
        for (int w = 0; w < PA_SUMS; ++w) row[w] += S[w];
        row[PA_W_PAIRS] += pairs;
        row[PA_W_FACING] += facing;
      }
      for (int k = 0; k < PA_ROW_WORDS; ++k) {
        long long s = 0;
        for (int w = 0; w < PA_WAVES; ++w) s += red[(size_t)(pa_lds_row(w) + k)];
        red[(size_t)(pa_lds_total() + k)] = s;
      }
      const long long* tot = red.data() + pa_lds_total();
      int64_t St[PA_SUMS];
      for (int w = 0; w < PA_SUMS; ++w) St[w] = tot[w];
      const bool fin = pa_step(T, St, (uint32_t)tot[PA_W_PAIRS], (uint32_t)tot[PA_W_FACING], it, prm, rec);
      if (rec.status == SE3TN_ALIGN_ITERS || rec.status == SE3TN_ALIGN_CONVERGED)
        for (int i = 0; i < 3; ++i) { sp[4 * i] = T.r[i][0]; sp[4 * i + 1] = T.r[i][1]; sp[4 * i + 2] = T.r[i][2]; sp[4 * i + 3] = T.t[i]; }
      if (fin) break;
    }
    std::memcpy(poses_out.data() + (size_t)p * 16, sp, sizeof(sp));
    const double row3[4] = {0.0, 0.0, 0.0, 1.0};
    std::memcpy(poses_out.data() + (size_t)p * 16 + 12, row3, sizeof(row3));
    recs[(size_t)p] = rec;
    for (int w = 0; w < PA_SUMS; ++w) sums[(size_t)p * PA_SUMS + (size_t)w] = red[(size_t)(pa_lds_total() + w)];
  }
  std::FILE* g = std::fopen(out, "wb");
  CHECK(g != nullptr);
  CHECK(std::fwrite(poses_out.data(), sizeof(double), poses_out.size(), g) == poses_out.size());
  CHECK(std::fwrite(recs.data(), sizeof(se3tn_align_rec), recs.size(), g) == recs.size());
  CHECK(std::fwrite(sums.data(), sizeof(int64_t), sums.size(), g) == sums.size());
  CHECK(std::fclose(g) == 0);
  std::puts("pose_align_check: case done");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return run_case(argv[1], argv[2]);
  if (argc == 1) return check_plan();
  std::fprintf(stderr, "usage: pose_align_check [CASE OUT]\n");
  return 2;
}
