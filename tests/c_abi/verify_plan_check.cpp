// Stand-alone host check of csrc/verify_plan.h (built with -fsanitize=address,undefined by tests/test_color_fit_host.py): the staging
// buffer of se3tn_verify_poses_host for 1 .. 40 hypotheses of every kind of window (inside the frame, over a border, larger than the
// frame, off the frame) against ONE frame.  The buffer is malloc'ed with EXACTLY the planned bytes; the records in front are written in
// full as the kernel and the read-back touch them, the windows are staged behind them, and afterwards every record byte and every
// window pixel read through the crop descriptors must still hold what was put there: nothing overlaps, nothing overruns.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "verify_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

// fx = fy = 100 and z = 0.1 m: the window is the square of side w pixels centred at pixel (cx, cy)
static const double K[9] = {100, 0, 0, 0, 100, 0, 0, 0, 1};
static void pose_at(double cx, double cy, double z, double P[16]) {
  for (int i = 0; i < 16; ++i) P[i] = i % 5 == 0 ? 1.0 : 0.0;
  P[3] = cx / 1000; P[7] = cy / 1000; P[11] = z;
}

static int check_frame(int H, int W) {
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<uint16_t> depth((size_t)H * W);
  unsigned s = 777u + (unsigned)W;
  for (auto& v : rgb) v = (uint8_t)(1 + (s = s * 1664525u + 1013904223u) % 255);          // never 0: the padding is
  for (auto& v : depth) v = (uint16_t)(1 + (s = s * 1664525u + 1013904223u) % 65535);
  const int big = 2 * (H > W ? H : W) + 4;
  const int kinds[5][3] = {{W / 2, H / 2, H < 8 ? 2 : 4}, {0, H / 2, 6}, {W, H, 6}, {W / 2, H / 2, big}, {W + 50, H + 50, 10}};
  for (int n = 1; n <= 40; n += (n < 9 ? 1 : 31)) {   // 1 .. 9 and 40
    const VerifyLayout L = plan_verify(n);
    CHECK(L.fit_off == 0 && L.color_off == (size_t)n * 32 && L.rec_bytes == (size_t)n * 112);
    CHECK(L.begin >= L.rec_bytes && L.begin - L.rec_bytes < 256 && L.begin % 256 == 0 && L.color_off % 4 == 0);
    std::vector<TrackWindow> win(n);
    size_t bytes = L.begin;
    for (int i = 0; i < n; ++i) {
      const int* kd = kinds[(i + n) % 5];
      double P[16];
      pose_at(kd[0], kd[1], 0.1, P);
      CHECK(plan_window(P, K, kd[2], H, W, bytes, win[i]) == PlanStatus::OK);
      CHECK(win[i].off_rgb >= L.begin && win[i].off_rgb % 64 == 0 && win[i].off_d % 64 == 0);
    }
    CHECK(bytes > L.begin);   // every window stages at least its zero pixel: the upload is never empty
    uint8_t* host = (uint8_t*)std::malloc(bytes);
    CHECK(host);
    se3tn_fit* fit = (se3tn_fit*)(host + L.fit_off);
    se3tn_color_fit* col = (se3tn_color_fit*)(host + L.color_off);
    for (int i = 0; i < n; ++i) {
      fit[i] = se3tn_fit{1u + i, 2, 3, 4, 5, 6, 7, 0};
      col[i].px = 100u + i; col[i].tol_mm = 7;
      for (int ch = 0; ch < 3; ++ch) {
        col[i].sum_m[ch] = col[i].sum_o[ch] = col[i].sum_mm[ch] = col[i].sum_oo[ch] = col[i].sum_mo[ch] = 0xFFFFFFFFu - ch;
        col[i].sum_abs[ch] = 9u + ch;
      }
    }
    for (int i = 0; i < n; ++i) stage_window(win[i], rgb.data(), depth.data(), W, host);
    for (int i = 0; i < n; ++i) {
      CHECK(fit[i].model_px == 1u + i && fit[i].tol_mm == 7 && col[i].px == 100u + i && col[i].sum_abs[2] == 11u && col[i].sum_mo[1] == 0xFFFFFFFEu);
      se3tn_crop ca, cb;
      const ImageA windowA{rgb.data(), depth.data(), nullptr};
      crop_pair(win[i], 0.0, windowA, host, ca, cb);
      const TrackWindow& t = win[i];
      for (int y = 0; y < cb.bottom - cb.top; ++y)
        for (int x = 0; x < cb.right - cb.left; ++x) {
          const int sx = cb.left + x, sy = cb.top + y, fx = t.winB[0] + x, fy = t.winB[1] + y;
          const bool in_sub = sx >= 0 && sx < cb.W && sy >= 0 && sy < cb.H, in_frame = fx >= 0 && fx < W && fy >= 0 && fy < H;
          CHECK((in_sub ? cb.depth[(size_t)sy * cb.W + sx] : 0) == (in_frame ? depth[(size_t)fy * W + fx] : 0));
          CHECK((in_sub ? cb.rgb[((size_t)sy * cb.W + sx) * 3 + 2] : 0) == (in_frame ? rgb[((size_t)fy * W + fx) * 3 + 2] : 0));
        }
    }
    std::free(host);
  }
  return 0;
}

int main() {
  const int frames[3][2] = {{120, 160}, {97, 131}, {1, 1}};
  for (const auto& f : frames)
    if (check_frame(f[0], f[1])) return 1;
  std::puts("verify_plan_check: ok");
  return 0;
}
