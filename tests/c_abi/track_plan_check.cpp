// Stand-alone host check of csrc/track_plan.h (built with -fsanitize=address,undefined by tests/test_host_abi.py): for several frame
// sizes and 1 .. 7 windows of every kind (inside the frame, over each border, larger than the frame, off the frame) the staging buffer
// is malloc'ed with EXACTLY the planned bytes, staged in one range and in four, and every window pixel read through the crop
// descriptors must equal a direct read of the frame with zero outside.  Exits non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "track_plan.h"

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

// every pixel of the descriptor's window against the frame under winB (zero outside either image)
static int check_crop(const se3tn_crop& k, const TrackWindow& t, const uint8_t* rgb, const uint16_t* depth, int H, int W) {
  CHECK(k.right - k.left == t.winB[2] - t.winB[0] && k.bottom - k.top == t.winB[3] - t.winB[1]);
  for (int i = 0; i < k.bottom - k.top; ++i)
    for (int j = 0; j < k.right - k.left; ++j) {
      const int sx = k.left + j, sy = k.top + i, fx = t.winB[0] + j, fy = t.winB[1] + i;
      const bool in_sub = sx >= 0 && sx < k.W && sy >= 0 && sy < k.H, in_frame = fx >= 0 && fx < W && fy >= 0 && fy < H;
      for (int ch = 0; ch < 3; ++ch)
        CHECK((in_sub ? k.rgb[((size_t)sy * k.W + sx) * 3 + ch] : 0) == (in_frame ? rgb[((size_t)fy * W + fx) * 3 + ch] : 0));
      CHECK((in_sub ? k.depth[(size_t)sy * k.W + sx] : 0) == (in_frame ? depth[(size_t)fy * W + fx] : 0));
    }
  return 0;
}

static int check_frame(int H, int W) {
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  std::vector<uint16_t> depth((size_t)H * W);
  unsigned s = 12345u + (unsigned)H;
  for (auto& v : rgb) v = (uint8_t)(1 + (s = s * 1664525u + 1013904223u) % 255);          // never 0: the padding is
  for (auto& v : depth) v = (uint16_t)(1 + (s = s * 1664525u + 1013904223u) % 65535);
  const int big = 2 * (H > W ? H : W) + 4;
  // centre x, centre y, side: inside (a 1 x 1 frame: around it), over the left / top / right / bottom border, larger than the frame, off it
  const int kinds[7][3] = {{W / 2, H / 2, H < 8 ? 2 : 4}, {0, H / 2, 6}, {W / 2, 0, 6}, {W, H / 2, 6}, {W / 2, H, 6}, {W / 2, H / 2, big}, {W + 50, H + 50, 10}};
  alignas(64) static const uint8_t zero[64] = {};
  for (int n = 1; n <= 7; ++n) {
    std::vector<TrackWindow> win(n);
    size_t bytes = 256;
    for (int i = 0; i < n; ++i) {
      const int* kd = kinds[(i + H) % 7];   // (another kind first per frame size)
      double P[16];
      pose_at(kd[0], kd[1], 0.1, P);
      const size_t before = bytes;
      CHECK(plan_window(P, K, kd[2], H, W, bytes, win[i]) == PlanStatus::OK);
      const TrackWindow& t = win[i];
      CHECK(t.winB[2] - t.winB[0] == kd[2] && t.winB[3] - t.winB[1] == kd[2] && t.winA[2] - t.winA[0] == kd[2]);
      CHECK(t.off_rgb == before && t.off_rgb % 64 == 0 && t.off_d % 64 == 0 && bytes % 64 == 0);
      CHECK(t.off_d >= t.off_rgb + (size_t)t.sw * t.sh * 3 && bytes >= t.off_d + (size_t)t.sw * t.sh * 2);
      CHECK(t.miss == (kd == kinds[6]) && (kd != kinds[5] || (t.sw == W && t.sh == H)));
      CHECK(t.miss ? (t.sw == 1 && t.sh == 1) : (t.x0 >= 0 && t.y0 >= 0 && t.x0 + t.sw <= W && t.y0 + t.sh <= H && t.sw > 0 && t.sh > 0));
    }
    for (int parts = 1; parts <= 4; parts += 3) {   // one range, then four (the helper threads' split of se3tn_on_track_batch)
      uint8_t* host = (uint8_t*)std::malloc(bytes);
      CHECK(host);
      for (int k = 0; k < parts; ++k)
        for (int i = (int)((long long)n * k / parts); i < (int)((long long)n * (k + 1) / parts); ++i)
          stage_window(win[i], rgb.data(), depth.data(), W, host);
      for (int i = 0; i < n; ++i) {
        se3tn_crop ca, cb;
        const ImageA windowA{rgb.data(), depth.data(), nullptr};
        crop_pair(win[i], 100.0, windowA, host, ca, cb);
        CHECK(ca.rgb == rgb.data() && ca.H == 176 && ca.W == 176 && ca.left == 0 && ca.top == 0 && ca.right == 176 && ca.bottom == 176);
        CHECK(ca.stats == 0 && cb.stats == 1 && ca.z_offset_mm == 100.0 && cb.z_offset_mm == 100.0);
        if (check_crop(cb, win[i], rgb.data(), depth.data(), H, W)) return 1;
        // the frame route's image A: the "rendered rectangle" is the staged sub-image here, a miss reads the zero image
        const ImageA frameA{host + win[i].off_rgb, (const uint16_t*)(host + win[i].off_d), zero};
        crop_pair(win[i], 100.0, frameA, host, ca, cb);
        CHECK(ca.stats == 0 && (ca.rgb == zero) == win[i].miss && ca.H == win[i].sh && ca.W == win[i].sw);
        if (check_crop(ca, win[i], rgb.data(), depth.data(), H, W)) return 1;
      }
      std::free(host);
    }
  }
  return 0;
}

int main() {
  const int frames[3][2] = {{480, 640}, {97, 131}, {1, 1}};
  for (const auto& f : frames)
    if (check_frame(f[0], f[1])) return 1;
  // the refusals: a pose at or behind the camera plane or not finite, and a window without pixels
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  TrackWindow t;
  double P[16];
  size_t bytes = 0;
  for (double z : {0.0, -0.5, nan}) {
    pose_at(10, 10, z, P);
    CHECK(plan_window(P, K, 100.0, 480, 640, bytes, t) == PlanStatus::NOT_IN_FRONT);
  }
  pose_at(nan, 10, 0.1, P);
  CHECK(plan_window(P, K, 100.0, 480, 640, bytes, t) == PlanStatus::NOT_IN_FRONT);
  pose_at(10, inf, 0.1, P);
  CHECK(plan_window(P, K, 100.0, 480, 640, bytes, t) == PlanStatus::NOT_IN_FRONT);
  pose_at(10, 10, 1e-12, P);   // the projection leaves the int32 range
  CHECK(plan_window(P, K, 100.0, 480, 640, bytes, t) == PlanStatus::NOT_IN_FRONT);
  pose_at(10, 10, inf, P);     // every corner projects onto the principal point
  CHECK(plan_window(P, K, 100.0, 480, 640, bytes, t) == PlanStatus::EMPTY_WINDOW);
  pose_at(10, 10, 0.1, P);
  CHECK(plan_window(P, K, 0.0, 480, 640, bytes, t) == PlanStatus::EMPTY_WINDOW);
  CHECK(bytes == 0);   // a refusal places nothing
  std::puts("track_plan_check: ok");
  return 0;
}
