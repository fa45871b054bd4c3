// Stand-alone host check of the live-camera layout of csrc/track_plan.h (plan_live, stage_window's BGR swap, crop_pair on the layout;
// built with -fsanitize=address,undefined by tests/test_multi_live_host.py).  For seeded poses at 480 x 640 and 37 x 53 -- windows
// inside the frame, over its borders and off it -- the regions of the staging buffer of se3tn_on_track_objects_live must be disjoint,
// 64-byte aligned and inside the planned size; staging with the swap must write exactly its regions of a buffer malloc'ed with
// EXACTLY the planned bytes; and crop_pair must give the descriptors of the non-live plan, shifted.  Exits non-zero at the first
// mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
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

static unsigned g_seed = 2024u;
static int rnd(int lo, int hi) {   // [lo, hi]
  g_seed = g_seed * 1664525u + 1013904223u;
  return lo + (int)((g_seed >> 8) % (unsigned)(hi - lo + 1));
}

static const uint8_t FILL = 0xCD;
static int seen_miss = 0, seen_border = 0, seen_inside = 0;

// every pixel of the descriptor's window against the frame under winB (zero outside either image); the frame is BGR, the crop RGB
static int check_crop(const se3tn_crop& k, const TrackWindow& t, const uint8_t* bgr, const uint16_t* depth, int H, int W) {
  CHECK(k.right - k.left == t.winB[2] - t.winB[0] && k.bottom - k.top == t.winB[3] - t.winB[1]);
  for (int i = 0; i < k.bottom - k.top; ++i)
    for (int j = 0; j < k.right - k.left; ++j) {
      const int sx = k.left + j, sy = k.top + i, fx = t.winB[0] + j, fy = t.winB[1] + i;
      const bool in_sub = sx >= 0 && sx < k.W && sy >= 0 && sy < k.H, in_frame = fx >= 0 && fx < W && fy >= 0 && fy < H;
      for (int ch = 0; ch < 3; ++ch)
        CHECK((in_sub ? k.rgb[((size_t)sy * k.W + sx) * 3 + ch] : 0) == (in_frame ? bgr[((size_t)fy * W + fx) * 3 + (2 - ch)] : 0));
      CHECK((in_sub ? k.depth[(size_t)sy * k.W + sx] : 0) == (in_frame ? depth[(size_t)fy * W + fx] : 0));
    }
  return 0;
}

static int check_call(int n, int H, int W, const uint8_t* bgr, const uint16_t* depth) {
  std::vector<TrackWindow> plain(n);
  std::vector<double> z(n);
  const size_t begin = 2 * ((((size_t)n * 128) + 255) & ~(size_t)255);   // poses | mean / std table, as the library lays them
  size_t plain_bytes = begin;
  for (int i = 0; i < n; ++i) {
    double P[16];
    const int side = rnd(2, H < 100 ? 30 : 180);
    z[i] = 0.1;
    pose_at(rnd(-40, W + 40), rnd(-40, H + 40), z[i], P);
    CHECK(plan_window(P, K, side, H, W, plain_bytes, plain[i]) == PlanStatus::OK);
    const TrackWindow& t = plain[i];
    if (t.miss) ++seen_miss;
    else if (t.sw < side || t.sh < side) ++seen_border;
    else ++seen_inside;
  }
  std::vector<TrackWindow> live = plain;
  const LiveLayout L = plan_live(n, live.data(), H, W, begin);
  const size_t fpx = (size_t)H * W;

  // the regions: disjoint, 64-byte aligned, behind `begin`, inside the planned size
  std::vector<std::pair<size_t, size_t>> reg;   // [first, second)
  int fills = 0;
  for (int i = 0; i < n; ++i) {
    const TrackWindow& t = live[i];
    const size_t px = (size_t)t.sw * t.sh;
    reg.push_back({t.off_rgb, t.off_rgb + px * 3});
    CHECK(t.off_rgb + px * 3 <= L.zero_off);          // the colour windows travel: in front of the zero pixel
    if (t.miss) {
      CHECK(t.off_d == L.zero_off && px == 1);        // a miss reads the zero pixel
    } else {
      reg.push_back({t.off_d, t.off_d + px * 2});
      CHECK(t.off_d >= L.upload_bytes);               // the filled windows exist on the device only: behind the upload
      ++fills;
    }
    // nothing but the two offsets changes
    const TrackWindow& p = plain[i];
    CHECK(t.x0 == p.x0 && t.y0 == p.y0 && t.sw == p.sw && t.sh == p.sh && t.miss == p.miss);
    for (int k = 0; k < 4; ++k) CHECK(t.winA[k] == p.winA[k] && t.winB[k] == p.winB[k]);
  }
  CHECK(fills == L.fills);
  reg.push_back({L.zero_off, L.zero_off + 64});
  reg.push_back({L.raw_off, L.raw_off + fpx * 2});
  CHECK(L.raw_off == L.zero_off + 64 && L.upload_bytes == L.raw_off + fpx * 2);
  std::sort(reg.begin(), reg.end());
  CHECK(reg.front().first >= begin);
  for (size_t k = 0; k < reg.size(); ++k) {
    CHECK(reg[k].first % 64 == 0 && reg[k].second > reg[k].first && reg[k].second <= L.total);
    if (k) CHECK(reg[k].first >= reg[k - 1].second);
  }
  CHECK(L.total % 64 == 0 && L.total >= L.upload_bytes);

  // staging with the BGR swap writes exactly its regions (the buffer has exactly the planned bytes: an overrun is a report)
  uint8_t* host = (uint8_t*)std::malloc(L.total);
  CHECK(host);
  std::memset(host, FILL, L.total);
  for (int i = 0; i < n; ++i) stage_window(live[i], bgr, nullptr, W, host, true);
  std::vector<uint8_t> written(L.total, 0);
  for (int i = 0; i < n; ++i) {
    const TrackWindow& t = live[i];
    const size_t bytes = (size_t)t.sw * t.sh * 3;
    for (size_t b = 0; b < bytes; ++b) written[t.off_rgb + b] = 1;
    if (t.miss) { CHECK(host[t.off_rgb] == 0 && host[t.off_rgb + 1] == 0 && host[t.off_rgb + 2] == 0); continue; }
    for (int y = 0; y < t.sh; ++y)
      for (int x = 0; x < t.sw; ++x)
        for (int ch = 0; ch < 3; ++ch)
          CHECK(host[t.off_rgb + ((size_t)y * t.sw + x) * 3 + ch] == bgr[((size_t)(t.y0 + y) * W + t.x0 + x) * 3 + (2 - ch)]);
  }
  for (size_t b = 0; b < L.total; ++b) CHECK(written[b] || host[b] == FILL);

  // the rest of the upload as the library stages it, and the filled windows as the device pass leaves them (here: the frame's own
  // depth), then every window pixel through the descriptors
  std::memset(host + L.zero_off, 0, 2);
  std::memcpy(host + L.raw_off, depth, fpx * 2);
  for (int i = 0; i < n; ++i) {
    const TrackWindow& t = live[i];
    if (t.miss) continue;
    for (int y = 0; y < t.sh; ++y)
      std::memcpy(host + t.off_d + (size_t)y * t.sw * 2, depth + (size_t)(t.y0 + y) * W + t.x0, (size_t)t.sw * 2);
  }
  alignas(64) static const uint8_t zero[64] = {};
  for (int i = 0; i < n; ++i) {
    for (int route = 0; route < 2; ++route) {
      const ImageA A = route ? ImageA{bgr, depth, zero} : ImageA{bgr, depth, nullptr};
      se3tn_crop la, lb, pa, pb;
      crop_pair(live[i], z[i] * 1000, A, host, la, lb);
      crop_pair(plain[i], z[i] * 1000, A, host, pa, pb);
      // image B: the descriptor of the non-live plan with its two pointers shifted to the live regions
      CHECK(lb.rgb == host + live[i].off_rgb && pb.rgb == host + plain[i].off_rgb);
      CHECK((const uint8_t*)lb.depth == host + live[i].off_d && (const uint8_t*)pb.depth == host + plain[i].off_d);
      CHECK(lb.H == pb.H && lb.W == pb.W && lb.left == pb.left && lb.top == pb.top && lb.right == pb.right && lb.bottom == pb.bottom);
      CHECK(lb.z_offset_mm == pb.z_offset_mm && lb.stats == 1 && pb.stats == 1 && lb._pad == 0);
      // image A does not depend on the layout
      CHECK(la.rgb == pa.rgb && la.depth == pa.depth && la.H == pa.H && la.W == pa.W && la.left == pa.left && la.top == pa.top);
      CHECK(la.right == pa.right && la.bottom == pa.bottom && la.z_offset_mm == pa.z_offset_mm && la.stats == 0 && pa.stats == 0);
      if (!route && check_crop(lb, live[i], bgr, depth, H, W)) return 1;
    }
  }
  std::free(host);
  return 0;
}

int main() {
  const int frames[2][2] = {{480, 640}, {37, 53}};
  for (const auto& f : frames) {
    const int H = f[0], W = f[1];
    std::vector<uint8_t> bgr((size_t)H * W * 3);
    std::vector<uint16_t> depth((size_t)H * W);
    unsigned s = 977u + (unsigned)H;
    for (auto& v : bgr) { v = (uint8_t)(1 + (s = s * 1664525u + 1013904223u) % 255); if (v == FILL) v = 1; }   // never 0, never the fill byte
    for (auto& v : depth) v = (uint16_t)(1 + (s = s * 1664525u + 1013904223u) % 65535);
    for (int rep = 0; rep < 6; ++rep)
      for (int n : {1, 2, 3, 5, 9})
        if (check_call(n, H, W, bgr.data(), depth.data())) return 1;
  }
  CHECK(seen_miss >= 5 && seen_border >= 5 && seen_inside >= 5);   // the seeded poses cover all three kinds
  // all objects off the frame: no rectangle, every depth pointer on the zero pixel
  {
    TrackWindow t[2];
    size_t bytes = 512;
    double P[16];
    pose_at(900, 700, 0.1, P);
    CHECK(plan_window(P, K, 20, 480, 640, bytes, t[0]) == PlanStatus::OK && plan_window(P, K, 30, 480, 640, bytes, t[1]) == PlanStatus::OK);
    const LiveLayout L = plan_live(2, t, 480, 640, 512);
    CHECK(L.fills == 0 && t[0].off_d == L.zero_off && t[1].off_d == L.zero_off && L.total == ((L.upload_bytes + 63) & ~(size_t)63));
  }
  std::puts("live_plan_check: ok");
  return 0;
}
