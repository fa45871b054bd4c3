// Stand-alone host check of csrc/fit_rule.h, csrc/scene_fit_rule.h and csrc/scene_fit_plan.h (built with -fsanitize=address,undefined by
// tests/test_scene_fit_host.py).  The scene kernel is replayed on the host exactly as it is laid out -- the plan's tiles, 256 threads
// per tile, every thread's pixel through the rule's statements -- on frames, layers and outputs malloc'ed with EXACTLY their bytes, so
// an index past a layer, a frame or an output is a sanitizer report.  Checked: the records of synthetic cases equal numbers written
// here; every pixel of the union of the rectangles is visited exactly once and no tile beyond the planned ones is needed; the
// multiply-and-shift that finds a tile's row equals the division for every tile of the extreme frames; the staging regions of
// se3tn_scene_fit_host do not overlap; fit_classify (the depth rule of a pixel) gives the counts written here, and scene_classify on
// an owned pixel is fit_classify with the visible bit inserted.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_fit_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

struct Rec { unsigned w[SCENE_RECORD_WORDS]; };   // se3tn_scene_fit's words

struct Case {
  int H, W, n, tol;
  std::vector<int32_t> rects;             // [n,4]
  std::vector<uint16_t*> depth;           // exact-size mallocs (nullptr: empty)
  uint16_t* observed;                     // exact-size malloc
  ~Case() { for (auto* d : depth) std::free(d); std::free(observed); }
};

static uint16_t* alloc_u16(size_t count, int value) {
  uint16_t* p = (uint16_t*)std::malloc(count * 2);
  for (size_t i = 0; i < count; ++i) p[i] = (uint16_t)value;
  return p;
}
static void add_layer(Case& c, int x0, int y0, int x1, int y1, int value) {
  const int32_t r[4] = {x0, y0, x1, y1};
  c.rects.insert(c.rects.end(), r, r + 4);
  c.depth.push_back(scene_rect_empty(r) ? nullptr : alloc_u16((size_t)(x1 - x0) * (y1 - y0), value));
  c.n = (int)c.depth.size();
}

// the kernel, tile by tile and thread by thread; ids / scene may be null.  visits [H,W] counts how often a pixel was a thread's
static int replay(const Case& c, bool whole, std::vector<Rec>& out, uint8_t* ids, uint16_t* scene, std::vector<int>& visits, ScenePlan& plan) {
  std::vector<SceneLayer> l(c.n);
  for (int i = 0; i < c.n; ++i) {
    const int32_t* r = &c.rects[4 * i];
    CHECK(scene_rect_ok(r, c.H, c.W));
    l[i] = scene_rect_empty(r) ? SceneLayer{nullptr, 0, 0, 0, 0} : SceneLayer{c.depth[i], r[0], r[1], r[2], r[3]};
  }
  plan = plan_scene(c.n, c.rects.data(), c.H, c.W, whole);
  CHECK(plan.tiles_x >= 1 && plan.tiles_y >= 1 && plan.x0 >= 0 && plan.y0 >= 0 && plan.x1 <= c.W && plan.y1 <= c.H);
  std::vector<unsigned> cnt((size_t)c.n * SCENE_WORDS, 0u);
  visits.assign((size_t)c.H * c.W, 0);
  for (unsigned b = 0; b < (unsigned)(plan.tiles_x * plan.tiles_y); ++b) {
    int bx, by;
    scene_tile_of(plan, b, bx, by);
    CHECK(by == (int)(b / (unsigned)plan.tiles_x) && bx == (int)(b % (unsigned)plan.tiles_x));
    for (int t = 0; t < SCENE_THREADS; ++t) {
      int x, y;
      scene_thread_pixel(plan, bx, by, t, x, y);
      if (!(x < plan.x1 && y < plan.y1)) continue;
      const size_t q = (size_t)y * c.W + x;
      ++visits[q];
      const int o = c.observed[q];
      int owner = -1, best = 0;
      for (int i = 0; i < c.n; ++i) scene_offer(i, scene_layer_at(l[i], x, y), owner, best);
      if (ids) ids[q] = (uint8_t)(owner + 1);
      if (scene) scene[q] = (uint16_t)best;
      for (int i = 0; i < c.n; ++i) {
        unsigned ad, hb;
        const unsigned bits = scene_classify(i, scene_layer_at(l[i], x, y), owner, o, c.tol, ad, hb);
        for (int k = 0; k < SC_COUNTS; ++k) cnt[(size_t)i * SCENE_WORDS + k] += (bits >> k) & 1u;
        cnt[(size_t)i * SCENE_WORDS + SCENE_SUM] += ad;
        cnt[(size_t)i * SCENE_WORDS + SCENE_BY] |= hb;
      }
    }
  }
  out.resize(c.n);
  for (int i = 0; i < c.n; ++i) {
    const unsigned* s = &cnt[(size_t)i * SCENE_WORDS];
    out[i] = Rec{{s[SC_MODEL], s[SC_VISIBLE], s[SC_MODEL] - s[SC_VISIBLE], s[SC_SEEN], s[SC_INLIER], s[SC_FRONT], s[SC_BEHIND], s[SCENE_SUM],
                  s[SCENE_BY], (unsigned)c.tol, (unsigned)c.n, 0u}};
  }
  return 0;
}

// every pixel inside a rectangle (whole: every pixel of the frame) exactly once, no pixel twice, and the planned tiles are all there are
static int check_cover(const Case& c, bool whole, const std::vector<int>& visits, const ScenePlan& plan) {
  bool any = false;
  for (int y = 0; y < c.H; ++y)
    for (int x = 0; x < c.W; ++x) {
      bool in_union = whole;
      for (int i = 0; i < c.n && !in_union; ++i) {
        const int32_t* r = &c.rects[4 * i];
        in_union = x >= r[0] && x < r[2] && y >= r[1] && y < r[3];
      }
      const int v = visits[(size_t)y * c.W + x];
      CHECK(v <= 1 && (!in_union || v == 1));
      any = any || in_union;
    }
  if (!any) { CHECK(plan.tiles_x == 1 && plan.tiles_y == 1 && plan.x1 == plan.x0); return 0; }
  // no more tiles than the area needs: a tile less in either direction would leave a pixel of the area out
  CHECK((plan.tiles_x - 1) * SCENE_TILE_W < plan.x1 - plan.x0 && (plan.tiles_y - 1) * SCENE_TILE_H < plan.y1 - plan.y0);
  CHECK(plan.tiles_x * SCENE_TILE_W >= plan.x1 - plan.x0 && plan.tiles_y * SCENE_TILE_H >= plan.y1 - plan.y0);
  return 0;
}

static bool same(const Rec& r, const unsigned (&w)[SCENE_RECORD_WORDS]) { return std::memcmp(r.w, w, sizeof(w)) == 0; }

static int run(const Case& c, std::vector<Rec>& rec, std::vector<uint8_t>& ids_v, std::vector<uint16_t>& scene_v) {
  const size_t px = (size_t)c.H * c.W;
  uint8_t* ids = (uint8_t*)std::malloc(px);
  uint16_t* scene = (uint16_t*)std::malloc(px * 2);
  std::vector<int> visits;
  std::vector<Rec> rec_box;
  ScenePlan plan;
  int rc = replay(c, true, rec, ids, scene, visits, plan) || check_cover(c, true, visits, plan);
  if (!rc) rc = replay(c, false, rec_box, nullptr, nullptr, visits, plan) || check_cover(c, false, visits, plan);
  if (!rc && std::memcmp(rec.data(), rec_box.data(), sizeof(Rec) * c.n) != 0) { std::fprintf(stderr, "records differ between the two areas\n"); rc = 1; }
  ids_v.assign(ids, ids + px);
  scene_v.assign(scene, scene + px);
  std::free(ids);
  std::free(scene);
  return rc;
}

static int thresholds() {   // model depths 100 / 101 / 1999 / 2000, |o - m| at tol and tol + 1 on either side, observed invalid
  Case c{4, 8, 0, 10, {}, {}, alloc_u16(32, 700)};
  add_layer(c, 0, 0, 8, 4, 0);
  const int m0[8] = {100, 101, 1999, 2000, 500, 500, 500, 500}, o0[8] = {500, 111, 1989, 500, 510, 511, 490, 489};
  for (int x = 0; x < 8; ++x) { c.depth[0][x] = (uint16_t)m0[x]; c.observed[x] = (uint16_t)o0[x]; }
  c.depth[0][8] = 500; c.observed[8] = 100;
  c.depth[0][9] = 500; c.observed[9] = 2000;
  std::vector<Rec> r; std::vector<uint8_t> ids; std::vector<uint16_t> scene;
  CHECK(run(c, r, ids, scene) == 0);
  const unsigned want[12] = {8, 8, 0, 6, 4, 1, 1, 40, 0, 10, 1, 0};
  CHECK(same(r[0], want));
  CHECK(ids[0] == 0 && ids[1] == 1 && ids[2] == 1 && ids[3] == 0 && ids[8] == 1 && ids[10] == 0 && scene[2] == 1999 && scene[3] == 0);
  return 0;
}

static int ties() {   // two identical layers: layer 0 owns every pixel, layer 1 is all hidden behind it
  Case c{4, 8, 0, 10, {}, {}, alloc_u16(32, 605)};
  add_layer(c, 0, 0, 8, 4, 600);
  add_layer(c, 0, 0, 8, 4, 600);
  std::vector<Rec> r; std::vector<uint8_t> ids; std::vector<uint16_t> scene;
  CHECK(run(c, r, ids, scene) == 0);
  const unsigned w0[12] = {32, 32, 0, 32, 32, 0, 0, 160, 0, 10, 2, 0}, w1[12] = {32, 0, 32, 0, 0, 0, 0, 0, 1, 10, 2, 0};
  CHECK(same(r[0], w0) && same(r[1], w1));
  for (int q = 0; q < 32; ++q) CHECK(ids[q] == 1 && scene[q] == 600);
  return 0;
}

static int rectangles() {   // overlap, an empty layer, a 1 x 1 rectangle in the corner, a gap; neither side a multiple of the tile
  Case c{20, 70, 0, 10, {}, {}, alloc_u16(20 * 70, 655)};
  add_layer(c, 2, 1, 12, 6, 700);
  add_layer(c, 8, 3, 18, 9, 650);
  add_layer(c, 0, 0, 0, 0, 0);
  add_layer(c, 69, 19, 70, 20, 900);
  add_layer(c, 40, 0, 45, 2, 1500);
  std::vector<Rec> r; std::vector<uint8_t> ids; std::vector<uint16_t> scene;
  CHECK(run(c, r, ids, scene) == 0);
  const unsigned w[5][12] = {{50, 38, 12, 38, 0, 38, 0, 0, 2, 10, 5, 0}, {60, 60, 0, 60, 60, 0, 0, 300, 0, 10, 5, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 5, 0},
                             {1, 1, 0, 1, 0, 1, 0, 0, 0, 10, 5, 0}, {10, 10, 0, 10, 0, 10, 0, 0, 0, 10, 5, 0}};
  for (int i = 0; i < 5; ++i) CHECK(same(r[i], w[i]));
  int owned = 0;
  for (auto v : ids) owned += v != 0;
  CHECK(owned == 38 + 60 + 1 + 10 && ids[19 * 70 + 69] == 4 && ids[3 * 70 + 8] == 2 && ids[3 * 70 + 7] == 1 && ids[0] == 0);
  const ScenePlan p = plan_scene(c.n, c.rects.data(), c.H, c.W, false);
  CHECK(p.x0 == 2 && p.y0 == 0 && p.x1 == 70 && p.y1 == 20 && p.tiles_x == 3 && p.tiles_y == 3);
  return 0;
}

static int many_and_none() {   // 32 overlapping layers, each a step nearer: the last owns its whole rectangle; then every layer empty
  Case c{9, 45, 0, 5, {}, {}, alloc_u16(9 * 45, 0)};
  for (int i = 0; i < 32; ++i) add_layer(c, i, i / 8, i + 8, i / 8 + 5, 1000 - 10 * i);
  std::vector<Rec> r; std::vector<uint8_t> ids; std::vector<uint16_t> scene;
  CHECK(run(c, r, ids, scene) == 0);
  unsigned visible = 0;
  for (int i = 0; i < 32; ++i) {
    CHECK(r[i].w[0] == 40 && r[i].w[1] + r[i].w[2] == 40 && r[i].w[3] == 0 && r[i].w[10] == 32);
    CHECK((r[i].w[8] & ((1u << i) | ((1u << i) - 1u))) == 0);   // only a later (nearer) layer hides layer i
    visible += r[i].w[1];
  }
  const unsigned last[12] = {40, 40, 0, 0, 0, 0, 0, 0, 0, 5, 32, 0};
  CHECK(same(r[31], last) && r[0].w[8] != 0);
  unsigned owned = 0;
  for (auto v : ids) owned += v != 0;
  CHECK(owned == visible);
  Case e{5, 7, 0, 5, {}, {}, alloc_u16(35, 700)};
  add_layer(e, 0, 0, 0, 0, 0);
  add_layer(e, 3, 3, 3, 9, 0);
  CHECK(run(e, r, ids, scene) == 0);
  const unsigned zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 2, 0};
  CHECK(same(r[0], zero) && same(r[1], zero));
  for (auto v : ids) CHECK(v == 0);
  return 0;
}

static int tiles_and_stage() {
  // the row of every tile of the frames with the most tiles, the widest and the tallest grid
  const int frames[5][2] = {{1, 1 << 21}, {1 << 21, 1}, {2048, 1024}, {63550, 33}, {120, 160}};
  for (const auto& f : frames) {
    CHECK(scene_frame_ok(f[0], f[1]));
    const ScenePlan p = plan_scene(0, nullptr, f[0], f[1], true);
    CHECK((unsigned long long)p.tiles_x * p.tiles_y < (1ull << 19) && p.tiles_x <= (1 << 16));
    for (unsigned b = 0; b < (unsigned)(p.tiles_x * p.tiles_y); ++b) {
      int bx, by;
      scene_tile_of(p, b, bx, by);
      CHECK(by == (int)(b / (unsigned)p.tiles_x) && bx == (int)(b % (unsigned)p.tiles_x));
    }
  }
  CHECK(!scene_frame_ok(2048, 1025) && !scene_frame_ok(0, 5) && !scene_frame_ok(1 << 20, 1 << 20) && scene_frame_ok(1080, 1920));
  const int32_t out[4] = {0, 0, 9, 4}, neg[4] = {-1, 0, 3, 3}, ok[4] = {0, 0, 8, 4}, empty[4] = {5, 9, 5, 40};
  CHECK(!scene_rect_ok(out, 4, 8) && !scene_rect_ok(neg, 4, 8) && scene_rect_ok(ok, 4, 8) && scene_rect_ok(empty, 4, 8));
  // the staging of the host entry: every region written in full inside exactly `total` bytes, and read back unharmed
  for (int mode = 0; mode < 4; ++mode) {
    const int n = 3, H = 7, W = 13;
    const bool ids = mode & 1, scene = mode & 2;
    const SceneStage s = plan_scene_stage(n, H, W, ids, scene);
    unsigned char* buf = (unsigned char*)std::malloc(s.total);
    CHECK(s.up_bytes == (size_t)H * W * 2 && s.rec_off >= s.up_bytes && s.rec_off % 256 == 0);
    std::memset(buf, 1, s.up_bytes);
    std::memset(buf + s.rec_off, 2, (size_t)n * 48);
    if (ids) std::memset(buf + s.ids_off, 3, (size_t)H * W);
    if (scene) std::memset(buf + s.scene_off, 4, (size_t)H * W * 2);
    CHECK(buf[s.up_bytes - 1] == 1 && buf[s.rec_off] == 2 && buf[s.rec_off + n * 48 - 1] == 2);
    if (ids) CHECK(s.ids_off >= s.rec_off + n * 48 && buf[s.ids_off] == 3 && buf[s.ids_off + H * W - 1] == 3);
    if (scene) CHECK(s.scene_off % 2 == 0 && s.scene_off >= s.rec_off + n * 48 && buf[s.scene_off] == 4 && buf[s.total - 1] == 4);
    std::free(buf);
  }
  return 0;
}

// csrc/fit_rule.h against numbers written here
static int fit_rule() {
  const unsigned M = 1u << FC_MODEL, S = 1u << FC_SEEN, I = 1u << FC_INLIER, F = 1u << FC_FRONT, B = 1u << FC_BEHIND;
  CHECK(M == 1u && S == 2u && I == 4u && F == 8u && B == 16u && FC_COUNTS == 5);   // the order of se3tn_fit's fields
  // the eleven rows of literal_pair() of tests/test_fit_check_host.py (TOL = 7) as runs of {m, o, pixels}
  const int T = 7;
  const int rows[][3] = {{0, 500, 176}, {100, 500, 88}, {2000, 500, 88}, {65535, 500, 176}, {500, 0, 44}, {500, 100, 44}, {500, 2000, 44},
                         {500, 65535, 44}, {500, 500 + T, 176}, {500, 500 - T, 176}, {500, 500, 100}, {500, 499, 76}, {500, 500 - T - 1, 176},
                         {500, 500 + T + 1, 50}, {500, 1999, 126}, {101, 1999, 176}, {1999, 101, 176}};
  const unsigned want[2][6] = {{8 * 176, 7 * 176, 3 * 176, 2 * 176, 2 * 176, 2 * 176 * 7 + 76},                      // LITERAL
                               {8 * 176, 7 * 176, 4 * 176 + 50, 176, 126 + 176, 2 * 176 * 7 + 76 + (176 + 50) * 8}};   // at TOL + 1
  for (int w = 0; w < 2; ++w) {
    unsigned got[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (const auto& r : rows) {
      unsigned ad = 77u;
      const unsigned bits = fit_classify(r[0], r[1], T + w, ad);
      for (int k = 0; k < FC_COUNTS; ++k) got[k] += ((bits >> k) & 1u) * (unsigned)r[2];
      got[5] += ad * (unsigned)r[2];
    }
    CHECK(std::memcmp(got, want[w], sizeof(got)) == 0);
  }
  // the edges alone: {m, o, tol, bits, ad}.  Two valid depths differ by at most 1999 - 101 = 1898, so at tol = 65535 every seen
  // pixel is an inlier; 1898 and 1897 are the largest tolerances that |o - m| = tol and tol + 1 can meet
  const unsigned edges[][5] = {
      {100, 500, 65535, 0, 0}, {101, 500, 65535, M | S | I, 399}, {1999, 500, 65535, M | S | I, 1499}, {2000, 500, 65535, 0, 0}, {65535, 500, 65535, 0, 0},
      {500, 100, 65535, M, 0}, {500, 101, 65535, M | S | I, 399}, {500, 1999, 65535, M | S | I, 1499}, {500, 2000, 65535, M, 0}, {500, 65535, 65535, M, 0},
      {100, 500, 1, 0, 0},     {101, 500, 1, M | S | B, 0},       {1999, 500, 1, M | S | F, 0},        {2000, 500, 1, 0, 0},     {65535, 500, 1, 0, 0},
      {500, 100, 1, M, 0},     {500, 101, 1, M | S | F, 0},       {500, 1999, 1, M | S | B, 0},        {500, 2000, 1, M, 0},     {500, 65535, 1, M, 0},
      {500, 501, 1, M | S | I, 1}, {500, 499, 1, M | S | I, 1}, {500, 502, 1, M | S | B, 0}, {500, 498, 1, M | S | F, 0}, {500, 500, 1, M | S | I, 0},
      {101, 1999, 65535, M | S | I, 1898}, {1999, 101, 65535, M | S | I, 1898}, {101, 1999, 1898, M | S | I, 1898}, {1999, 101, 1898, M | S | I, 1898},
      {101, 1999, 1897, M | S | B, 0}, {1999, 101, 1897, M | S | F, 0}, {0, 0, 65535, 0, 0}, {65535, 65535, 65535, 0, 0}};
  for (const auto& e : edges) {
    unsigned ad = 77u;
    CHECK(fit_classify((int)e[0], (int)e[1], (int)e[2], ad) == e[3] && ad == e[4]);
    CHECK(depth_valid((int)e[0]) == ((e[3] & M) != 0u));
  }
  // scene_classify on an owned pixel: fit_classify with the visible bit inserted after model; a pixel of another owner: model and by
  const int d[6] = {0, 100, 101, 500, 1999, 2000}, tols[2] = {10, 1898};
  for (int tol : tols)
    for (int m : d)
      for (int o : d) {
        unsigned fa = 77u, sa = 77u, by = 77u;
        const unsigned f = fit_classify(m, o, tol, fa);
        const unsigned want_sc = f ? (f & 1u) | (1u << SC_VISIBLE) | ((f & ~1u) << 1) : 0u;
        CHECK(scene_classify(3, m, 3, o, tol, sa, by) == want_sc && sa == fa && by == 0u);
        CHECK(scene_classify(3, m, 5, o, tol, sa, by) == (f & 1u) && sa == 0u && by == (f ? 1u << 5 : 0u));
      }
  return 0;
}

int main() {
  if (thresholds() || ties() || rectangles() || many_and_none() || tiles_and_stage() || fit_rule()) return 1;
  std::puts("scene_fit_check: ok");
  return 0;
}
