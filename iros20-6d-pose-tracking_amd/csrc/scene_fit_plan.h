// Host-only: the sizes and the grid of the scene kernel (scene_fit.hip), and where se3tn_scene_fit_host keeps its frame and its
// results in the staging buffer.  No HIP in here, so a plain host program can include it (tests/c_abi/scene_fit_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scene_fit_rule.h"

namespace se3tn {

// One workgroup of 256 threads per tile of 32 x 8 frame pixels, one thread per pixel: a wave holds two rows of 32 pixels, so its 64
// two-byte loads of a layer are two runs of 64 bytes
constexpr int SCENE_TILE_W = 32, SCENE_TILE_H = 8, SCENE_THREADS = SCENE_TILE_W * SCENE_TILE_H;
// Counter words per layer: the SC_COUNTS counts | sum |o - m| of the inliers | hidden_by.  SCENE_THREADS == SCENE_MAX_LAYERS *
// SCENE_WORDS: after the reduction one thread per (layer, word) adds its word
constexpr int SCENE_SUM = SC_COUNTS, SCENE_BY = SC_COUNTS + 1, SCENE_WORDS = SC_COUNTS + 2;
static_assert(SCENE_MAX_LAYERS * SCENE_WORDS == SCENE_THREADS, "one thread per (layer, counter word)");
// The context's counters: SCENE_MAX_LAYERS x SCENE_WORDS sums, then the arrival ticket (zero between launches)
constexpr int SCENE_TICKET = SCENE_MAX_LAYERS * SCENE_WORDS, SCENE_COUNTER_WORDS = SCENE_TICKET + 8;
constexpr int SCENE_RECORD_WORDS = 12;   // se3tn_scene_fit

inline bool scene_rect_empty(const int32_t r[4]) { return r[2] <= r[0] || r[3] <= r[1]; }
// a rectangle the kernel may be given: empty, or inside the frame
inline bool scene_rect_ok(const int32_t r[4], int H, int W) {
  return scene_rect_empty(r) || (r[0] >= 0 && r[1] >= 0 && r[2] <= W && r[3] <= H);
}
// H * W <= SCENE_MAX_PIXELS without forming a product that could overflow
inline bool scene_frame_ok(int H, int W) { return H >= 1 && W >= 1 && (unsigned long long)H * (unsigned long long)W <= SCENE_MAX_PIXELS; }

// The pixels the launch covers, [y0, y1) x [x0, x1), and its tiles.  whole_frame (ids or scene asked for: they are defined for every
// pixel of the frame): the frame.  Otherwise the bounding box of the rectangles that are not empty -- it covers their union; if every
// rectangle is empty the area is empty and ONE workgroup runs, which stores the all-zero records.
struct ScenePlan {
  int x0, y0, x1, y1;
  int tiles_x, tiles_y;   // >= 1 each
  // ceil(2^40 / tiles_x): tile b of the 1-D grid lies in tile row (b * inv_tiles_x) >> 40 -- an integer division without the float
  // reciprocal a compiler expands `/` into.  Exact for b * tiles_x < 2^40; a frame has at most 2^21 pixels, so b < 2^19 and
  // tiles_x <= 2^16 (tests/c_abi/scene_fit_check.cpp tries every b of the extreme frames)
  unsigned long long inv_tiles_x;
};
inline ScenePlan plan_scene(int n, const int32_t* rects /* [n,4] */, int H, int W, bool whole_frame) {
  ScenePlan p{0, 0, 0, 0, 1, 1, 0};
  if (whole_frame) { p.x1 = W; p.y1 = H; }
  else {
    bool any = false;
    for (int i = 0; i < n; ++i) {
      const int32_t* r = rects + 4 * (size_t)i;
      if (scene_rect_empty(r)) continue;
      if (!any) { p.x0 = r[0]; p.y0 = r[1]; p.x1 = r[2]; p.y1 = r[3]; any = true; continue; }
      p.x0 = r[0] < p.x0 ? r[0] : p.x0; p.y0 = r[1] < p.y0 ? r[1] : p.y0;
      p.x1 = r[2] > p.x1 ? r[2] : p.x1; p.y1 = r[3] > p.y1 ? r[3] : p.y1;
    }
  }
  if (p.x1 > p.x0 && p.y1 > p.y0) {
    p.tiles_x = (p.x1 - p.x0 + SCENE_TILE_W - 1) / SCENE_TILE_W;
    p.tiles_y = (p.y1 - p.y0 + SCENE_TILE_H - 1) / SCENE_TILE_H;
  }
  p.inv_tiles_x = ((1ull << 40) + (unsigned long long)p.tiles_x - 1) / (unsigned long long)p.tiles_x;
  return p;
}
// tile b of the 1-D grid -> its column and row of tiles (this and the next statement are what the kernel compiles of this header)
SE3TN_SC_HD inline void scene_tile_of(const ScenePlan& p, unsigned b, int& bx, int& by) {
  by = (int)(((unsigned long long)b * p.inv_tiles_x) >> 40);
  bx = (int)b - by * p.tiles_x;
}
// the frame pixel of thread t of tile (bx, by); the caller tests it against the plan's area
SE3TN_SC_HD inline void scene_thread_pixel(const ScenePlan& p, int bx, int by, int t, int& x, int& y) {
  x = p.x0 + bx * SCENE_TILE_W + (t & (SCENE_TILE_W - 1));
  y = p.y0 + by * SCENE_TILE_H + t / SCENE_TILE_W;
}

// se3tn_scene_fit_host's staging: [observed frame H W uint16 | pad | n records | ids H W uint8 | pad | scene H W uint16].  The upload is
// [0, up_bytes), the read-back [rec_off, total): ids and scene are laid out only when asked for
struct SceneStage {
  size_t up_bytes, rec_off, ids_off, scene_off, total;
};
inline SceneStage plan_scene_stage(int n, int H, int W, bool ids, bool scene) {
  auto a256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t px = (size_t)H * (size_t)W;
  SceneStage s{};
  s.up_bytes = px * 2;
  s.rec_off = a256(s.up_bytes);
  size_t end = s.rec_off + (size_t)n * SCENE_RECORD_WORDS * 4;
  s.ids_off = s.scene_off = 0;
  if (ids) { s.ids_off = a256(end); end = s.ids_off + px; }
  if (scene) { s.scene_off = a256(end); end = s.scene_off + px * 2; }
  s.total = end;
  return s;
}

}  // namespace se3tn
