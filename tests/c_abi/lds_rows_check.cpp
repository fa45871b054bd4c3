// Host check of the swizzled LDS row tile (csrc/lds_rows.h): the staging side (which source block a thread fetches into the
// physical slot it fills) against the fragment side (where a lane reads a logical block), for tiles of 32 .. 256 rows.
// Stand-alone: built with -fsanitize=address,undefined by tests/test_lds_rows_host.py, prints "lds_rows ok" and returns 0.
#include <cstdio>
#include <vector>

#include "lds_rows.h"

using namespace se3tn::lds_rows;

static int failures = 0;
#define CHECK(COND, ...)                                     \
  do {                                                       \
    if (!(COND)) {                                           \
      if (++failures <= 20) {                                \
        std::printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #COND); \
        std::printf(__VA_ARGS__);                            \
        std::printf("\n");                                   \
      }                                                      \
    }                                                        \
  } while (0)

// element (row, channel) of the source tile
static float src_value(int row, int channel) { return (float)(row * ROW_FLOATS + channel); }

// the emulated DMA: 16 bytes from float offset `from` of the row-major source into physical slot `slot` of LDS row `row`
static void dma16(std::vector<float>& lds, const std::vector<float>& src, int row, int slot, int from) {
  for (int e = 0; e < SLOT_FLOATS; ++e) lds.at(row * ROW_FLOATS + slot * SLOT_FLOATS + e) = src.at(from + e);
}

static void check_tile(int rows) {
  std::vector<float> src(rows * ROW_FLOATS);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < ROW_FLOATS; ++c) src[r * ROW_FLOATS + c] = src_value(r, c);

  // ---- staging, stated per row: the thread that fills slot s of row r reads at stage_src(r, s)
  std::vector<float> lds(rows * ROW_FLOATS, -1.f);
  for (int r = 0; r < rows; ++r) {
    unsigned seen = 0;
    for (int s = 0; s < SLOTS; ++s) {
      CHECK(stage_src(r, s) == r * ROW_FLOATS + slot_block(r, s) * SLOT_FLOATS, "rows %d r %d s %d", rows, r, s);
      CHECK((s ^ SE3TN_ROW_KEY(r)) == slot_block(r, s), "macro spelling, r %d s %d", r, s);
      dma16(lds, src, r, s, stage_src(r, s));
      seen |= 1u << slot_block(r, s);
    }
    CHECK(seen == 0xffu, "the slot map of row %d is no permutation: %#x", r, seen);
  }

  // ---- the workgroup maps of the kernels: NT threads, thread t -> slot t & 7 of rows (t >> 3) + RS j, RS = NT / 8, with ONE
  // block c4 / source offset per thread and the piece reached by adding RS rows to the base (weights) or to the row (pixels)
  for (int nt : {256, 512}) {
    const int RS = nt / 8;
    if (rows % RS != 0) continue;
    std::vector<float> img(rows * ROW_FLOATS, -1.f);
    for (int t = 0; t < nt; ++t) {
      const int r0 = t >> 3, slot = t & 7;
      const int c4 = slot_block(r0, slot), wvoff = stage_src(r0, slot);
      for (int j = 0; j < rows / RS; ++j) {
        const int row = r0 + RS * j;
        CHECK(wvoff + j * RS * ROW_FLOATS == stage_src(row, slot), "piece base: rows %d nt %d t %d j %d", rows, nt, t, j);
        CHECK(c4 == slot_block(row, slot), "one block per thread: rows %d nt %d t %d j %d", rows, nt, t, j);
        // LDS-DMA image is lane-linear: thread t of piece j lands at float (j RS 32 + 4 t)
        const int dst = j * RS * ROW_FLOATS + 4 * t;
        CHECK(dst == row * ROW_FLOATS + slot * SLOT_FLOATS, "lane-linear image: t %d j %d", t, j);
        // weight side: contiguous tile, piece j = base + j RS rows; pixel side: the row's own address + the thread's block
        CHECK(wvoff + j * RS * ROW_FLOATS == row * ROW_FLOATS + c4 * 4, "the two sides' sources: t %d j %d", t, j);
        dma16(img, src, row, slot, row * ROW_FLOATS + c4 * 4);
      }
    }
    CHECK(img == lds, "workgroup map of %d threads, %d rows", nt, rows);
  }
  // ---- the 8-row pieces of one wave (conv3x3_slab_kernel): lane l -> row 8 j + (l >> 3), slot l & 7, key in lane form
  {
    std::vector<float> img(rows * ROW_FLOATS, -1.f);
    for (int j = 0; j < rows / 8; ++j)
      for (int l = 0; l < 64; ++l) {
        const int row = 8 * j + (l >> 3), slot = l & 7;
        const int blk = j % 2 ? (slot ^ ((4 + (l >> 4)) & 7)) : (slot ^ ((l >> 4) & 7));
        CHECK(blk == slot_block(row, slot), "slab lane form: j %d lane %d", j, l);
        CHECK(j * 256 + 4 * l == row * ROW_FLOATS + slot * SLOT_FLOATS, "lane-linear piece: j %d lane %d", j, l);
        dma16(img, src, row, slot, row * ROW_FLOATS + blk * 4);
      }
    CHECK(img == lds, "8-row pieces, %d rows", rows);
  }

  // ---- fragments: lane (l31, hh) of a wave whose 32-row block starts at `base` reads channels 8 G + 4 hh .. + 3 of row base + l31
  for (int base = 0; base < rows; base += 32)
    for (int l31 = 0; l31 < 32; ++l31)
      for (int hh = 0; hh < 2; ++hh) {
        const LaneFrag fo = lane_frag(l31, hh);
        const int row = base + l31;
        const int o[4] = {SE3TN_FRAG_OFF(fo, 0), SE3TN_FRAG_OFF(fo, 1), SE3TN_FRAG_OFF(fo, 2), SE3TN_FRAG_OFF(fo, 3)};
        for (int G = 0; G < 4; ++G) {
          CHECK(o[G] == frag_off(row, G, hh), "lane_frag vs frag_off: row %d hh %d G %d", row, hh, G);
          CHECK(o[G] >= 0 && o[G] + 3 < ROW_FLOATS && o[G] % 4 == 0, "offset %d", o[G]);
          for (int e = 0; e < SLOT_FLOATS; ++e)
            CHECK(lds.at(row * ROW_FLOATS + o[G] + e) == src_value(row, 8 * G + 4 * hh + e), "rows %d row %d hh %d G %d e %d: %g",
                  rows, row, hh, G, e, (double)lds.at(row * ROW_FLOATS + o[G] + e));
        }
      }
  // rows keyed by their own index (slab and patch rows, any row, no 32-row block): frag_off and the kernels' spellings of it
  for (int row = 0; row < rows; ++row)
    for (int hh = 0; hh < 2; ++hh)
      for (int G = 0; G < 4; ++G) {
        const int off = frag_off(row, G, hh);
        CHECK(off == ((8 * G) ^ slot_off(row, hh)), "slab spelling: row %d hh %d G %d", row, hh, G);
        CHECK(off == key_off(row_key(row), 2 * G + hh), "key_off spelling: row %d hh %d G %d", row, hh, G);
        for (int e = 0; e < SLOT_FLOATS; ++e)
          CHECK(lds.at(row * ROW_FLOATS + off + e) == src_value(row, 8 * G + 4 * hh + e), "row %d hh %d G %d e %d", row, hh, G, e);
      }
  // the 16x16x4 form (conv64_small.hip): lane quarter q reads channels 4 q .. + 3 and 16 + 4 q .. + 3 = logical blocks q and 4 + q
  for (int row = 0; row < rows; ++row)
    for (int q = 0; q < 4; ++q)
      for (int half = 0; half < 2; ++half) {
        const int off = key_off(row_key(row), 4 * half + q);
        CHECK(off == slot_off(row, 4 * half + q), "row %d q %d", row, q);
        for (int e = 0; e < SLOT_FLOATS; ++e)
          CHECK(lds.at(row * ROW_FLOATS + off + e) == src_value(row, 16 * half + 4 * q + e), "16x16x4: row %d q %d half %d e %d", row, q,
                half, e);
      }
}

int main() {
  // the two spellings of a fragment offset agree for all arguments
  for (int key = 0; key < 8; ++key)
    for (int G = 0; G < 4; ++G)
      for (int hh = 0; hh < 2; ++hh) {
        const int xk = key >> 1;
        CHECK(((G ^ xk) << 3) + (hh ^ (key & 1)) * 4 == (((2 * G + hh) ^ key) << 2), "key %d G %d hh %d", key, G, hh);
        CHECK(key_off(key, 2 * G + hh) == (((2 * G + hh) ^ key) << 2), "key %d G %d hh %d", key, G, hh);
      }
  for (int row = 0; row < 4096; ++row) {
    CHECK(row_key(row) == ((row >> 1) & 7) && row_key(row) == SE3TN_ROW_KEY(row), "row %d", row);
    CHECK(row_key(row) == row_key(row % 16), "the key has period 16: row %d", row);
  }
  for (int rows : {32, 64, 128, 256}) check_tile(rows);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("lds_rows ok\n");
  return 0;
}
