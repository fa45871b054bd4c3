// The swizzled LDS row tile of the matrix kernels, stated once.  No HIP include: this header compiles for the host too, where
// tests/c_abi/lds_rows_check.cpp holds the two sides of the contract below against each other (tests/test_lds_rows_host.py).
//
// Every MFMA kernel keeps its operands in LDS as ROWS of 32 floats = 128 bytes = eight 16-byte SLOTS: one row per pixel / Winograd
// tile / cout, holding the 32 channels of one K chunk in eight logical channel BLOCKS of 4 floats.
//   * Why a swizzle.  The tiles arrive by LDS-DMA (global_load_lds_dwordx4), whose LDS image is lane-linear: rows cannot be padded.
//     A fragment read (ds_read_b128) has 32 lanes read the same logical block of 32 consecutive rows, 128 bytes apart: unswizzled
//     that is one bank group for all of them.  So physical slot s of row r holds logical block s ^ row_key(r), row_key(r) =
//     (r >> 1) & 7: sixteen consecutive rows spread a block over all eight slots, two rows per slot.
//   * The layout is a contract with two sides, and a kernel whose sides disagree still runs and returns wrong numbers:
//       STAGING side: the XOR is applied to the DMA *source*: the thread that fills physical slot s of row r fetches block
//         slot_block(r, s) of that row (stage_src: its float offset in a row-major [rows][32] source tile);
//       FRAGMENT side: the XOR is applied to the ds_read_b128 address: the lane that wants logical block b of row r reads
//         slot_off(r, b) floats into the row.  Of the four 8-k groups G of a 32x32x2 K-step, lane half hh takes block 2 G + hh
//         (frag_off); the 16x16x4 form (conv64_small.hip) has lane quarter q take blocks q and 4 + q.
//   * The key of row base + r equals the key of r whenever base is a multiple of 16: every tile and wave-tile base in the kernels
//     is a multiple of 32 rows, so a lane computes its four fragment offsets once from its row inside the 32 x 32 block (lane_frag).
//     Rows of a slab or patch (one row per input pixel, read at a per-tap offset) are keyed by their own index instead.
//   * A split row (f16x3 mode, mfma_common.h: 32 x f16 hi | 32 x f16 lo) has the same size, slots and swizzle: slots 0-3 = hi
//     channels 0-31, slots 4-7 = lo, and the four 8-k groups ARE (hi kb0, hi kb1, lo kb0, lo kb1).
#pragma once

#if defined(__HIPCC__)
#define SE3TN_HD __host__ __device__
#else
#define SE3TN_HD
#endif
// inlined before anything else is optimised: the kernels' address arithmetic then folds as if the expression stood in place
#define SE3TN_ALWAYS_INLINE inline __attribute__((always_inline))

namespace se3tn {
namespace lds_rows {

constexpr int ROW_FLOATS = 32, SLOT_FLOATS = 4, SLOTS = 8;

// (the macro is the same statement as plain tokens, for the few address expressions that the compiler folds into other
// instructions when the key reaches them through a call)
#define SE3TN_ROW_KEY(row) (((row) >> 1) & 7)
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int row_key(int row) { return SE3TN_ROW_KEY(row); }

// staging: the logical channel block that belongs in physical slot `slot` of row `row` ...
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int slot_block(int row, int slot) { return slot ^ row_key(row); }
// ... and its float offset inside a row-major [rows][32] source tile
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int stage_src(int row, int slot) { return row * ROW_FLOATS + (slot_block(row, slot) << 2); }

// fragments: float offset inside row `row` at which logical block `block` lies (key_off: for a caller that reads several
// blocks of one row and keeps key = row_key(row)) ...
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int key_off(int key, int block) { return (block ^ key) << 2; }
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int slot_off(int row, int block) { return key_off(row_key(row), block); }
// ... and that of lane half hh's operand of 8-k group G (= (8 G) ^ slot_off(row, hh))
SE3TN_HD SE3TN_ALWAYS_INLINE constexpr int frag_off(int row, int G, int hh) { return slot_off(row, 2 * G + hh); }

// The four frag_off of lane (l31, hh) for rows base + l31, base % 16 == 0.  Spelled high bits | low bit -- G ^ (key >> 1) and
// hh ^ (key & 1) -- and kept as four scalars: the form the K-loops were tuned with (an array indexed by the group changes the
// compiler's unrolling).  SE3TN_FRAG_OFF selects one by a literal group.
struct LaneFrag { int o0, o1, o2, o3; };
SE3TN_HD SE3TN_ALWAYS_INLINE LaneFrag lane_frag(int l31, int hh) {
  const int X = row_key(l31);
  const int lo = (hh ^ (X & 1)) * 4, xk = X >> 1;
  return LaneFrag{((0 ^ xk) << 3) + lo, ((1 ^ xk) << 3) + lo, ((2 ^ xk) << 3) + lo, ((3 ^ xk) << 3) + lo};
}
#define SE3TN_FRAG_OFF(F, G) ((G) == 0 ? (F).o0 : (G) == 1 ? (F).o1 : (G) == 2 ? (F).o2 : (F).o3)

}  // namespace lds_rows
}  // namespace se3tn
