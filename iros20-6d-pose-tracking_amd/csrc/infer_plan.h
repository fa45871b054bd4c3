// Host-only: WHICH kernel runs for WHICH conv of one forward pass (se3tn_infer, and the mixed-model call of se3tn_on_track_objects),
// decided before anything is enqueued.  plan_infer() maps an InferConfig -- the batch, every switch and every readiness bit the route
// depends on, and nothing else -- to an InferPlan; api.cpp fills the config from the context and executes the plan, the launchers in the
// .hip files dispatch on its steps.  The ten convs and their buffers are stated once, in conv_table().  No HIP in here, so a plain host
// program can include it (tests/c_abi/infer_plan_check.cpp walks the grid of configurations under ASan + UBSan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/se3tracknet.h"

namespace se3tn {

// Network geometry follows se3_tracknet.py:52-112 of the reference.
constexpr int RES = SE3TN_RES;  // 176
constexpr int S1 = 88;          // after the 7x7 s2 stems
constexpr int S2 = 44;          // after maxpool 3x3 s2
constexpr int S3 = 22;          // after convAB1 (s2)
constexpr int S4 = 11;          // after {trans,rot}_conv1 (s2)

struct Conv3 {
  int cin, cout, groups;  // weights of `groups` independent convs stored back to back
};
constexpr size_t conv3_words(int cin, int cout) { return (size_t)9 * cin * cout; }

enum ConvId {
  L64_1 = 0,  // convA2.conv1 | convB2.conv1     (2 groups, 64->64)
  L64_2,      // convA2.conv2 | convB2.conv2     (2 groups)
  L64_3,      // convB3.conv1
  L64_4,      // convB3.conv2
  LAB1,       // convAB1 128->256 s2
  LAB2_1,     // convAB2.conv1 256->256
  LAB2_2,     // convAB2.conv2
  LH1,        // trans_conv1 | rot_conv1 fused along Cout: 256->1024 s2
  LH2_1,      // trans_conv2.conv1 | rot_conv2.conv1   (2 groups, 512->512)
  LH2_2,      // trans_conv2.conv2 | rot_conv2.conv2   (2 groups)
  NUM_CONV3
};

inline const Conv3* conv_specs() {
  static const Conv3 s[NUM_CONV3] = {
      {64, 64, 2},   {64, 64, 2},   {64, 64, 1},   {64, 64, 1},  {128, 256, 1},
      {256, 256, 1}, {256, 256, 1}, {256, 1024, 1}, {512, 512, 2}, {512, 512, 2}};
  return s;
}

// ---- the ten convs, once ---------------------------------------------------------------------------------------------------------------
// the activation buffers se3tn_debug_buffer hands out, as bits of se3tn_ctx::written
enum : unsigned { STAGE_STEM = 1, STAGE_POOL = 2, STAGE_T64 = 4, STAGE_Q64 = 8, STAGE_AB = 16, STAGE_AB_T = 32, STAGE_HEAD = 64,
                  STAGE_HEAD_T = 128 };
// BUF_HEAD_OUT: the float32 map of the last head conv -- `head` itself, or in f16x3 mode `head_f` (head holds split rows, and the in-place
// residual update cannot change format)
enum BufId : uint8_t { BUF_NONE = 0, BUF_POOL, BUF_T64, BUF_Q64, BUF_AB, BUF_AB_T, BUF_HEAD, BUF_HEAD_T, BUF_HEAD_OUT };
struct TensorRef {
  BufId buf;
  int ch, ld, gs;   // channel offset into the buffer, floats per pixel, floats between the groups of the launch
};
struct ConvRow {
  ConvId id;
  TensorRef in, res, out;
  int hin, stride, epi;   // input map size; epi: 0 bias+relu, 1 bias+res+relu, 2 bias+selu
  const char* name;       // base profile name (step_label adds the algorithm)
};
// 64-channel trunk: pool = a0|b0 ; t64 scratch ; q64 = a1|b1 -> a1|b2 (== torch.cat((a,b),1)); then convAB1, the 256-channel
// ResnetBasicBlock, the two heads' stride-2 conv (fused along Cout) and their 512-channel blocks (2 groups)
inline const ConvRow* conv_table() {
  static const ConvRow t[NUM_CONV3] = {
      {L64_1, {BUF_POOL, 0, 128, 64}, {BUF_NONE, 0, 0, 0}, {BUF_T64, 0, 128, 64}, S2, 1, 0, "conv64 A2.conv1|B2.conv1"},
      {L64_2, {BUF_T64, 0, 128, 64}, {BUF_POOL, 0, 128, 64}, {BUF_Q64, 0, 128, 64}, S2, 1, 1, "conv64 A2.conv2|B2.conv2"},
      {L64_3, {BUF_Q64, 64, 128, 0}, {BUF_NONE, 0, 0, 0}, {BUF_T64, 64, 128, 0}, S2, 1, 0, "conv64 B3.conv1"},
      {L64_4, {BUF_T64, 64, 128, 0}, {BUF_Q64, 64, 128, 0}, {BUF_Q64, 64, 128, 0}, S2, 1, 1, "conv64 B3.conv2"},
      {LAB1, {BUF_Q64, 0, 128, 0}, {BUF_NONE, 0, 0, 0}, {BUF_AB, 0, 256, 0}, S2, 2, 2, "convAB1 s2"},
      {LAB2_1, {BUF_AB, 0, 256, 0}, {BUF_NONE, 0, 0, 0}, {BUF_AB_T, 0, 256, 0}, S3, 1, 0, "convAB2.conv1"},
      {LAB2_2, {BUF_AB_T, 0, 256, 0}, {BUF_AB, 0, 256, 0}, {BUF_AB, 0, 256, 0}, S3, 1, 1, "convAB2.conv2"},
      {LH1, {BUF_AB, 0, 256, 0}, {BUF_NONE, 0, 0, 0}, {BUF_HEAD, 0, 1024, 0}, S3, 2, 2, "trans|rot conv1 s2"},
      {LH2_1, {BUF_HEAD, 0, 1024, 512}, {BUF_NONE, 0, 0, 0}, {BUF_HEAD_T, 0, 1024, 512}, S4, 1, 0, "trans|rot conv2.conv1"},
      {LH2_2, {BUF_HEAD_T, 0, 1024, 512}, {BUF_HEAD, 0, 1024, 512}, {BUF_HEAD_OUT, 0, 1024, 512}, S4, 1, 1, "trans|rot conv2.conv2"}};
  return t;
}
// the Winograd block a conv belongs to: 0 = the 256-channel block (convAB2), 1 = the 512-channel heads, -1 = none
inline int wino_block_of(ConvId id) { return (id == LAB2_1 || id == LAB2_2) ? 0 : (id == LH2_1 || id == LH2_2) ? 1 : -1; }

// ---- thresholds (each with the measurement it came from) ---------------------------------------------------------------------------
// batch 1-5 kernel family: most pairs a launch takes (stem + pool, trunk convs, channel-slice convs, and so the per-image tables)
#ifndef SE3TN_SLICES_SMALL_MAX_N
#define SE3TN_SLICES_SMALL_MAX_N 5   // up to this many pairs the 128 .. 512-channel convs take conv_slices_small_kernel (0: never)
#endif
constexpr int SMALL_MAX_IMG = 5;
static_assert(SE3TN_SLICES_SMALL_MAX_N <= SMALL_MAX_IMG, "the per-image tables hold SMALL_MAX_IMG entries");
#ifndef SE3TN_STEM_SMALL_MAX_N
#define SE3TN_STEM_SMALL_MAX_N 5     // stem + max-pool of both branches in one launch (stem_pool_small.hip)
#endif
#ifndef SE3TN_CONV64_SMALL_MAX_N
#define SE3TN_CONV64_SMALL_MAX_N 5   // the trunk convs of up to this many pairs take conv64_small_kernel (0: never).  Measured 2 vs 5:
                                     // 8.6k -> 9.6k / 10.2k -> 11.0k / 10.8k -> 11.2k pairs/s at 3 / 4 / 5 pairs (one stream)
#endif
// Split-K is used when the big-tile grid would leave most of the 256 CUs idle and the partial-sum workspace is large enough.
// slices = the largest divisor of the K-step count (cin / 32 x 9) that leaves every workgroup >= SE3TN_SPLITK_MIN_STEPS K-steps and
// the launch <= 512 workgroups (two per CU).  Up to SE3TN_SPLITK_FIXED_MAX_N images the workgroup count is taken from the ONE-image
// geometry -- 6 / 12 / 24 / 24 / 48 slices of 3 steps for the 64-ch / convAB1 / convAB2 / trans|rot conv1 / conv2 layers -- so the
// slice count is a function of the layer (the same summation order for one pair alone or two together); larger batches count the
// real grid (fewer, longer slices), so from 3 pairs on a pair's last bits may depend on the batch it travels in -- as they do across
// the algorithm switches at 6 / 14 pairs, and in the reference under cuDNN.
#ifndef SE3TN_SPLITK_MIN_STEPS
#define SE3TN_SPLITK_MIN_STEPS 3   // measured at batch 1: 2 -> 280 us, 3 -> 268 us, 4 -> 276 us per forward (whole chunks before: 321 us)
#endif
#ifndef SE3TN_SPLITK_MAX_WGS
#define SE3TN_SPLITK_MAX_WGS 512
#endif
#ifndef SE3TN_SPLITK_FIXED_MAX_N
#define SE3TN_SPLITK_FIXED_MAX_N 2  // (5 = up to the Winograd threshold was measured: 15 % slower at n = 4 -- 4 x the partial sums of 48 slices)
#endif
// (SE3TN_WINOGRAD_* / SE3TN_TRUNK_WINOGRAD_*: include/se3tracknet.h, they are part of the public surface)

// ---- what the route depends on --------------------------------------------------------------------------------------------------------
// one bit per derived weight set: a set that is missing or stale makes its algorithm fall back, never fail (except the f16x3 panels,
// without which SE3TN_PREC_F16X3 has no kernel at all)
enum : unsigned {
  READY_WINO_VM = 1,      // the V / M workspaces exist
  READY_U2 = 2,           // wino_u holds the F(2x2) planes ...
  READY_U4 = 4,           // ... or the F(4x4) planes (one of the two)
  READY_U6 = 8,           // the F(6x6) planes are current
  READY_TRUNK = 16,       // the trunk's fused F(2x2) planes are current
  READY_SPLIT_W = 32,     // the f16x3 panels are current
  READY_SPLIT_U4 = 64     // the split F(4x4) planes are current
};
// Compared as a whole where a captured launch sequence is looked up (api.cpp GraphKey): zero it (memset) before filling it
struct InferConfig {
  int n;
  int prec;                  // SE3TN_PREC_*
  int keep_intermediates;
  int small_kernels;
  int small_family;          // the mixed-model call: the batch 1-5 family chosen EXPLICITLY -- a shape or batch it does not cover is an
                             // error, not another algorithm (the bits must equal each model's batch-1 run)
  int tail_parts, tail_parts_ch;
  int wino_min_batch, wino_tile, auto_tile_override[2];
  int wino_fuse;
  int gemmp;                 // persistent 128 x 256 GEMM: -1 = when its tiles fill every CU twice, 0 = never, 1 = whenever the shape allows
  int wino64_min_batch, wino64_min_fill;
  int num_cus;               // compute units of the device (0: 256)
  unsigned ready;            // READY_*
  size_t part_bytes;         // partial-sum workspace (0: none)
  double tn, rn;
};

struct GemmPlan {
  enum Kind : uint8_t { NONE = 0, ROWS96, ROWS128, PERSISTENT };
  Kind kind = NONE;
  int tiles = 0, grid = 0;   // PERSISTENT: 128 x 256 tiles in all, workgroups that walk them
};
struct ConvStep {
  enum Algo : uint8_t { NONE = 0, SMALL64, SLICES, SPLITK, SLAB, GATHER, WINO, WINO64 };
  Algo algo = NONE;
  bool reduce = true;   // SLICES / SPLITK: the conv adds its slices itself (conv_reduce_kernel).  false: the output map is NOT written,
                        // the partial sums are left to the tail (tail_parts_kernel)
  int tile = 0;         // WINO: F(tile x tile, 3x3)
  int slices = 0;       // SLICES / SPLITK: partial-sum slices
  GemmPlan gemm;        // WINO
};
struct InferPlan {
  enum Stem : uint8_t { STEM_BIG = 0, STEM_SMALL };        // stem7x7_mfma + maxpool | both in one launch of small tiles (map not stored)
  enum Tail : uint8_t { TAIL_PLAIN = 0, TAIL_PARTS, TAIL_FUSED };   // tail_kernel | tail_parts_kernel on the slices | the heads' block
  Stem stem = STEM_BIG;
  Tail tail = TAIL_PLAIN;
  bool block[2] = {false, false};   // the residual block runs as ONE fused launch sequence (launch_wino_block)
  bool tail_stores_word = false;    // the tail stores se3tn_on_track's completion word (the fused heads' tail never does)
  int tail_ch = 16;                 // TAIL_PARTS: channels per workgroup
  unsigned written = 0;             // STAGE_* the sequence writes
  ConvStep conv[NUM_CONV3];
};
enum InferPlanStatus { INFER_PLAN_OK = 0, INFER_PLAN_NO_SPLIT_PANELS, INFER_PLAN_FAMILY_MISS };

// ---- the rules ------------------------------------------------------------------------------------------------------------------------
// The tile the 256 / 512-channel blocks of a batch of n pairs run with.  F(6x6) exists in float32 only (SE3TN_PREC_F16X3 keeps F(4x4)
// and its fused head block on split operands) and pays from 14 pairs on (scripts/tile_sweep.sh: 0.511 vs 0.462 ms at n = 6, 0.701 vs
// 0.718 at n = 16, 1.76 vs 1.86 at n = 64): SE3TN_WINOGRAD_TILE_AUTO switches there.  With tile 6 | AUTO selected both U sets are
// resident: the F(4x4) planes in wino_u, the F(6x6) planes in wino_u6.
// which: 0 = the 256-channel block (convAB2), 1 = the 512-channel heads
inline int tile_for(const InferConfig& c, int which) {
  const int t = c.wino_tile;
  if (t == 2 || t == 4) return t;
  if (c.prec == SE3TN_PREC_F16X3) return 4;
  if (t == 6) return 6;
  if (t == SE3TN_WINOGRAD_TILE_6_4) return which == 0 ? 6 : 4;
  if (c.auto_tile_override[which]) return c.auto_tile_override[which];   // developer switch: SE3TN_WINOGRAD_AUTO_TILE_AB2 / _HEADS
  if (c.n < SE3TN_WINOGRAD_TILE6_MIN_BATCH) return 4;
  // AUTO: F(6x6) where its rounding is cheap.  The heads' products feed the average pool + FC directly: F(6x6) there doubles the
  // logits' rounding error (1.3e-5 vs 6.0e-6 in the batched 30-degree closed loop), and the rotation logits reach the composed pose
  // multiplied by rot_normalizer -- with a large normaliser (YCBInEOAT's 30 degrees, predict.py:586) the heads stay on F(4x4)
  return (which == 0 || c.rn <= SE3TN_WINOGRAD_HEADS_TILE6_MAX_ROT) ? 6 : 4;
}
inline bool wino_planes_ready(const InferConfig& c, int tile) {
  return (c.ready & (tile == 6 ? READY_U6 : tile == 4 ? READY_U4 : tile == 2 ? READY_U2 : 0u)) != 0;
}
inline bool wino_on(const InferConfig& c) { return c.wino_min_batch > 0 && c.n >= c.wino_min_batch && (c.ready & READY_WINO_VM); }

// The fused trunk kernel occupies a CU per workgroup (126 KB of LDS) for ~52 us whatever the batch: it beats the direct kernels when
// its 4 n groups workgroups fill the rounds of the CUs to more than half (measured, scripts/trunk_sweep.sh -> profiles/r03f_trunk_sweep.txt:
// n = 64 -> 2 | 1 rounds, 108 | 56 us vs 155 | 80 us direct; n = 20 grouped = 0.63 round 53 vs 80; but n = 16 grouped and n = 32 single
// = half a round 52 vs 45; the direct kernels step from one round of their own tiles to two at n = 17 grouped / n = 34 single).
inline bool wino64_pays(const InferConfig& c, int groups) {
  if (c.wino64_min_batch <= 0 || c.n < c.wino64_min_batch) return false;
  const long wgs = 4L * c.n * groups, rounds = (wgs + c.num_cus - 1) / c.num_cus;
  return 100 * wgs >= (long)c.wino64_min_fill * rounds * c.num_cus;   // the rounds are at least min_fill % full
}

// ResnetBasicBlocks of 256 / 512 channels: at n >= wino_min_batch with F(4x4) or F(6x6) the whole block runs through launch_wino_block
// (conv1's out-transform fused with conv2's in-transform; the heads' last out-transform fused with avg-pool + FC + tanh); otherwise
// conv by conv.  f16x3 mode: the batched GEMMs of the 256-channel block are bandwidth-bound at the f16 matrix rate (41 FLOP per byte of
// V / M traffic) and lose to the direct f16x3 kernels (0.247 vs 0.220 ms at batch 64); the 512-channel heads win (0.349 vs 0.427 ms)
inline bool block_fused(const InferConfig& c, int which) {
  const bool fast = c.prec == SE3TN_PREC_F16X3;
  const int bt = tile_for(c, which);
  const bool planes_ready = bt == 6 ? (!fast && wino_planes_ready(c, 6)) : (bt == 4 && wino_planes_ready(c, 4));
  return c.wino_fuse && wino_on(c) && planes_ready && (!fast || (c.ready & READY_SPLIT_U4)) && !(which == 0 && fast);
}

// channel slices of conv_slices_small_kernel per layer shape (0: the family has no kernel for it)
inline int conv_slices_small_count(int cin, int stride, int H) {
  if (cin == 128 && stride == 2 && H == S2) return 4;
  if (cin == 256 && stride == 1 && H == S3) return 8;
  if (cin == 256 && stride == 2 && H == S3) return 8;
  if (cin == 512 && stride == 1 && H == S4) return 8;
  return 0;
}

// split-K slices of one conv of M output rows (0: the big-tile kernel): the comment at SE3TN_SPLITK_MIN_STEPS above
inline int pick_slices(const InferConfig& c, int M, int hw, int cin, int cout, int groups, int big_tile_rows, int bn_big) {
  const int big_blocks = ((M + big_tile_rows - 1) / big_tile_rows) * (cout / bn_big) * groups;
  if (big_blocks >= 200 || c.part_bytes == 0) return 0;
  const int bn = cout >= 128 ? 128 : 64;
  const int rows = M <= SE3TN_SPLITK_FIXED_MAX_N * hw ? hw : M;          // one image's rows | the real grid
  const int base = ((rows + 127) / 128) * (cout / bn) * groups;          // workgroups per slice
  const int ks = cin / 32 * 9;
  const size_t per_slice = (size_t)groups * M * cout * sizeof(float);
  int best = 0;
  for (int sl = 1; sl <= ks; ++sl) {
    if (ks % sl != 0 || ks / sl < SE3TN_SPLITK_MIN_STEPS) continue;
    if (per_slice * sl > c.part_bytes) break;
    if (best > 0 && base * sl > SE3TN_SPLITK_MAX_WGS) break;
    best = sl;
  }
  return best;
}

// GEMM tiling of one Winograd conv: 128- or 96-row tiles, whichever leaves the shorter per-CU queue (in 32 x 32 x K blocks) on 256 CUs;
// or persistent 128 x 256 tiles, one 8-wave workgroup per CU: when they fill every CU at least twice (F(6x6) at batch 64: exactly 2.0)
// and the plane count lets the XCD-local tile order cover them (groups nf % 8 == 0: 36 F(4x4) planes do not).
// gemmp: -1 = that rule, 0 = never, 1 = whenever the shape allows (SE3TN_WINO_GEMMP at se3tn_create: A/B runs and the tests'
// bit-equality check of the two kernels on ragged shapes)
inline GemmPlan plan_gemm(const InferConfig& c, int T, int cout, int groups, int nf, bool split) {
  GemmPlan g;
  const long long per_b = (long long)(cout / 128) * groups * nf;
  const long long q128 = ((((T + 127) / 128) * per_b + 255) / 256) * 16;
  const long long q96 = ((((T + 95) / 96) * per_b + 255) / 256) * 12;
  g.kind = q96 < q128 ? GemmPlan::ROWS96 : GemmPlan::ROWS128;
  if (split || c.gemmp == 0 || cout % 256 != 0 || (groups * nf) % 8 != 0) return g;
  const int cus = c.num_cus > 0 ? c.num_cus : 256;
  const int tiles = (cout / 256) * ((T + 127) / 128) * groups * nf;
  // the automatic rule takes it for the plane sets it was measured on (EXPERIMENTS item 27): F(6x6).  The two-group F(4x4) heads
  // (72 planes, T = 576 at batch 64 = 4.5 row tiles) also pass the divisibility test above and would trade their exact-fit 96-row
  // tiling for it unmeasured: they keep the plain tiles unless gemmp == 1 forces it.
  const bool measured_shape = nf == 64;
  if (c.gemmp == 1 || (tiles >= 2 * cus && measured_shape)) {
    g.kind = GemmPlan::PERSISTENT;
    g.tiles = tiles;
    g.grid = tiles < cus ? tiles : (cus / 8) * 8;
  }
  return g;
}

// one conv outside a fused block.  may_leave_slices: the tail can take this conv's channel slices unreduced
inline InferPlanStatus plan_conv(const InferConfig& c, const ConvRow& r, bool may_leave_slices, ConvStep& s) {
  const Conv3& sp = conv_specs()[r.id];
  const bool fast = c.prec == SE3TN_PREC_F16X3;
  const int n = c.n, ho = (r.hin - 1) / r.stride + 1, M = n * ho * ho;
  s = ConvStep{};
  const bool conv64 = sp.cin == 64 && sp.cout == 64 && r.stride == 1 && r.hin == S2 && r.epi != 2;
  const int sl_small = conv_slices_small_count(sp.cin, r.stride, r.hin);
  const bool sl_fits = sl_small > 0 && (size_t)sl_small * sp.groups * M * sp.cout * sizeof(float) <= c.part_bytes;
  if (c.small_family) {   // nothing to fall through to
    if (fast || n < 1 || n > SE3TN_SLICES_SMALL_MAX_N || (conv64 ? n > SE3TN_CONV64_SMALL_MAX_N : !sl_fits)) return INFER_PLAN_FAMILY_MISS;
    s.algo = conv64 ? ConvStep::SMALL64 : ConvStep::SLICES;
    if (!conv64) { s.slices = sl_small; s.reduce = !may_leave_slices; }
    return INFER_PLAN_OK;
  }
  const int blk = wino_block_of(r.id);
  const int wtile = tile_for(c, blk > 0 ? 1 : 0);
  if (blk >= 0 && !fast && wino_on(c) && wino_planes_ready(c, wtile)) {
    const int th = (r.hin + wtile - 1) / wtile;
    s.algo = ConvStep::WINO;
    s.tile = wtile;
    s.gemm = plan_gemm(c, n * th * th, sp.cout, sp.groups, (wtile + 2) * (wtile + 2), false);
    return INFER_PLAN_OK;
  }
  if (r.id <= L64_4 && !fast && wino64_pays(c, sp.groups) && (c.ready & READY_TRUNK) && conv64) {
    s.algo = ConvStep::WINO64;
    return INFER_PLAN_OK;
  }
  if (!fast && c.small_kernels && conv64 && n <= SE3TN_CONV64_SMALL_MAX_N) {
    s.algo = ConvStep::SMALL64;
    return INFER_PLAN_OK;
  }
  // batch 1-5, float32: the wide convs as one round of 128-pixel x 32-cout x channel-slice workgroups (conv_slices_small.hip)
  if (!fast && c.small_kernels && n <= SE3TN_SLICES_SMALL_MAX_N && sl_fits) {
    s.algo = ConvStep::SLICES;
    s.slices = sl_small;
    s.reduce = !may_leave_slices;
    return INFER_PLAN_OK;
  }
  s.slices = pick_slices(c, M, ho * ho, sp.cin, sp.cout, sp.groups, r.stride == 1 ? 256 : 128, sp.cout >= 128 ? 128 : 64);
  s.algo = s.slices > 0 ? ConvStep::SPLITK : r.stride == 1 ? ConvStep::SLAB : ConvStep::GATHER;   // (the big-tile kernels: slab at stride 1, gather at 2)
  return INFER_PLAN_OK;
}

inline InferPlanStatus plan_infer(const InferConfig& c, InferPlan& p) {
  const bool fast = c.prec == SE3TN_PREC_F16X3, keep = c.keep_intermediates != 0;
  p = InferPlan{};
  if (fast && !(c.ready & READY_SPLIT_W)) return INFER_PLAN_NO_SPLIT_PANELS;
  if (c.small_family && (fast || c.n < 1 || c.n > SE3TN_STEM_SMALL_MAX_N)) return INFER_PLAN_FAMILY_MISS;
  // batch 1-5 (the per-frame regime): stem + max-pool of both branches in ONE launch of 16-pool-pixel tiles; the 88 x 88 x 128 stem
  // map is not stored, so a caller who asked for the intermediates gets the batch-64 pair
  p.stem = (c.small_family || (c.small_kernels && !fast && !keep && c.n <= SE3TN_STEM_SMALL_MAX_N)) ? InferPlan::STEM_SMALL : InferPlan::STEM_BIG;
  p.written = STAGE_POOL | STAGE_T64 | STAGE_Q64 | STAGE_AB | (p.stem == InferPlan::STEM_BIG ? STAGE_STEM : 0u);
  for (int b = 0; b < 2; ++b) p.block[b] = !c.small_family && block_fused(c, b);
  // batch 1-5 (conv_slices_small: 8 partial-sum slices per output) may leave the last head conv's slices to the tail -- no conv_reduce
  // launch, the final head map not written (se3tn_keep_intermediates keeps it)
  const bool tail_may_take = c.small_family || (c.tail_parts && !keep);
  const ConvRow* rows = conv_table();
  for (int i = 0; i < NUM_CONV3; ++i) {
    const int blk = wino_block_of(rows[i].id);
    ConvStep& s = p.conv[i];
    if (blk >= 0 && p.block[blk]) {
      const Conv3& sp = conv_specs()[rows[i].id];
      const int bt = tile_for(c, blk), th = (rows[i].hin + bt - 1) / bt;
      s.algo = ConvStep::WINO;
      s.tile = bt;
      s.gemm = plan_gemm(c, c.n * th * th, sp.cout, sp.groups, (bt + 2) * (bt + 2), fast);
    } else if (InferPlanStatus st = plan_conv(c, rows[i], rows[i].id == LH2_2 && tail_may_take, s)) {
      return st;
    }
  }
  if (!p.block[0] || keep) p.written |= STAGE_AB_T;
  if (!p.block[1] || keep) p.written |= STAGE_HEAD_T;
  const ConvStep& last = p.conv[LH2_2];
  p.tail = p.block[1] ? InferPlan::TAIL_FUSED : (last.algo == ConvStep::SLICES && !last.reduce) ? InferPlan::TAIL_PARTS : InferPlan::TAIL_PLAIN;
  if (p.block[1] ? keep : p.tail == InferPlan::TAIL_PLAIN) p.written |= STAGE_HEAD;
  p.tail_stores_word = p.tail != InferPlan::TAIL_FUSED;
  p.tail_ch = c.small_family ? 16 : c.tail_parts_ch;
  return INFER_PLAN_OK;
}

// ---- profile names ----------------------------------------------------------------------------------------------------------------------
// Profile names say which ALGORITHM a launch took ("convAB2.conv1 [F(6x6)] fused block", "convAB1 s2 [slices]", "[slab f16x3]"): the tests
// assert from them that the path they mean to check is the one that ran.  String work: only ever called for a profiled call
inline std::string step_label(const ConvRow& r, const ConvStep& s, bool fast, bool in_block, bool fused_tail) {
  static const char* const tags[] = {"", "conv64 small", "slices", "split-K", "slab", "gather"};
  std::string name = r.name;
  if (in_block && fused_tail && r.id == LH2_2) name += " + avgpool+fc+tanh+pose";
  if (s.algo == ConvStep::WINO) {
    const std::string t = std::to_string(s.tile);
    return name + " [F(" + t + "x" + t + ")]" + (in_block ? " fused block" : "");
  }
  if (s.algo == ConvStep::WINO64) return name + " [fused F(2x2)]";
  if (s.algo == ConvStep::NONE) return name;
  return name + " [" + tags[s.algo] + (fast ? " f16x3]" : "]");
}
inline const char* stem_label(const InferPlan& p, int launch) {   // launch 0 | 1 (STEM_BIG only)
  return p.stem == InferPlan::STEM_SMALL ? "stem7x7 + maxpool [small tiles]" : launch == 0 ? "stem7x7_mfma" : "maxpool3x3s2";
}
inline const char* tail_label(const InferPlan& p) {   // (TAIL_FUSED: the heads' block carries it)
  return p.tail == InferPlan::TAIL_PARTS ? "tail slices+avgpool+fc+tanh+pose" : p.tail == InferPlan::TAIL_PLAIN ? "tail avgpool+fc+tanh+pose" : nullptr;
}

}  // namespace se3tn
