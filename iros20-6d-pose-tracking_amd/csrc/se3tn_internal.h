// Internal definitions shared by the host-side weight packer and the gfx950 kernels.
// Network geometry follows se3_tracknet.py:52-112 of the reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/se3tracknet.h"
#include "scene_fit_plan.h"   // the scene kernel's rule, tiles and counter words
#include "infer_plan.h"   // network geometry, ConvId / conv_specs, the planned steps the conv launchers execute

namespace se3tn {

// ---------------------------------------------------------------------------------------------
// Packed weight blob (float32 words).  One contiguous allocation so that multi-GPU start-up is a
// single RCCL broadcast.  3x3 convolutions are stored as the MFMA "A" operand panels
//   [chunk = Cin/32][tap = r*3+s][Cout][32]        (BN folded, see weights.cpp)
// i.e. for every K-step (chunk,tap) a [Cout][32] row-major tile whose rows are the K-contiguous
// runs a lane reads with one ds_read_b128.  Stems: [Cout = 64][204], k = pair*8 + half*4 + c
// (tap pairing: weights.cpp pack_stem / stem7x7_mfma.hip).
// ---------------------------------------------------------------------------------------------
struct BlobLayout {
  // offsets in float32 words
  size_t stem_w;   // [2 branches][64][204]
  size_t stem_b;   // [2][64]
  size_t conv_w[NUM_CONV3];
  size_t conv_b[NUM_CONV3];
  size_t fc_w;     // [2 heads][3][512]
  size_t fc_b;     // [2][4] (3 used)
  size_t total;    // words, incl. the 64-word header
};

constexpr int HEADER_WORDS = 64;
constexpr uint32_t BLOB_MAGIC = 0x53453354u;  // 'SE3T'
constexpr uint32_t BLOB_VERSION = 7;  // 7: float32 panels only (54 MB); the f16x3 split panels are derived on the device

// f16x3 mode: the same panels as "split rows" (32 x f16 hi | 32 x f16 lo of w * 2^k per cout) and the per-cout 2^-k.
// NOT part of the blob (since v7): a context-owned device buffer derived from the bound blob by launch_split_weights when
// SE3TN_PREC_F16X3 is first selected -- like the Winograd planes, so the RCCL broadcast carries the float32 panels only.
struct SplitLayout {
  size_t stem_ws;  // [2][64][204] words, each 16-byte (pair, half) entry = 4 f16 hi | 4 f16 lo
  size_t stem_sc;  // [2][64] per-cout 2^-k
  size_t conv_ws[NUM_CONV3];
  size_t conv_sc[NUM_CONV3];
  size_t total;    // words
};

inline BlobLayout blob_layout() {
  BlobLayout L{};
  size_t o = HEADER_WORDS;
  L.stem_w = o; o += (size_t)2 * 64 * 204;
  L.stem_b = o; o += 2 * 64;
  const Conv3* s = conv_specs();
  for (int i = 0; i < NUM_CONV3; ++i) {
    L.conv_w[i] = o; o += conv3_words(s[i].cin, s[i].cout) * s[i].groups;
    L.conv_b[i] = o; o += (size_t)s[i].cout * s[i].groups;
  }
  L.fc_w = o; o += 2 * 3 * 512;
  L.fc_b = o; o += 2 * 4;
  o = (o + 63) & ~(size_t)63;
  L.total = o;
  return L;
}

inline SplitLayout split_layout() {
  SplitLayout L{};
  size_t o = 0;
  L.stem_ws = o; o += (size_t)2 * 64 * 204;
  L.stem_sc = o; o += 2 * 64;
  const Conv3* s = conv_specs();
  for (int i = 0; i < NUM_CONV3; ++i) {
    L.conv_ws[i] = o; o += conv3_words(s[i].cin, s[i].cout) * s[i].groups;
    L.conv_sc[i] = o; o += (size_t)s[i].cout * s[i].groups;
  }
  o = (o + 63) & ~(size_t)63;
  L.total = o;
  return L;
}

// Exponent k of the exact per-cout power-of-two weight scaling of the f16x3 mode: the largest |w| of a cout row lands in
// [2^10, 2^11) (k = floor(10 - log2(mx)), evaluated on the float's own exponent so that host and device agree bit for bit).
__host__ __device__ inline int split_exponent(float mx) {
  if (!(mx > 0.f)) return 0;
  int e;
  const float m = frexpf(mx, &e);  // mx = m 2^e, m in [0.5, 1)
  int k = (m == 0.5f) ? 11 - e : 10 - e;
  if (k > 40) k = 40;
  if (k < -20) k = -20;
  return k;
}

// ---------------------------------------------------------------------------------------------
// kernel argument blocks
// ---------------------------------------------------------------------------------------------
// All conv activations are NHWC with a one-pixel zero border: a tensor of interior size H x W is
// stored as [n][H+2][W+2][ld] (+ PAD_SLACK_PX pixels of slack after the last image, the slab DMA
// rounds its run up to 8 pixels).
constexpr int PAD_SLACK_PX = 8;
// The network input (one 16-byte RGBD pixel) is stored with a 3-pixel zero border: [n,182,182,4]
// (+ IN_SLACK_ROWS rows of slack: the stem's slab DMA always fetches 13 rows).
constexpr int IN_PAD = 3;
constexpr int IN_P = RES + 2 * IN_PAD;  // 182
constexpr int IN_SLACK_ROWS = 6;
// (SMALL_MAX_IMG, the most pairs a launch of the batch 1-5 kernel family takes: infer_plan.h)
// Mixed-model launches of the batch 1-5 family (se3tn_on_track_objects): image i of a launch reads every weight / bias / FC tensor
// img_off[i] floats away from the launch's own pointers (all blobs share one layout, so one offset per image serves every tensor),
// and its pose update takes tn[i] / rn[i].  The offset is looked up once per workgroup from the image index of blockIdx (a scalar
// load); the kernels take it through a template switch, so the single-model instantiations are the code they were.
struct ImgParams {
  long long off[SMALL_MAX_IMG];
  double tn[SMALL_MAX_IMG], rn[SMALL_MAX_IMG];
};
struct ConvArgs {
  const float* in;    // padded NHWC, `in_ld` floats per pixel; channel offset already applied
  const float* w;     // packed panels of group 0
  const float* bias;  // folded bias of group 0
  const float* res;   // residual (geometry of out) or nullptr
  float* out;         // padded NHWC
  int in_ld, res_ld, out_ld;
  int H, W, Ho, Wo;   // input / output INTERIOR spatial size
  int M;              // n * Ho * Wo  (GEMM rows = output pixels)
  int tiles_n;        // Cout / BN
  int groups;         // independent convolutions in this launch
  int in_gs, res_gs, out_gs, bias_gs;  // per-group strides (floats)
  long long w_gs;
  // small-batch split-K path (conv3x3_splitk_kernel): partial-sum workspace, 0 slices = not used
  float* part;
  size_t part_bytes;
  int slices;
  int reserved[2];            // unused.  The words keep img_off (below) at its offset: the per-image conv_reduce kernels address that table
                              // through vector immediates, which a shorter struct would change (profiles/EXPERIMENTS.md item 80)
  // f16x3 mode: per-cout power-of-two weight scale (acc * wscale = true sum), overflow flag,
  // fast = 0 (f32 everywhere) | 1 | 2 (see launch_conv3x3)
  const float* wscale;
  int* overflow;
  int fast;
  // mixed-model batch (batch 1-5 family only): per_img != 0 => image i reads w / bias at img_off[i] floats from them (ImgParams)
  int per_img = 0;
  long long img_off[SMALL_MAX_IMG] = {};
};

// Winograd F(m x m,3x3) path of the stride-1 256/512-channel convs at large batch (wino_mfma.hip)
struct WinoArgs {
  const float* in;    // padded NHWC input, channel offset of group 0 applied
  const float* U;     // transformed weights of group 0: [chunk][nf][Cout][32]
  const float* bias;
  const float* res;   // residual or nullptr
  float* out;         // padded NHWC
  float* V;           // workspace [groups][nf][T][C]     (transformed input tiles)
  float* Mw;          // workspace [groups][nf][T][Cout]  (per-frequency products)
  int in_ld, res_ld, out_ld;
  int H, W;           // interior size (input == output, stride 1)
  int m, nf;          // output tile edge (2 | 4), nf = (m+2)^2 frequencies
  int th, tw;         // m x m output tiles per image: ceil(H/m), ceil(W/m)
  int n, T;           // images, T = n * th * tw
  int C, Cout, groups;
  int in_gs, res_gs, out_gs, bias_gs;
  long long u_gs;     // floats per group of U
  // f16x3 mode of the fused F(4x4) blocks (split != 0): in / res / out are split-row tensors, V is written as split rows, U points
  // at the split planes and uscale[g][f][Cout] holds their exact power-of-two scales (undone in the GEMM epilogue, M is float32)
  int split;
  const float* uscale;
  int* overflow;
};

// outputs of the fused out-transform + avg-pool + FC + tanh (wino_tail_kernel)
struct TailArgs {
  const float* fc_w;  // [2 heads][3][512]
  const float* fc_b;  // [2][4]
  float* logits;      // [n,6] pre-tanh
  float* fcpart;      // [n][2 heads][8 channel slices][3] partial FC dot products
  float* trans;       // [n,3] or nullptr
  float* rot;         // [n,3] or nullptr
  const double* poseA;  // [n,16] or nullptr
  double* poseB;
  double tn, rn;
};

struct CropArgs {  // one launch handles up to MAX crops
  static constexpr int MAX = 64;  // 64 x 56 B + constants = 3.75 KB of kernel arguments (limit 4 KB, asserted below)
  se3tn_crop c[MAX];
  double mean[8], stdv[8];
  float* out;   // plain [n,176,176,4], or (padded != 0) the interior of [n,182,182,4]
  float* out2;  // crops n_first.. go here, numbered from 0 (image A and image B of a frame in ONE launch: se3tn_on_track); else unused
  int n_first;  // (n when out2 is unused)
  int n;
  int padded;
  int split;    // f16x3 mode: a pixel is stored as 4 x f16 hi | 4 x f16 lo (same 16 bytes)
  int offset_rule;  // SE3TN_OFFSET_RULE_*: how `depth -= z` rounds (NumPy 1.x: one float32 operation; NumPy 2: float64, rounded once)
  int* overflow;
  // nullptr: every crop normalises with mean / stdv above.  Otherwise a DEVICE table [n_first][16] (mean[8] | std[8] per object):
  // crop i normalises with row (i < n_first ? i : i - n_first) -- several models' crops in one launch (se3tn_on_track_objects)
  const double* norm = nullptr;
  // non-null: crop i < n_first also stores its raw pixels (crop_bbox alone, what launch_crop_raw writes) as image i of raw_rgb
  // [n_first,176,176,3] / raw_depth [n_first,176,176] -- image A of the full-frame route, in the launch that normalises it
  uint8_t* raw_rgb = nullptr;
  uint16_t* raw_depth = nullptr;
};

static_assert(sizeof(CropArgs) <= 4096, "CropArgs travels as kernel arguments: HIP's limit is 4 KB");

// depth record, or depth AND colour record in one pass, of up to MAX (model, observed) pairs per launch (fit_stats.hip); the
// descriptors travel as kernel arguments
struct FitArgs {
  static constexpr int MAX = SE3TN_FIT_MAX_PAIRS;   // 2 x 32 x 56 B + constants = 3.6 KB of kernel arguments (limit 4 KB, asserted below)
  static constexpr int SUMS = 6, WORDS = 8;          // depth only: the six sums of se3tn_fit; counter words per pair: the SUMS | the arrival counter | unused
  static constexpr bool SCENE = false;              // (FitSceneArgs below: true -- what fit_launches in api.cpp branches on)
  static constexpr int COLOUR_SUMS = 24, COLOUR_WORDS = 32;   // with colour: + sum_m .. sum_abs of se3tn_color_fit (px = inlier_px); the same layout
  se3tn_crop m[MAX], o[MAX];  // model / observed image of pair i: depth, H, W, left .. bottom are read (rgb: with colour or raw_rgb only)
  unsigned* counters;         // [n][WORDS] or (colour) [n][COLOUR_WORDS], zero between launches (the last workgroup of a pair to arrive re-arms them)
  se3tn_fit* fit;             // [n] depth records: device memory, or mapped pinned host memory (each word stored once); with colour: or nullptr
  int tol;
  // non-null (depth only): pair i also stores the raw crop of its MODEL image (crop_bbox alone, what launch_crop_raw writes) as image
  // i of raw_rgb [n,176,176,3] / raw_depth [n,176,176] -- the estimate render of the full-frame route, in the launch that scores it
  uint8_t* raw_rgb = nullptr;
  uint16_t* raw_depth = nullptr;
  se3tn_color_fit* colour = nullptr;   // non-null: [n] colour records as well (the COLOUR instantiation, its own counters)
};
static_assert(sizeof(FitArgs) <= 4096, "FitArgs travels as kernel arguments: HIP's limit is 4 KB");
static_assert(sizeof(se3tn_color_fit) == 80 && sizeof(se3tn_fit) == 32, "the records are 20 / 8 words");
hipError_t launch_fit_stats(const FitArgs& a, int n, hipStream_t st);

// both records under the scene-aware rule (fit_rule.h: fit_classify_scene) of up to MAX (model, observed, scene) triples per launch:
// fit_stats_kernel<true, true>.  A third descriptor per pair would push FitArgs past the 4 KB of kernel arguments at 32 pairs, so the
// scene instantiation has its own arguments with SE3TN_FIT_SCENE_MAX_PAIRS pairs; the members the kernel body shares keep FitArgs' names
struct FitSceneArgs {
  static constexpr int MAX = SE3TN_FIT_SCENE_MAX_PAIRS;   // 3 x 16 x 56 B + constants = 2.7 KB of kernel arguments (limit 4 KB, asserted below)
  static constexpr bool SCENE = true;
  static constexpr int SUMS = FitArgs::COLOUR_SUMS + 1;   // the 24 of the colour instantiation | hidden; the ticket follows: 26 of COLOUR_WORDS
  se3tn_crop m[MAX], o[MAX];  // as FitArgs (rgb and depth are read)
  se3tn_crop s[MAX];          // the scene of pair i -- the composed depth of the tracked objects: depth, H, W, left .. bottom are read
  unsigned* counters;         // [n][FitArgs::COLOUR_WORDS], the colour instantiation's own words: the layout is shared, word 24 is zero between launches
  se3tn_fit* fit;             // [n] depth records, the last word = hidden_px; or nullptr
  int tol;
  se3tn_color_fit* colour;    // [n] colour records
};
static_assert(sizeof(FitSceneArgs) <= 4096, "FitSceneArgs travels as kernel arguments: HIP's limit is 4 KB");
static_assert(FitSceneArgs::SUMS + 1 <= FitArgs::COLOUR_WORDS, "25 sums and the ticket fit the colour counters of a pair");
hipError_t launch_fit_stats(const FitSceneArgs& a, int n, hipStream_t st);

// n depth layers of one frame through a shared depth test (scene_fit.hip; the rule: scene_fit_rule.h, tiles and counters: scene_fit_plan.h);
// the layers travel as kernel arguments
struct SceneArgs {
  static constexpr int MAX = SCENE_MAX_LAYERS;   // 32 x 24 B + constants = 0.9 KB of kernel arguments
  SceneLayer l[MAX];          // layer i: device depth sub-image and its rectangle (empty: no pixels)
  const uint16_t* observed;   // [H,W] millimetres
  int H, W, n, tol;
  ScenePlan plan;             // the area the tiles cover
  unsigned* counters;         // [SCENE_COUNTER_WORDS], zero between launches (the last workgroup to arrive re-arms them)
  struct se3tn_scene_fit* out;       // [n] records: device memory, or mapped pinned host memory (each word stored once)
  uint8_t* ids;               // [H,W] or nullptr (then plan must cover the whole frame)
  uint16_t* scene;            // [H,W] or nullptr
};
static_assert(sizeof(SceneArgs) <= 4096 && SceneArgs::MAX == SE3TN_SCENE_MAX_OBJECTS, "SceneArgs travels as kernel arguments: HIP's limit is 4 KB");
static_assert(sizeof(struct se3tn_scene_fit) == 4 * SCENE_RECORD_WORDS, "the record is 12 words");
hipError_t launch_scene_fit(const SceneArgs& a, hipStream_t st);

// ADD / ADD-S of one chunk of pose pairs (pose_errors.hip; the index arithmetic is pose_errors_plan.h)
struct PoseErrArgs {
  const double* pts;    // [P,3] model points
  int P;
  const double* pred;   // [.,16] row-major poses of the chunk's FIRST pair onwards (rows 0-2 are read)
  const double* gt;
  double* part;         // [PE_CHUNK][tiles][2] partial sums of this chunk
  double* add;          // [count] results of the chunk, or nullptr
  double* adds;         // [count] or nullptr: the all-pairs loop is skipped
};
hipError_t launch_pose_errors(const PoseErrArgs& a, int count, hipStream_t st);

// n candidate poses against one depth frame (pose_search.hip; key, geometry and staging: pose_search_plan.h)
struct PoseScoreArgs {
  const double* pts;       // [P,3] model points
  int P;
  const double* poses;     // [n,16] row-major candidates (rows 0-2 are read)
  const uint16_t* depth;   // [H,W] millimetres
  int H, W;
  double K[9];             // row-major intrinsics: [0], [2], [4], [5] are read
  int tol;                 // millimetres
  se3tn_point_fit* out;    // [n] records, every word stored once
};
hipError_t launch_pose_score(const PoseScoreArgs& a, int n, hipStream_t st);
// the indices of the k largest keys of n records, descending, into idx; top_fit (or nullptr) receives those k records
hipError_t launch_pose_rank(const se3tn_point_fit* fit, int n, int k, int32_t* idx, se3tn_point_fit* top_fit, hipStream_t st);

// n_rot x n_trans candidate poses [R_r | t_t] against one depth frame (pose_grid.hip; tiling, LDS and staging: pose_grid_plan.h)
struct PoseGridArgs {
  const double* pts;       // [P,3] model points
  const double* nrm;       // [P,3] model normals (read with facing only)
  int P;
  const double* rots;      // [n_rot,9] row-major 3x3
  const double* trans;     // [n_trans,3]
  int n_trans;
  const uint16_t* depth;   // [H,W] millimetres
  int H, W;
  double K[9];             // row-major intrinsics: [0], [2], [4], [5] are read
  int tol;                 // millimetres
  int facing;              // 0 | 1
  se3tn_point_fit* out;    // [n_rot * n_trans] records, every word stored once
  const uint16_t* scene;   // NULL, or [H,W] millimetres, the composed depth of the tracked objects: the scene-aware rule, and `out`
                           // holds se3tn_scene_point_fit records (word 7 = hidden_pts).  Last: the plain kernels' arguments stay put
};
hipError_t launch_pose_grid(const PoseGridArgs& a, int n_rot, hipStream_t st);

// n poses aligned to one depth frame, all iterations in one launch (pose_align.hip; geometry and staging: pose_align_plan.h, the
// arithmetic: pose_align_math.h)
struct PoseAlignArgs {
  const double* pts;       // [P,3] model points
  const double* nrm;       // [P,3] model normals
  int P;
  const double* poses;     // [n,16] row-major hypotheses (rows 0-2 are read)
  const uint16_t* depth;   // [H,W] millimetres
  int H, W;
  double K[9];             // row-major intrinsics: [0], [2], [4], [5] are read
  se3tn_align_params p;
  double* poses_out;       // [n,16]; may be `poses`
  se3tn_align_rec* rec;    // [n]
  int64_t* sums;           // [n,28] or nullptr
  const uint16_t* scene;   // NULL, or [H,W] millimetres, the composed depth of the tracked objects: the scene-aware rule, and `rec`
  int scene_tol;           // holds se3tn_scene_align_rec records (hidden_pts at offset 28).  Last: the plain kernel's arguments stay put
};
hipError_t launch_pose_align(const PoseAlignArgs& a, int n, hipStream_t st);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies per DEVICE: a launcher remembers which device
// ordinals it has already raised the limit on (several contexts on different GPUs in one process).
struct PerDeviceOnce {
  bool done[64] = {};
  // returns the flag of the calling thread's current device (nullptr if the ordinal cannot be read)
  bool* current() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    return &done[dev];
  }
};
// raises a kernel's dynamic-LDS limit to `lds` bytes, once per device; `once` belongs to that kernel (a function-local static)
template <typename K>
inline hipError_t set_lds(K kern, size_t lds, PerDeviceOnce& once) {
  bool* done = once.current();
  if (done && *done) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess && done) *done = true;
  return e;
}

// launchers (defined in the .hip files)
// f16x3 split panels + per-cout scales of every conv / both stems from the bound float32 blob (kernels_misc.hip)
hipError_t launch_split_weights(const float* blob, const BlobLayout& L, float* split, const SplitLayout& S, hipStream_t st);
// split rows + per-(frequency, cout) scales of one group's Winograd planes U [chunk][nf][cout][32] (f16x3 Winograd blocks)
hipError_t launch_split_wino_u(const float* U, float* Us, float* scale, int cin, int cout, int nf, hipStream_t st);
// NCHW [n,4,176,176] (nchw != 0) or plain NHWC [n,176,176,4] -> interior of the padded [n,182,182,4]
hipError_t launch_to_padded_input(const float* in, float* out, int n, int nchw, int split, int* overflow,
                                  hipStream_t st);
hipError_t launch_preprocess(const CropArgs& a, hipStream_t st);
hipError_t launch_crop_raw(const se3tn_crop& c, uint8_t* rgb_out, uint16_t* depth_out, hipStream_t st);
// wscale != nullptr selects the f16x3 stem (split pixels, split weights w)
hipError_t launch_stem(const float* inA, const float* inB, const float* w, const float* bias,
                       const float* wscale, float* out, int n, hipStream_t st);
// split_out != 0: write split rows (f16 hi | f16 lo) for the f16x3 mode
hipError_t launch_maxpool(const float* in, float* out, int n, int split_out, int* overflow, hipStream_t st);
// conv3x3: executes the planned step (SMALL64 .. GATHER; its slice count, whether it reduces them); cin/cout/stride select the
// instantiation; epi: 0 bias+relu, 1 bias+res+relu, 2 bias+selu.  hipErrorInvalidValue: no kernel of that algorithm for the shape
hipError_t launch_conv3x3(const ConvArgs& a, const ConvStep& step, int cin, int cout, int stride, int epi, hipStream_t st);
// Winograd F(m x m,3x3): U = G g G^T (float64, rounded once) from the packed direct weights
// [chunk][9][cout][32] -> [chunk][(m+2)^2][cout][32]; launch_wino_conv = input transform + nf x groups
// batched MFMA GEMMs + output transform with the conv epilogue (epi 0 | 1)
hipError_t launch_wino_weights(const float* packed, float* U, int cin, int cout, int m, hipStream_t st);
hipError_t launch_wino_conv(const WinoArgs& a, const GemmPlan& gemm, int epi, hipStream_t st);
// fused Winograd F(2x2,3x3) of a 64 -> 64 channel convolution on the 44 x 44 maps (wino64_fused.hip); U: F(2x2) planes of launch_wino_weights
hipError_t launch_wino64(const float* in, int in_ld, int in_gs, const float* U, long long u_gs, const float* bias, int bias_gs,
                         const float* res, int res_ld, int res_gs, float* out, int out_ld, int out_gs, int n, int groups, int epi,
                         hipStream_t st);
// a whole residual block on the Winograd F(4x4) path with the fused mid / tail transforms (wino_mfma.hip);
// mark_after_mid: optional profiling hook called between conv1 and conv2 (returns non-zero on error)
hipError_t launch_wino_block(const WinoArgs& c1, const GemmPlan& gemm, const float* U2, const float* uscale2, const float* bias2, float* out2, int keep_mid,
                             float* keep_out2, const TailArgs* tl, hipStream_t st, int mark_after_mid(void*), void* mark_ctx);
// stem + max-pool of both branches in one launch at batch 1-2 (stem_pool_small.hip)
hipError_t launch_stem_pool_small(const float* inA, const float* inB, const float* w, const float* bias, float* pool, int n, hipStream_t st);
// the 64 -> 64 trunk convs at batch 1-5 without a K split (conv64_small.hip)
hipError_t launch_conv64_small(const ConvArgs& a, int n, int epi, hipStream_t st);
// the 128 .. 512-channel convs at batch 1-5: 128 pixels x 32 couts x one channel slice with all nine taps per workgroup
// (conv_slices_small.hip); partial sums for conv_reduce_kernel (the slice count per shape: infer_plan.h conv_slices_small_count)
hipError_t launch_conv_slices_small(const ConvArgs& a, int cin, int stride, hipStream_t st);
// stem + max-pool with a per-image weight offset table (ImgParams::off; nullptr = the single-model kernel)
hipError_t launch_stem_pool_small_multi(const float* inA, const float* inB, const float* w, const float* bias, float* pool, int n,
                                        const long long* img_off, hipStream_t st);
hipError_t launch_tail(const float* head, const float* fc_w, const float* fc_b, float* logits,
                       float* trans, float* rot, const double* poseA, double* poseB, double tn,
                       double rn, int n, hipStream_t st, float* fcpart, int* arrive, int* done_flag = nullptr, int done_seq = 0);
// the same fed by the 8 partial-sum slices of the last head conv at batch 1-5 (no conv_reduce launch in between); fcpart [n][64][3]
hipError_t launch_tail_parts(const float* part, int slices, size_t slice_stride, int M, const float* bias, const float* res, int res_ld,
                             const float* fc_w, const float* fc_b, float* logits, float* trans, float* rot, const double* poseA,
                             double* poseB, double tn, double rn, int n, hipStream_t st, float* fcpart, int* arrive, int* done_flag = nullptr,
                             int done_seq = 0, int ch = 16, const ImgParams* img = nullptr);
// padded [n,h+2,w+2,c] NHWC interior -> [n,c,h,w]
// split != 0: the source holds split rows (32 f16 hi | 32 f16 lo per 32-channel chunk)
hipError_t launch_padded_nhwc_to_nchw(const float* in, float* out, int n, int h, int w, int c, int split,
                                      hipStream_t st);

// rasteriser (raster.hip)
constexpr double R_NEAR_D = 0.1, R_FAR_D = 2.0;   // vispy_renderer.py:139-140, offscreen_renderer.py znear / zfar
// per-instance uniforms of a BATCHED rasteriser launch (grid.y = instance: n poses of one mesh in four launches, se3tn_on_track_batch)
struct RasterInstance {
  float PV[16];
  float light[3];
  float _pad;
  double dA, dB;
  // RasterArgs::inst_mesh != 0 (several meshes in one launch, se3tn_on_track_objects): this instance's mesh and its counts
  const float *verts, *normals, *colors;
  const int* faces;
  int V, F;
  int rect[4];   // RasterArgs::scissor != 0: this instance's rectangle sx0, sy0, sx1, sy1 (GL window coordinates; may be empty)
};
// per-instance material of a batched mode-1 launch with several meshes (RasterArgs::inst_mesh == 2, se3tn_on_track_objects on
// SE3TN_ROUTE_FRAME): what RasterArgs uv .. kd hold for a single mesh.  The table of a launch of n instances is
// [n x RasterInstance | n x RasterMaterial] in one allocation (one upload).  Only raster_resolve_kernel reads the materials.
// tex == nullptr: the instance's vertex colours are the base colour (textured and un-textured instances share a launch)
struct RasterMaterial {
  const float* uv;
  const uint8_t* tex;
  int tw, th, tlevels;
  float kd[3];
  unsigned tex_off[16];
};
struct RasterArgs {
  const RasterInstance* inst;  // nullptr: one instance, uniforms below.  Otherwise instance b = blockIdx.y takes PV / light / dA / dB from
                               // inst[b] and its scratch / outputs at b x (V | 1 + F | rw rh) elements behind the pointers below
  const float* verts;    // [V,3] object space
  const float* normals;  // [V,3]
  const float* colors;   // [V,3] in [0,1]
  const int* faces;      // [F,3]
  float4* vpost;         // [V] scratch: post-transform clip position (x, y, (z + w) / 2, w)
  int4* vsnap;           // [V] scratch: window X, Y in 1 / 2^sub_bits pixel, bits of z / w, bits of 1 / w
  unsigned long long* zbuf;  // [rw*rh] scratch: (sortable z << 32 | triangle)
  int* big;              // [1 + F] queue of triangles with large bounding boxes (big[0] = count)
  int* clipq;            // [1 + F] queue of triangles that cross the frustum
  uint8_t* rgb;          // out [rh,rw,3]
  uint16_t* depth;       // out [rh,rw] millimetres
  float PV[16];          // the shader's proj * view (mode 1: u_pv), row-major
  float light[3];        // light_direction in object space
  double dA, dB;         // mode 0: projection_matrix[2,2], [3,2] as vispy_renderer.py:163-164 reads them (float64)
  int numpy_rule;        // SE3TN_OFFSET_RULE_*: the NumPy generation's scalar casting in vispy_renderer.py:165-169
  int sub_bits;          // sub-pixel bits of the window coordinates (4 | 8)
  int V, F;
  int rw, rh;            // output resolution (176 x 176 for the Vispy-style window, the camera frame in pyrender mode)
  int mode;              // 0: VispyRenderer (Lambert shader, window crop)   1: pyrender (ambient only, full frame)
  const float* uv;       // mode 1: [V,2] texture coordinates or nullptr
  const uint8_t* tex;    // mode 1: RGB uint8 mip pyramid or nullptr (then the vertex colours are the base colour)
  int tw, th, tlevels;
  unsigned tex_off[16];  // byte offset of every mip level
  float kd[3];           // base colour factor (mtl Kd)
  int inst_mesh = 0;     // batched launch: 1 = every instance brings its own mesh (RasterInstance verts .. F); V / F above are then
                         // the LARGEST counts (grid and scratch strides), and threads past their own instance's counts exit
                         // 2 (mode 1 only) = and its own material: instance b shades with the RasterMaterial b that follows the
                         // launch's RasterInstance records (uv .. kd above are then unused) -- the resolve kernel's InstMat instantiation
  // scissor != 0 (mode 1, se3tn_render_frame_rect): only the pixels [sx0, sx1) x [sy0, sy1) of the rw x rh window (GL window coordinates:
  // row 0 at the BOTTOM) are cleared, covered and resolved; zbuf / rgb / depth hold that rectangle tightly packed, spx pixels per
  // instance (>= the area of every rectangle of the launch).  0: the whole window (the kernels set the rectangle themselves)
  int scissor = 0;
  int sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
  int spx = 0;
};
hipError_t launch_raster(const RasterArgs& a, hipStream_t st, int instances = 1);

// depth hole filling (depth_fill.hip)
struct FillDepthArgs {
  const uint16_t* depth_mm;  // [H,W]
  int H, W;
  double max_depth;          // metres
  int extrapolate;
  int blur;                  // SE3TN_BLUR_*
  double sigma_color, sigma_space;
  float *buf0, *buf1, *buf2; // [H,W] float32 scratch
  unsigned* minmax;          // [2]
  float* lut;                // [4098]
  uint16_t* out_mm;          // [H,W] or nullptr
  float* out_m;              // [H,W] or nullptr
};
hipError_t launch_fill_depth(const FillDepthArgs& a, hipStream_t st);
void launch_fill_depth_to_median(const FillDepthArgs& a, hipStream_t st, float** median, float** spare);
void bilateral_space_taps(double sigma_space, float w[12]);   // cv2.bilateralFilter's 12 space weights of the radius-2 disc

// the same on a rectangle of the frame (depth_fill_fused.hip): the chain up to the median in one tiled launch over the whole frame
// (extrapolate != 0: the launches above), then blur + invert-back + uint16 on the pixels asked for only.  out_mm / out_m unused.
struct FillDepthRectArgs {
  FillDepthArgs f;
  int cx0, cy0, cx1, cy1;    // pixels the last pass computes: [cy0, cy1) x [cx0, cx1), inside the frame, not empty
  uint16_t* out_full;        // [H,W]: every computed pixel at its place in the frame, or nullptr
  uint16_t* out_sub;         // [sy1 - sy0, sx1 - sx0] tightly packed: the computed pixels inside [sy0, sy1) x [sx0, sx1), or nullptr
  int sx0, sy0, sx1, sy1;
};
hipError_t launch_fill_depth_rect(const FillDepthRectArgs& a, hipStream_t st);

// n rectangles of ONE frame behind one run of the chain.  The rectangles travel as kernel arguments, MAX per launch (as CropArgs)
struct FillRectTable {
  static constexpr int MAX = 64;   // 64 x 24 B + constants = 1.5 KB of kernel arguments
  int n = 0;
  int full = -1;                   // this entry writes out_full (the whole frame), not out_base + off
  int x0[MAX], y0[MAX], w[MAX], h[MAX];
  long long off[MAX];              // uint16 elements from out_base
};
static_assert(sizeof(FillRectTable) <= 2048, "FillRectTable travels as kernel arguments beside the taps and pointers: HIP's limit is 4 KB");
struct FillDepthRectsArgs {
  FillDepthArgs f;
  int n;
  const int32_t* rects;      // host [n,4] {x0, y0, x1, y1}: inside the frame, or empty (x1 <= x0 or y1 <= y0: skipped)
  const size_t* offs;        // host [n]: where rectangle i goes, tightly packed, in uint16 elements from out_base
  uint16_t* out_base;
  uint16_t* out_full;        // [H,W]: the whole frame as well, or nullptr
};
hipError_t launch_fill_depth_rects(const FillDepthRectsArgs& a, hipStream_t st);

// host-side packer (weights.cpp)
struct HostTensor {
  const float* data;
  int64_t shape[4];
  int ndim;
};

}  // namespace se3tn
