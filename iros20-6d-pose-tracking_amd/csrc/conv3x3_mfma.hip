// 3x3 convolution (pad 1, stride 1|2) + folded-BN bias + {ReLU | residual+ReLU | SELU} as an
// im2col-free implicit GEMM on the gfx950 exact-f32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces every nn.Conv2d(k=3)+BatchNorm2d(+SELU/ReLU/+identity) of Se3TrackNet
// (se3_tracknet.py:59-76 via network_modules.py:59-66 ConvBNReLU, :86-120 ResnetBasicBlock).
//
// Common to both kernels below
//  * activations are NHWC float32 with a one-pixel ZERO BORDER kept in HBM ([n,H+2,W+2,C]): the
//    conv padding is data, there is no bounds logic anywhere on the operand path;
//  * GEMM rows = output pixels flattened over the batch, cols = Cout, K = (32-channel chunk) x tap,
//    walked chunk-major / tap-minor (weights are packed [chunk][tap][Cout][32] on the host);
//  * MFMA operand roles are SWAPPED (A-operand = weight rows, B-operand = pixel rows): a lane of the
//    accumulator holds ONE pixel x 4 runs of 4 consecutive couts, so bias / residual / activation /
//    store are float4 traffic;
//  * operand tiles are DMA'd global -> LDS with global_load_lds_dwordx4 (no staging VGPRs, no
//    ds_write pass).  A DMA's LDS image is lane-linear, so LDS rows are unpadded 128-byte runs
//    (32 floats) and ds_read_b128 bank conflicts are removed by an XOR swizzle applied on the SOURCE
//    side (which 16-byte slot a lane fetches) and again on the read address: lds_rows.h states it;
//  * the DMA is issued from inline asm: for the builtin hipcc (ROCm 7.2) cannot prove that the DMA
//    destination (the other buffer) does not alias the ds_reads of the current buffer and puts
//    `s_waitcnt vmcnt(0)` in front of the first ds_read of every K-step.  The one wait needed
//    (vmcnt(0) before the barrier that ends a K-step) is written by hand;
//  * workgroup id -> (pixel tile, weight panel) with panel = id % panels, panels | 8: id % 8 is the
//    XCD, so an XCD's 4 MB L2 only ever holds its own weight panel(s) (<= 2.4 MB).
//
// conv3x3_slab_kernel  (stride 1: 78 % of the network's FLOPs)
//    256 px x {128|64} cout per 512-thread workgroup (8 waves, 2 per SIMD, one workgroup per CU).
//    Because the zero border is in memory, the 9 taps of a run of consecutive output pixels are 9
//    SHIFTED WINDOWS of one contiguous run of input pixels: per 32-channel chunk that "slab"
//    (tile + (W+3)-pixel halo either side, <= 464 px) is DMA'd ONCE and the taps read it at
//    different offsets -- pixel-side staging traffic drops ~6x vs re-gathering each tap, and
//    the only per-K-step DMA left is the 16 KB weight tile.
// conv3x3_gather_s2_kernel (stride 2: convAB1, trans|rot conv1)
//    128 px x 128 cout per 256-thread workgroup, 2 workgroups per CU; pixel rows are gathered per
//    tap (strided windows have no contiguous slab).
#include "mfma_common.h"

namespace se3tn {

// shared epilogue: lane holds pixel l31 x couts {8q + 4hh + 0..3} of each 32x32 tile.
// MM_F16X3 accumulators carry the per-cout power-of-two weight scale: acc * wscale[c] first.
// rpre != nullptr: the float32 residual values were loaded ahead of time (same [i][j][q] order)
template <int PT, int CT, int EPI, int MM, int OUTF, int RESF>
__device__ __forceinline__ void store_tiles(const ConvArgs& a, int g, const f32x16 (&acc)[PT][CT],
                                            const int (&opix)[PT], const bool (&ok)[PT], int cbase, int hh,
                                            const float4* rpre = nullptr) {
  const float* __restrict__ bias = a.bias + (size_t)g * a.bias_gs;
  const float* __restrict__ wsc = (MM == MM_F16X3) ? a.wscale + (size_t)g * a.bias_gs : nullptr;
  const float* __restrict__ res = (EPI == 1) ? a.res + (size_t)g * a.res_gs : nullptr;
  float* __restrict__ out = a.out + (size_t)g * a.out_gs;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    if (!ok[i]) continue;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cbase + j * 32 + q * 8 + hh * 4;
        float4 v = make_float4(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2],
                               acc[i][j][4 * q + 3]);
        if (MM == MM_F16X3) {
          const float4 w = *reinterpret_cast<const float4*>(wsc + c);
          v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
        }
        const float4 b = *reinterpret_cast<const float4*>(bias + c);
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EPI == 1) {
          if (rpre) r = rpre[(i * CT + j) * 4 + q];
          else
            r = (RESF == FMT_SPLIT) ? load_split4(res, (size_t)opix[i], a.res_ld, c)
                                    : *reinterpret_cast<const float4*>(res + (size_t)opix[i] * a.res_ld + c);
        }
        v = apply_epilogue<EPI>(v, b, r);
        if (OUTF == FMT_SPLIT) bad |= store_split4(out, (size_t)opix[i], a.out_ld, c, v);
        else *reinterpret_cast<float4*>(out + (size_t)opix[i] * a.out_ld + c) = v;
      }
    }
  }
  if (OUTF == FMT_SPLIT && bad) atomicOr(a.overflow, 1);
}

// =================================================================================================
// stride 1: slab kernel.  8 waves = WM x WN; wave tile = PT x CT tiles of 32x32.
// LDS: [slab 0][slab 1][weights 0][weights 1], slab = SLABPX pixel rows of 32 floats.
// =================================================================================================
template <int CIN, int WM, int WN, int PT, int CT, int SLABPX, int EPI, int MM, int OUTF, int RESF>
__global__ __launch_bounds__(512, 2) void conv3x3_slab_kernel(const ConvArgs a) {
  constexpr int BM = WM * PT * 32, BN = WN * CT * 32;
  constexpr int NCH = CIN / 32;
  constexpr int SLAB = SLABPX * 32;  // floats
  constexpr int WT = BN * 32;        // floats per weight tile
  constexpr int WPIECES = BN / 8;    // 1 KB DMA pieces per weight tile (16 or 8)
  static_assert(WM * WN == 8 && (WPIECES == 16 || WPIECES == 8), "8 waves");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int l31 = lane & 31, hh = lane >> 5;

  // PERSISTENT tiles: workgroup b handles tiles b, b + gridDim.x, ...; gridDim.x is a multiple of `panels`
  // (or the whole tile count), so a workgroup keeps its weight panel and the panel <-> XCD affinity.
  // The next tile's first slab and weight tile are DMA'd during the last chunk of the current one, and
  // the epilogue's stores drain under the next tile's first K-steps: no per-tile prologue / epilogue bubble.
  const int panels = a.groups * a.tiles_n;
  const int ntiles = ((a.M + BM - 1) / BM) * panels;
  const int p = blockIdx.x % panels;
  const int g = p / a.tiles_n, nt = p % a.tiles_n;
  const int n0 = nt * BN;
  const float* __restrict__ in = a.in + (size_t)g * a.in_gs;
  const float* __restrict__ wgt = a.w + (size_t)g * a.w_gs + (size_t)n0 * 32;
  const int W = a.W, Wp = W + 2, HW = a.H * W;
  static_assert(NCH % 2 == 0, "chunk 0 of the next tile reuses slab buffer 0 during the last chunk");

  // slab of pixel tile mt = padded-flat pixels [lo, lo + 8 * npieces) covering the tile's pixels +- (Wp + 1)
#define TILE_GEOMETRY(MT, LO, NP)                                                                     \
  {                                                                                                  \
    const int m0_ = (MT) * BM, ml_ = min(m0_ + BM, a.M) - 1;                                          \
    LO = padded_index(m0_, HW, W) - (Wp + 1);                                                         \
    NP = min((padded_index(ml_, HW, W) + (Wp + 1) + 1 - LO + 7) >> 3, SLABPX / 8);                    \
  }
  int tile = blockIdx.x;
  int lo, npieces;
  TILE_GEOMETRY(tile / panels, lo, npieces)

  // ---- DMA geometry ---------------------------------------------------------------------------
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  // slab piece j = 8 pixels: lane l -> pixel 8 j + (l >> 3), LDS slot l & 7 holds channel block
  // lds_rows::slot_block(pixel, l & 7).  Lane form: row_key(8 j + (l >> 3)) = (4 j + (l >> 4)) & 7, two patterns (j even / odd);
  // written out because the compiler folds slot_block((l >> 3) [+ 8], l & 7) into other instructions here
  // (tests/c_abi/lds_rows_check.cpp holds the two spellings together)
  const unsigned sv_even = (unsigned)((lane >> 3) * a.in_ld * 4 + (((lane & 7) ^ ((lane >> 4) & 7)) << 4));
  const unsigned sv_odd = (unsigned)((lane >> 3) * a.in_ld * 4 + (((lane & 7) ^ ((4 + (lane >> 4)) & 7)) << 4));
  // weight piece q = 8 cout rows of the contiguous [BN][32] tile; same swizzle with row = 8 q + (l >> 3)
  const unsigned wv_even = (unsigned)((lane >> 3) * 128 + (((lane & 7) ^ ((lane >> 4) & 7)) << 4));
  const unsigned wv_odd = (unsigned)((lane >> 3) * 128 + (((lane & 7) ^ ((4 + (lane >> 4)) & 7)) << 4));

  // slab piece wid + 8 T of chunk CH into slab buffer SB (this wave owns pieces wid + 8 t, t = 0..8)
#define SLAB_PIECE(LO, NP, CH, SB, T)                                                                \
  {                                                                                                  \
    const int j_ = wid + 8 * (T);                                                                    \
    if (j_ < (NP)) {                                                                                 \
      const float* sb_ = in + (size_t)((LO) + 8 * j_) * a.in_ld + (CH) * 32;                          \
      glds16<0>(sb_, (j_ & 1) ? sv_odd : sv_even, lds0 + (unsigned)(((SB) * SLAB + j_ * 256) * 4));  \
    }                                                                                                \
  }
  // weight tile of K-step (CH, TAP) into weight buffer WB
#define WEIGHT_TILE(CH, TAP, WB)                                                                     \
  {                                                                                                  \
    const float* tb_ = wgt + (size_t)((CH) * 9 + (TAP)) * (a.tiles_n * BN) * 32;                     \
    const unsigned ld_ = lds0 + (unsigned)((2 * SLAB + (WB) * WT) * 4);                              \
    if (WPIECES == 16) {                                                                             \
      glds16<0>(tb_ + wid * 512, wv_even, ld_ + wid * 2048);                                         \
      glds16<1024>(tb_ + wid * 512, wv_odd, ld_ + wid * 2048);                                       \
    } else {                                                                                         \
      glds16<0>(tb_ + wid * 256, (wid & 1) ? wv_odd : wv_even, ld_ + wid * 1024);                    \
    }                                                                                                \
  }

  // weight fragment offsets (floats): lane (l31, hh) reads logical slot 2 kg + hh of row base + l31
  const lds_rows::LaneFrag fo = lds_rows::lane_frag(l31, hh);

  // prologue of the first tile: whole slab of chunk 0 + first weight tile
#pragma unroll
  for (int t = 0; t < 9; ++t) SLAB_PIECE(lo, npieces, 0, 0, t)
  WEIGHT_TILE(0, 0, 0)
  wait_dma_and_barrier();

  for (;;) {
    const int m0 = (tile / panels) * BM;
    const int mlast = min(m0 + BM, a.M) - 1;
    // per-lane pixel rows of this wave's tiles
    int ibase[PT];  // slab index of the pixel at the centre tap
    int opix[PT];   // padded-flat index in the output / residual tensor (same geometry as the input)
    bool ok[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int m = m0 + (wm * PT + i) * 32 + l31;
      ok[i] = m < a.M;
      opix[i] = padded_index(ok[i] ? m : mlast, HW, W);
      ibase[i] = opix[i] - lo;
    }
    const int tnext = tile + (int)gridDim.x;
    const bool more = tnext < ntiles;
    int nlo = 0, nnp = 0;
    if (more) TILE_GEOMETRY(tnext / panels, nlo, nnp)

    f32x16 acc[PT][CT];
    zero_acc(acc);

    // residual + ReLU epilogue of the short-K (64-channel) tiles: the residual values are fetched while the last
    // chunk's MFMAs run instead of after them (an L2 / HBM round trip per tile otherwise sits in the epilogue)
    constexpr bool PREFETCH_RES = (EPI == 1 && RESF == FMT_F32 && PT * CT <= 2);
    float4 rpre[PREFETCH_RES ? PT * CT * 4 : 1];

    int kt = 0;
    for (int ch = 0; ch < NCH; ++ch) {
      const int sb = ch & 1;
      if (PREFETCH_RES && ch == NCH - 1) {
        const float* __restrict__ res_ = a.res + (size_t)g * a.res_gs;
#pragma unroll
        for (int i = 0; i < PT; ++i)
#pragma unroll
          for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              rpre[(i * CT + j) * 4 + q] = *reinterpret_cast<const float4*>(
                  res_ + (size_t)opix[i] * a.res_ld + n0 + wn * CT * 32 + j * 32 + q * 8 + hh * 4);
      }
      for (int tap = 0; tap < 9; ++tap, ++kt) {
        const int wb = kt & 1;
        // next K-step's weights, and this wave's share of the next slab (next chunk, or chunk 0 of the
        // workgroup's next tile)
        if (tap < 8) {
          WEIGHT_TILE(ch, tap + 1, wb ^ 1)
        } else if (ch + 1 < NCH) {
          WEIGHT_TILE(ch + 1, 0, wb ^ 1)
        } else if (more) {
          WEIGHT_TILE(0, 0, wb ^ 1)
        }
        if (ch + 1 < NCH) {
          SLAB_PIECE(lo, npieces, ch + 1, sb ^ 1, tap)
        } else if (more) {
          SLAB_PIECE(nlo, nnp, 0, 0, tap)
        }

        const int r = tap / 3, s = tap - r * 3;
        const int tapoff = (r - 1) * Wp + (s - 1);
        // pixel fragment addresses: slab rows are keyed per pixel: row idx = ibase + tapoff, float offset
        // lds_rows::frag_off(idx, kg, hh) = (8 kg) ^ py with py = slot_off(idx, hh)
        int prow[PT], py[PT];
#pragma unroll
        for (int i = 0; i < PT; ++i) {
          const int idx = ibase[i] + tapoff;
          prow[i] = sb * SLAB + idx * 32;
          py[i] = lds_rows::slot_off(idx, hh);
        }
        const float* pW = smem + 2 * SLAB + wb * WT + (wn * CT * 32 + l31) * 32;
#define SLAB_PXF(G) *reinterpret_cast<const float4*>(smem + prow[i] + ((8 * (G)) ^ py[i]))
        SE3TN_MMA_KSTEP(MM, PT, CT, SLAB_PXF, SE3TN_ROWS_WTF)
#undef SLAB_PXF
        if (kt + 1 < NCH * 9 || more) wait_dma_and_barrier();
      }
    }
    store_tiles<PT, CT, EPI, MM, OUTF, RESF>(a, g, acc, opix, ok, n0 + wn * CT * 32, hh, PREFETCH_RES ? rpre : nullptr);
    if (!more) break;
    tile = tnext;
    lo = nlo;
    npieces = nnp;
  }
#undef SLAB_PIECE
#undef WEIGHT_TILE
#undef TILE_GEOMETRY
}

// =================================================================================================
// stride 2: gather kernel, 4 waves = 2 x 2, wave tile 2 x 2 tiles (128 px x 128 cout), 2 WGs per CU
// =================================================================================================
// NW = 4: 128 px x 128 cout, 2 workgroups per CU (small batches: more, smaller tiles);  NW = 8: 256 px x 128 cout, one
// workgroup per CU: 48 KB instead of 2 x 32 KB of operands DMA'd per K-step for the same flops (the DMA, not the MFMA
// stream, is what these kernels lose time to: scripts/probes/mfma_stream.hip)
template <int CIN, int EPI, int MM, int OUTF, int NW>
__global__ __launch_bounds__(NW * 64, 2) void conv3x3_gather_s2_kernel(const ConvArgs a) {
  constexpr int BM = NW * 32, BN = 128, PT = 2, CT = 2;
  constexpr int RS = NW * 8;          // rows staged per DMA step of the whole workgroup
  constexpr int PJ = BM / RS, WJ = BN / RS;
  constexpr int NCH = CIN / 32, KT = NCH * 9;
  constexpr int BUF = (BM + BN) * 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int l31 = lane & 31, hh = lane >> 5;

  const int panels = a.groups * a.tiles_n;
  const int p = blockIdx.x % panels, mt = blockIdx.x / panels;
  const int g = p / a.tiles_n, nt = p % a.tiles_n;
  const int m0 = mt * BM, n0 = nt * BN;
  const float* __restrict__ in = a.in + (size_t)g * a.in_gs;
  const float* __restrict__ wgt = a.w + (size_t)g * a.w_gs + (size_t)n0 * 32;
  const int Wp = a.W + 2, Hp = a.H + 2, HoWo = a.Ho * a.Wo;
  const int mlast = a.M - 1;

  // staging (lds_rows.h, mfma_common.h): thread t fills LDS slot (t & 7) of rows (t >> 3) + RS j
  const int r0 = tid >> 3;
  const int c4 = lds_rows::slot_block(r0, tid & 7);
  unsigned pvoff[PJ];
  SE3TN_GATHER_PVOFF(2)
  const unsigned wvoff = (unsigned)(lds_rows::stage_src(r0, tid & 7) * 4);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));

  const lds_rows::LaneFrag fo = lds_rows::lane_frag(l31, hh);

  f32x16 acc[PT][CT];
  zero_acc(acc);

  SE3TN_GATHER_ISSUE_TILE(0, 0, 0)
  wait_dma_and_barrier();

  int ch = 0, tap = 0;
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (++tap == 9) { tap = 0; ++ch; }
    if (kt + 1 < KT) SE3TN_GATHER_ISSUE_TILE(ch, tap, buf ^ 1)
    const float* pP = smem + buf * BUF + (wm * PT * 32 + l31) * 32;
    const float* pW = smem + buf * BUF + (BM + wn * CT * 32 + l31) * 32;
    SE3TN_MMA_KSTEP_ROWS(MM, PT, CT)
    if (kt + 1 < KT) wait_dma_and_barrier();
  }

  int opix[PT];
  bool ok[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int m = m0 + (wm * PT + i) * 32 + l31;
    ok[i] = m < a.M;
    opix[i] = padded_index(ok[i] ? m : mlast, HoWo, a.Wo);
  }
  store_tiles<PT, CT, EPI, MM, OUTF, FMT_F32>(a, g, acc, opix, ok, n0 + wn * CT * 32, hh);
}

// one float4 of the output: the slices' partial sums added in a FIXED order, then bias / residual / activation
// PI (mixed-model batch, conv_slices_small only): the bias of output row m's image, img_off[m / (Ho Wo)] floats from a.bias -- a
// per-lane index here (a workgroup may straddle two images), so the offset is selected from the table, not indexed
template <int EPI, int MM, int OUTF, int RESF, bool PI = false>
__device__ __forceinline__ void reduce_element(const ConvArgs& a, const float* src, size_t slice_stride, int g, int m, int c) {
  float4 v = *reinterpret_cast<const float4*>(src);
#pragma unroll 8
  for (int s = 1; s < a.slices; ++s) {  // fixed order: deterministic (unrolled: the loads of 8 slices are in flight together)
    const float4 u = *reinterpret_cast<const float4*>(src + s * slice_stride);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  if (MM == MM_F16X3) {
    const float4 w = *reinterpret_cast<const float4*>(a.wscale + (size_t)g * a.bias_gs + c);
    v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
  }
  const size_t opix = (size_t)padded_index(m, a.Ho * a.Wo, a.Wo);
  const float* bias = a.bias;
  if (PI) {
    const int im = m / (a.Ho * a.Wo);
    long long o = a.img_off[0];
#pragma unroll
    for (int k = 1; k < SMALL_MAX_IMG; ++k) o = im == k ? a.img_off[k] : o;
    bias += o;
  }
  const float4 b = *reinterpret_cast<const float4*>(bias + (size_t)g * a.bias_gs + c);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (EPI == 1) {
    const float* res = a.res + (size_t)g * a.res_gs;
    r = (RESF == FMT_SPLIT) ? load_split4(res, opix, a.res_ld, c) : *reinterpret_cast<const float4*>(res + opix * a.res_ld + c);
  }
  v = apply_epilogue<EPI>(v, b, r);
  float* out = a.out + (size_t)g * a.out_gs;
  if (OUTF == FMT_SPLIT) {
    if (store_split4(out, opix, a.out_ld, c, v)) atomicOr(a.overflow, 1);
  } else {
    *reinterpret_cast<float4*>(out + opix * a.out_ld + c) = v;
  }
}

template <int EPI, int MM, int OUTF, int RESF, bool PI = false>
__global__ __launch_bounds__(256) void conv_reduce_kernel(const ConvArgs a, int cout, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;  // (group, m, c4)
  if (idx >= total) return;
  const int q4 = cout >> 2;
  const int c = (idx % q4) * 4, t = idx / q4;
  const int g = t / a.M, m = t % a.M;
  reduce_element<EPI, MM, OUTF, RESF, PI>(a, a.part + ((size_t)g * a.M + m) * cout + c, (size_t)a.groups * a.M * cout, g, m, c);
}

// =================================================================================================
// small-batch (latency) path: split-K.  At batch 1 the big-tile kernels above would occupy 8-64 of
// the 256 CUs (M = 121..1936 rows), so the K dimension -- cin / 32 chunks x 9 taps K-steps -- is cut into `slices` runs of
// consecutive K-steps (round 4: runs of >= 3 (chunk, tap) steps instead of whole chunks: a K-step of these small grids is DMA-latency
// bound, ~1.3-2.6 us, so the kernel's time is its number of SEQUENTIAL steps; 9 per workgroup before)
// handled by different workgroups (128 px x {128|64} cout, 4 waves, per-tap gather on the
// zero-bordered input, stride 1 or 2, either arithmetic mode).  Each workgroup stores its raw partial accumulators to
// part[slice][group][M][cout]; conv_reduce_kernel sums the slices in a FIXED order (deterministic,
// no atomics) and applies the bias / residual / activation epilogue into the padded output.
// =================================================================================================
template <int CIN, int STRIDE, int CT, int MM>
__global__ __launch_bounds__(256, 2) void conv3x3_splitk_kernel(const ConvArgs a) {
  constexpr int BM = 128, BN = 64 * CT, PT = 2;
  constexpr int NCH = CIN / 32;
  constexpr int RS = 32, PJ = BM / RS, WJ = BN / RS;  // rows staged per DMA step; pixel / weight rows per staging thread
  constexpr int BUF = (BM + BN) * 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int l31 = lane & 31, hh = lane >> 5;

  const int panels = a.groups * a.tiles_n;
  const int sl = blockIdx.x % a.slices, rest = blockIdx.x / a.slices;
  const int p = rest % panels, mt = rest / panels;
  const int g = p / a.tiles_n, nt = p % a.tiles_n;
  const int m0 = mt * BM, n0 = nt * BN;
  const float* __restrict__ in = a.in + (size_t)g * a.in_gs;
  const float* __restrict__ wgt = a.w + (size_t)g * a.w_gs + (size_t)n0 * 32;
  const int Wp = a.W + 2, Hp = a.H + 2, HoWo = a.Ho * a.Wo;
  const int mlast = a.M - 1;
  // K-steps (32-channel chunk, tap) are numbered ch * 9 + tap; slice sl takes KT consecutive ones (a.slices divides NCH * 9)
  const int KT = NCH * 9 / a.slices, ks0 = sl * KT;

  // staging (lds_rows.h, mfma_common.h): thread t fills LDS slot (t & 7) of rows (t >> 3) + 32 j
  const int r0 = tid >> 3;
  const int c4 = lds_rows::slot_block(r0, tid & 7);
  unsigned pvoff[PJ];
  SE3TN_GATHER_PVOFF(STRIDE)
  const unsigned wvoff = (unsigned)(lds_rows::stage_src(r0, tid & 7) * 4);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));

  const lds_rows::LaneFrag fo = lds_rows::lane_frag(l31, hh);

  f32x16 acc[PT][CT];
  zero_acc(acc);

  int ch = ks0 / 9, tap = ks0 - ch * 9;
  SE3TN_GATHER_ISSUE_TILE(ch, tap, 0)
  wait_dma_and_barrier();

  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (++tap == 9) { tap = 0; ++ch; }
    if (kt + 1 < KT) SE3TN_GATHER_ISSUE_TILE(ch, tap, buf ^ 1)
    const float* pP = smem + buf * BUF + (wm * PT * 32 + l31) * 32;
    const float* pW = smem + buf * BUF + (BM + wn * CT * 32 + l31) * 32;
    SE3TN_MMA_KSTEP_ROWS(MM, PT, CT)
    if (kt + 1 < KT) wait_dma_and_barrier();
  }

  // raw partial sums: part[slice][group][m][cout] for conv_reduce_kernel
  const int cout = a.tiles_n * BN;
  float* __restrict__ part = a.part + ((size_t)(sl * a.groups + g) * a.M) * cout;
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int m = m0 + (wm * PT + i) * 32 + l31;
    if (m >= a.M) continue;
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = n0 + (wn * CT + j) * 32 + q * 8 + hh * 4;
        *reinterpret_cast<float4*>(part + (size_t)m * cout + c) =
            make_float4(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
      }
  }
}

template <int CIN, int WM, int WN, int PT, int CT, int SLABPX, int EPI, int MM = MM_F32, int OUTF = FMT_F32,
          int RESF = FMT_F32>
static hipError_t launch_slab(const ConvArgs& a, hipStream_t st) {
  constexpr int BM = WM * PT * 32, BN = WN * CT * 32;
  constexpr size_t lds = (size_t)(2 * SLABPX * 32 + 2 * BN * 32) * sizeof(float);
  static_assert(lds <= 160 * 1024, "LDS budget");
  auto kern = conv3x3_slab_kernel<CIN, WM, WN, PT, CT, SLABPX, EPI, MM, OUTF, RESF>;
  static PerDeviceOnce attr;
  hipError_t e = set_lds(kern, lds, attr);
  if (e != hipSuccess) return e;
  const int tiles_m = (a.M + BM - 1) / BM;
  // one workgroup per CU (LDS-bound); with more tiles than CUs the workgroups are persistent
  const int ntiles = tiles_m * a.tiles_n * a.groups;
  const int grid = ntiles > 256 ? 256 : ntiles;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, a);
  return hipGetLastError();
}

template <int CIN, int EPI, int MM, int OUTF, int NW>
static hipError_t launch_gather_nw(const ConvArgs& a, hipStream_t st) {
  constexpr int BM = NW * 32;
  constexpr size_t lds = (size_t)2 * (BM + 128) * 32 * sizeof(float);
  auto kern = conv3x3_gather_s2_kernel<CIN, EPI, MM, OUTF, NW>;
  static PerDeviceOnce attr;
  hipError_t e = set_lds(kern, lds, attr);
  if (e != hipSuccess) return e;
  const int tiles_m = (a.M + BM - 1) / BM;
  hipLaunchKernelGGL(kern, dim3(tiles_m * a.tiles_n * a.groups), dim3(NW * 64), lds, st, a);
  return hipGetLastError();
}

#ifndef SE3TN_GATHER8_MIN_TILES
#define SE3TN_GATHER8_MIN_TILES 200   // 256-px tiles (8 waves, 1 workgroup per CU) once they fill most of the 256 CUs
#endif
template <int CIN, int EPI, int MM = MM_F32, int OUTF = FMT_F32>
static hipError_t launch_gather(const ConvArgs& a, hipStream_t st) {
  const int tiles256 = ((a.M + 255) / 256) * a.tiles_n * a.groups;
  if (MM == MM_F32 && tiles256 >= SE3TN_GATHER8_MIN_TILES && tiles256 <= 256) return launch_gather_nw<CIN, EPI, MM, OUTF, 8>(a, st);
  return launch_gather_nw<CIN, EPI, MM, OUTF, 4>(a, st);
}

template <int EPI, int MM, int OUTF, int RESF, bool PI = false>
static void launch_reduce(const ConvArgs& a, int cout, hipStream_t st) {
  const int total = a.groups * a.M * (cout / 4);
  hipLaunchKernelGGL((conv_reduce_kernel<EPI, MM, OUTF, RESF, PI>), dim3((total + 255) / 256), dim3(256), 0, st, a, cout, total);
}

// The epilogue pass over the slices' partial sums, chosen once for every caller: epi 0 | 1 | 2, mm = MM_*, outf = FMT_* of the output
// tensor.  f16x3 mode reads split-row residuals and writes split rows, except the last head conv (float32 out); per_img: ConvArgs.
static hipError_t launch_reduce_for(const ConvArgs& a, int cout, int epi, int mm, int outf, bool per_img, hipStream_t st) {
  if (mm == MM_F16X3) {
    if (epi == 0) launch_reduce<0, MM_F16X3, FMT_SPLIT, FMT_F32>(a, cout, st);
    else if (epi == 2) launch_reduce<2, MM_F16X3, FMT_SPLIT, FMT_F32>(a, cout, st);
    else if (outf == FMT_SPLIT) launch_reduce<1, MM_F16X3, FMT_SPLIT, FMT_SPLIT>(a, cout, st);
    else launch_reduce<1, MM_F16X3, FMT_F32, FMT_SPLIT>(a, cout, st);
  } else if (per_img) {
    if (epi == 0) launch_reduce<0, MM_F32, FMT_F32, FMT_F32, true>(a, cout, st);
    else if (epi == 1) launch_reduce<1, MM_F32, FMT_F32, FMT_F32, true>(a, cout, st);
    else launch_reduce<2, MM_F32, FMT_F32, FMT_F32, true>(a, cout, st);
  } else {
    if (epi == 0) launch_reduce<0, MM_F32, FMT_F32, FMT_F32>(a, cout, st);
    else if (epi == 1) launch_reduce<1, MM_F32, FMT_F32, FMT_F32>(a, cout, st);
    else launch_reduce<2, MM_F32, FMT_F32, FMT_F32>(a, cout, st);
  }
  return hipGetLastError();
}

// outf: FMT_* of the output tensor (f16x3 mode: split rows except the last head conv)
template <int CIN, int STRIDE, int CT, int MM>
static hipError_t launch_splitk(const ConvArgs& a, int epi, int outf, hipStream_t st) {
  constexpr int BN = 64 * CT;
  constexpr size_t lds = (size_t)2 * (128 + BN) * 32 * sizeof(float);
  auto kern = conv3x3_splitk_kernel<CIN, STRIDE, CT, MM>;
  static PerDeviceOnce attr;
  hipError_t e = set_lds(kern, lds, attr);
  if (e != hipSuccess) return e;
  const int tiles = ((a.M + 127) / 128) * a.tiles_n * a.groups;
  hipLaunchKernelGGL(kern, dim3(tiles * a.slices), dim3(256), lds, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_reduce_for(a, a.tiles_n * BN, epi, MM, outf, false, st);
}

// Slab sizes (pixels, multiple of 8) = worst case of
//   255 + 2 per row break + (2 Wp + 2) per image break + 2 (Wp + 1) + 1     (tests/test_slab_geometry.py)
//   W = 44: 454 -> 464     W = 22: 378 -> 384     W = 11: 410 -> 424
// Executes the step csrc/infer_plan.h planned for this conv (plan_conv): the template ladders below map (algorithm, shape) to an
// instantiation and decide nothing
hipError_t launch_conv3x3(const ConvArgs& a0, const ConvStep& step, int cin, int cout, int stride, int epi, hipStream_t st) {
  ConvArgs a = a0;
  a.slices = step.slices;
  if (step.algo == ConvStep::SMALL64) return launch_conv64_small(a, a.M / (44 * 44), epi, st);
  if (step.algo == ConvStep::SLICES) {   // float32 only (per_img: the mixed-model call)
    a.tiles_n = cout / 32;
    hipError_t e = launch_conv_slices_small(a, cin, stride, st);
    if (e != hipSuccess || !step.reduce) return e;      // (!reduce: the tail adds the slices: kernels_misc.hip tail_parts_kernel)
    return launch_reduce_for(a, cout, epi, MM_F32, FMT_F32, a.per_img != 0, st);
  }
  if (step.algo == ConvStep::SPLITK) {
    a.tiles_n = cout >= 128 ? cout / 128 : 1;
    if (a.fast) {  // f16x3: split rows everywhere, float32 out of the last head conv (cin 512, residual)
      const int outf = (cin == 512 && epi == 1) ? FMT_F32 : FMT_SPLIT;
      if (cin == 64 && stride == 1) return launch_splitk<64, 1, 1, MM_F16X3>(a, epi, outf, st);
      if (cin == 128 && stride == 2) return launch_splitk<128, 2, 2, MM_F16X3>(a, epi, outf, st);
      if (cin == 256 && stride == 1) return launch_splitk<256, 1, 2, MM_F16X3>(a, epi, outf, st);
      if (cin == 256 && stride == 2) return launch_splitk<256, 2, 2, MM_F16X3>(a, epi, outf, st);
      if (cin == 512 && stride == 1) return launch_splitk<512, 1, 2, MM_F16X3>(a, epi, outf, st);
      return hipErrorInvalidValue;
    }
    if (cin == 64 && stride == 1) return launch_splitk<64, 1, 1, MM_F32>(a, epi, FMT_F32, st);
    if (cin == 128 && stride == 2) return launch_splitk<128, 2, 2, MM_F32>(a, epi, FMT_F32, st);
    if (cin == 256 && stride == 1) return launch_splitk<256, 1, 2, MM_F32>(a, epi, FMT_F32, st);
    if (cin == 256 && stride == 2) return launch_splitk<256, 2, 2, MM_F32>(a, epi, FMT_F32, st);
    if (cin == 512 && stride == 1) return launch_splitk<512, 1, 2, MM_F32>(a, epi, FMT_F32, st);
    return hipErrorInvalidValue;
  }
  if (step.algo != (stride == 1 ? ConvStep::SLAB : ConvStep::GATHER)) return hipErrorInvalidValue;   // (the big-tile kernels)
  if (a.fast) {
    // f16x3 mode (se3tn_set_precision): every 3x3 conv runs on the f16 matrix cores with split-row
    // operands; the max-pool produces the first split-row tensor, the last conv of the heads writes
    // float32 for the tail.
    if (stride == 1 && cin == 64 && cout == 64 && a.W == 44) {
      a.tiles_n = 1;
      if (epi == 0) return launch_slab<64, 8, 1, 1, 2, 464, 0, MM_F16X3, FMT_SPLIT, FMT_F32>(a, st);
      if (epi == 1) return launch_slab<64, 8, 1, 1, 2, 464, 1, MM_F16X3, FMT_SPLIT, FMT_SPLIT>(a, st);
    }
    a.tiles_n = cout / 128;
    if (stride == 2 && cin == 128 && epi == 2) return launch_gather<128, 2, MM_F16X3, FMT_SPLIT>(a, st);
    if (stride == 2 && cin == 256 && epi == 2) return launch_gather<256, 2, MM_F16X3, FMT_SPLIT>(a, st);
    if (stride == 1 && cin == 256 && a.W == 22 && epi == 0)
      return launch_slab<256, 4, 2, 2, 2, 384, 0, MM_F16X3, FMT_SPLIT, FMT_F32>(a, st);
    if (stride == 1 && cin == 256 && a.W == 22 && epi == 1)
      return launch_slab<256, 4, 2, 2, 2, 384, 1, MM_F16X3, FMT_SPLIT, FMT_SPLIT>(a, st);
    if (stride == 1 && cin == 512 && a.W == 11 && epi == 0)
      return launch_slab<512, 4, 2, 2, 2, 424, 0, MM_F16X3, FMT_SPLIT, FMT_F32>(a, st);
    if (stride == 1 && cin == 512 && a.W == 11 && epi == 1)
      return launch_slab<512, 4, 2, 2, 2, 424, 1, MM_F16X3, FMT_F32, FMT_SPLIT>(a, st);
    return hipErrorInvalidValue;
  }
  if (stride == 1 && cin == 64 && cout == 64 && a.W == 44) {
    a.tiles_n = 1;
    if (epi == 0) return launch_slab<64, 8, 1, 1, 2, 464, 0>(a, st);
    if (epi == 1) return launch_slab<64, 8, 1, 1, 2, 464, 1>(a, st);
  }
  a.tiles_n = cout / 128;
  if (stride == 1 && cin == 256 && a.W == 22) {
    if (epi == 0) return launch_slab<256, 4, 2, 2, 2, 384, 0>(a, st);
    if (epi == 1) return launch_slab<256, 4, 2, 2, 2, 384, 1>(a, st);
  }
  if (stride == 1 && cin == 512 && a.W == 11) {
    if (epi == 0) return launch_slab<512, 4, 2, 2, 2, 424, 0>(a, st);
    if (epi == 1) return launch_slab<512, 4, 2, 2, 2, 424, 1>(a, st);
  }
  if (stride == 2 && cin == 128 && epi == 2) return launch_gather<128, 2>(a, st);
  if (stride == 2 && cin == 256 && epi == 2) return launch_gather<256, 2>(a, st);
  return hipErrorInvalidValue;
}

}  // namespace se3tn
