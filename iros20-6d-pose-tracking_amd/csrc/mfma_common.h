// Device-side building blocks shared by the MFMA kernels (conv3x3_mfma.hip, wino_mfma.hip):
// LDS-DMA issue, the f32 / f16x3 MFMA K-step macros on the swizzled row tiles of lds_rows.h, split-row access, epilogue math.
#pragma once
#include "lds_rows.h"
#include "se3tn_internal.h"

namespace se3tn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

// Arithmetic modes of the MFMA core (template parameter MM)
//   MM_F32   v_mfma_f32_32x32x2_f32 on float32 operands: bitwise an fmaf chain (default).
//   MM_F16X3 operands stored as "split rows": per (pixel | cout, 32-channel chunk) 128 bytes =
//            32 x f16 hi | 32 x f16 lo with x = hi + lo to 22 significant bits; the product is formed
//            as hi*hi + hi*lo + lo*hi with three v_mfma_f32_32x32x16_f16 (f32 accumulate): 16/3 = 5.3x
//            the f32 MFMA rate at f32-class error (the dropped lo*lo term is 2^-22 relative).
//            A split row has the SAME size, 16-byte slot structure and swizzle as a float32 row (lds_rows.h):
//            slot 2 kb + hh (+4) is exactly the 8-half MFMA operand of lane-half hh for 16-channel block kb.
enum { MM_F32 = 0, MM_F16X3 = 1 };
// tensor element formats of the epilogue (template parameters OUTF / RESF)
enum { FMT_F32 = 0, FMT_SPLIT = 1 };

constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f;

__device__ __forceinline__ float selu_f(float v) {
  return v > 0.f ? SELU_SCALE * v : (SELU_SCALE * SELU_ALPHA) * expm1f(v);
}

// EPI: 0 = bias+ReLU, 1 = bias+residual+ReLU, 2 = bias+SELU
template <int EPI>
__device__ __forceinline__ float4 apply_epilogue(float4 v, const float4 b, const float4 r) {
  v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  if (EPI == 1) { v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
  if (EPI == 2) {
    v.x = selu_f(v.x); v.y = selu_f(v.y); v.z = selu_f(v.z); v.w = selu_f(v.w);
  } else {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
  }
  return v;
}

// ---- LDS-DMA helpers ---------------------------------------------------------------------------
// global_load_lds_dwordx4 voff, s[base:base+1] offset:IMM
//   lane l:  LDS[M0 + IMM + 16 l] <- 16 bytes at (base + voff_l + IMM)     (IMM moves BOTH sides,
//   verified on hardware: scripts/probes/probe_glds.hip)
__device__ __forceinline__ unsigned lds_addr_of(const float* p) {
  return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) float*)p;
}
template <int IMM>
__device__ __forceinline__ void glds16(const float* sbase, unsigned voff_bytes, unsigned lds_byte_addr) {
  // both scalar operands are wave-uniform by construction; readfirstlane makes that provable to
  // the compiler (an "s" constraint on a value it believes divergent does not assemble)
  const unsigned long long b_ = (unsigned long long)sbase;
  const unsigned blo_ = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)b_);  // (the builtin returns int)
  const unsigned bhi_ = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b_ >> 32));
  const unsigned long long sb_ = ((unsigned long long)bhi_ << 32) | (unsigned long long)blo_;
  const unsigned lds_ = __builtin_amdgcn_readfirstlane(lds_byte_addr);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3 offset:%4\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff_bytes), "s"(lds_), "s"(sb_), "i"(IMM)
      : "memory");
}
__device__ __forceinline__ void wait_dma_and_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// One 8-k group of a K-step: PTN x CTN x 4 MFMAs.  PVEXPR may use `i`, WVEXPR may use `j`.
#define SE3TN_MMA_GROUP(PTN, CTN, PVEXPR, WVEXPR)                                                     \
  {                                                                                                  \
    float4 pv_[PTN], wv_[CTN];                                                                       \
    _Pragma("unroll") for (int i = 0; i < PTN; ++i) pv_[i] = PVEXPR;                                 \
    _Pragma("unroll") for (int j = 0; j < CTN; ++j) wv_[j] = WVEXPR;                                 \
    _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[j].x, pv_[i].x, acc[i][j], 0, 0, 0);    \
    _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[j].y, pv_[i].y, acc[i][j], 0, 0, 0);    \
    _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[j].z, pv_[i].z, acc[i][j], 0, 0, 0);    \
    _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i)  \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv_[j].w, pv_[i].w, acc[i][j], 0, 0, 0);    \
  }

// MM_F16X3: all four groups' fragments, then per 16-channel block kb: Whi*Phi + Whi*Plo + Wlo*Phi.
// PVEXPR(G) / WVEXPR(G): float4 fragment of group G (may use `i` / `j`).
#define SE3TN_MMA_SPLIT(PTN, CTN, PVEXPR, WVEXPR)                                                    \
  {                                                                                                  \
    half8 ph_[4][PTN], wh_[4][CTN];                                                                  \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                               \
      _Pragma("unroll") for (int i = 0; i < PTN; ++i) {                                              \
        const float4 t_ = PVEXPR(gq);                                                                \
        ph_[gq][i] = __builtin_bit_cast(half8, t_);                                                  \
      }                                                                                              \
      _Pragma("unroll") for (int j = 0; j < CTN; ++j) {                                              \
        const float4 t_ = WVEXPR(gq);                                                                \
        wh_[gq][j] = __builtin_bit_cast(half8, t_);                                                  \
      }                                                                                              \
    }                                                                                                \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                               \
      _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i) \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[kb][j], ph_[kb][i], acc[i][j], 0, 0, 0);     \
      _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i) \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[kb][j], ph_[kb + 2][i], acc[i][j], 0, 0, 0); \
      _Pragma("unroll") for (int j = 0; j < CTN; ++j) _Pragma("unroll") for (int i = 0; i < PTN; ++i) \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh_[kb + 2][j], ph_[kb][i], acc[i][j], 0, 0, 0); \
    }                                                                                                \
  }

// ---- the K-step on row tiles (lds_rows.h) ---------------------------------------------------------
// One K-step (32 channels) in either arithmetic mode: PXF(G) / WTF(G) name the float4 fragment of 8-k group G (may use `i` / `j`).
#define SE3TN_MMA_KSTEP(MM, PTN, CTN, PXF, WTF)                                                       \
  if ((MM) == MM_F16X3) {                                                                            \
    SE3TN_MMA_SPLIT(PTN, CTN, PXF, WTF)                                                              \
  } else {                                                                                           \
    SE3TN_MMA_GROUP(PTN, CTN, PXF(0), WTF(0))                                                        \
    SE3TN_MMA_GROUP(PTN, CTN, PXF(1), WTF(1))                                                        \
    SE3TN_MMA_GROUP(PTN, CTN, PXF(2), WTF(2))                                                        \
    SE3TN_MMA_GROUP(PTN, CTN, PXF(3), WTF(3))                                                        \
  }
// The fragments of a wave's row tiles: `pP` / `pW` point at this lane's row (l31) of the wave's first 32-row pixel / weight block
// (a multiple of 32 rows into the tile), blocks i / j follow 1024 floats apart, `fo` = lds_rows::lane_frag(l31, hh).
#define SE3TN_ROWS_PXF(G) *reinterpret_cast<const float4*>(pP + i * 1024 + SE3TN_FRAG_OFF(fo, G))
#define SE3TN_ROWS_WTF(G) *reinterpret_cast<const float4*>(pW + j * 1024 + SE3TN_FRAG_OFF(fo, G))
// the whole K-step on pP / pW row tiles into acc[PTN][CTN]
#define SE3TN_MMA_KSTEP_ROWS(MM, PTN, CTN) SE3TN_MMA_KSTEP(MM, PTN, CTN, SE3TN_ROWS_PXF, SE3TN_ROWS_WTF)

template <int PT, int CT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[PT][CT]) {
#pragma unroll
  for (int i = 0; i < PT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// ---- per-tap gather of the 3x3 convs' row tiles (conv3x3_gather_s2_kernel, conv3x3_splitk_kernel) ----------------------
// A workgroup stages RS rows per DMA step: thread t fills LDS slot (t & 7) of rows r0 + RS j, r0 = t >> 3, with channel block
// c4 = lds_rows::slot_block(r0, t & 7) (RS % 16 == 0: one key for all of a thread's rows).  pvoff[j] = byte offset of that block
// of pixel row m0 + r0 + RS j (clamped to the last row) under tap (0, 0): in padded coordinates tap (r, s) of output (ho, wo)
// is input (STRIDE ho + r, STRIDE wo + s), so a tap is one scalar offset on the DMA base.
// (A macro, like the K-step: as a function the compiler forms other address arithmetic.)  Names of the calling kernel: a, m0, r0,
// c4, pvoff[PJ], Wp = a.W + 2, Hp = a.H + 2, HoWo = a.Ho * a.Wo, mlast = a.M - 1 and the constants RS, PJ.
#define SE3TN_GATHER_PVOFF(STRIDE)                                                                   \
  _Pragma("unroll") for (int j = 0; j < PJ; ++j) {                                                   \
    const int m = min(m0 + r0 + RS * j, mlast);                                                      \
    const int n = m / HoWo, rem = m - n * HoWo;                                                      \
    const int ho = rem / a.Wo, wo = rem - ho * a.Wo;                                                 \
    pvoff[j] = (unsigned)((((n * Hp + (STRIDE) * ho) * Wp + (STRIDE) * wo) * a.in_ld + c4 * 4) * 4); \
  }
// K-step (CH, TAP) into buffer BUFI = [BM pixel rows][BN weight rows]: PJ = 4 pixel pieces and WJ weight pieces of RS rows per
// thread.  Names of the calling kernel: in, wgt, Wp, a, lds0, wid, pvoff[PJ], wvoff and the constants BM, BN, BUF, RS, PJ, WJ.
#define SE3TN_GATHER_ISSUE_TILE(CH, TAP, BUFI)                                                       \
  {                                                                                                  \
    static_assert(PJ == 4 && PJ * RS == BM, "four pixel pieces per thread");                         \
    const int r_ = (TAP) / 3, s_ = (TAP) - r_ * 3;                                                   \
    const float* pb_ = in + (size_t)(r_ * Wp + s_) * a.in_ld + (CH) * 32;                            \
    const unsigned lb_ = lds0 + (unsigned)(((BUFI) * BUF + wid * 256) * 4);                          \
    glds16<0>(pb_, pvoff[0], lb_);                                                                   \
    glds16<0>(pb_, pvoff[1], lb_ + RS * 128);                                                        \
    glds16<0>(pb_, pvoff[2], lb_ + 2 * RS * 128);                                                    \
    glds16<0>(pb_, pvoff[3], lb_ + 3 * RS * 128);                                                    \
    const float* tb_ = wgt + (size_t)((CH) * 9 + (TAP)) * (a.tiles_n * BN) * 32;                     \
    _Pragma("unroll") for (int j_ = 0; j_ < WJ; ++j_)                                                \
        glds16<0>(tb_ + j_ * RS * 32, wvoff, lb_ + BM * 128 + j_ * RS * 128);                        \
  }

// ---- split-row element access: 4 consecutive channels c..c+3 (c % 4 == 0) of pixel `pix` ---------
__device__ __forceinline__ size_t split_byte_off(size_t pix, int ld, int c) {
  return (pix * ld) * 4 + (size_t)(c >> 5) * 128 + (c & 31) * 2;
}
__device__ __forceinline__ float4 load_split4(const float* base, size_t pix, int ld, int c) {
  const unsigned char* p_ = reinterpret_cast<const unsigned char*>(base) + split_byte_off(pix, ld, c);
  const half4 h = *reinterpret_cast<const half4*>(p_);
  const half4 l = *reinterpret_cast<const half4*>(p_ + 64);
  return make_float4((float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2],
                     (float)h[3] + (float)l[3]);
}
// returns true if a value is outside the f16 range (the caller raises the overflow flag)
__device__ __forceinline__ bool store_split4(float* base, size_t pix, int ld, int c, float4 v) {
  unsigned char* p_ = reinterpret_cast<unsigned char*>(base) + split_byte_off(pix, ld, c);
  half4 h, l;
  const float f[4] = {v.x, v.y, v.z, v.w};
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)f[e];
    l[e] = (_Float16)(f[e] - (float)h[e]);
    bad |= !(fabsf(f[e]) <= 65000.f);
  }
  *reinterpret_cast<half4*>(p_) = h;
  *reinterpret_cast<half4*>(p_ + 64) = l;
  return bad;
}

// padded-flat pixel index of interior pixel m (flattened over the batch) of an [n,H+2,W+2,*] tensor
__device__ __forceinline__ int padded_index(int m, int HW, int W) {
  const int n = m / HW, rem = m - n * HW;
  const int h = rem / W, w = rem - h * W;
  return (n * (HW / W + 2) + h + 1) * (W + 2) + w + 1;
}


}  // namespace se3tn
