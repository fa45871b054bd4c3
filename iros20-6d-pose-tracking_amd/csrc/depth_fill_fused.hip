// se3tn_fill_depth restricted to a rectangle of the frame (se3tn_fill_depth_rect, the live-camera call se3tn_on_track_live): the
// arithmetic of depth_fill.hip, bit for bit, in at most four stream operations instead of 10-13.
//   1. fd_fused_chain_kernel: prepare -> dilate (diamond) -> dilate 5x5 -> erode 5x5 -> holes := dilate 7x7 -> median 5x5 of the WHOLE
//      frame in one launch.  A workgroup stages its output tile with an 11-pixel halo (2 + 2 + 2 + 3 + 2) once and runs the steps from
//      LDS between two ping-pong buffers; the region that is valid shrinks step by step and only the median image goes to memory.  Every
//      step is a selection (max / min / exact median of 25), so the values are those of the one-launch-per-step chain whatever the tiling.
//      Positions outside the FRAME are never computed and never read: every step tests the frame coordinates of its taps as
//      fd_morph_kernel does (OpenCV's morphology ignores them: -inf to a dilate, +inf to an erode, at every step, not only for the
//      input), and the median clamps its coordinates to the frame (BORDER_REPLICATE of the filled image).
//      Its epilogue reduces the tile's min / max and publishes them with integer atomics on the order-preserving keys (the bilateral
//      table needs the range of the whole image: that is why this launch covers the frame, not the rectangle).
//   2. fd_rect_lut_kernel: the 4098-entry table of the bilateral filter (bilateral only).
//   3. fd_rect_kernel: bilateral / gaussian / no blur, invert back and the uint16 conversion for the pixels of the rectangle only, each
//      with the operations, their order and fp contract(off) of fd_bilateral5_kernel / fd_gauss5_kernel + fd_select_valid_kernel /
//      fd_finish_kernel.  fd_rects_kernel (se3tn_fill_depth_rects, se3tn_on_track_objects_live): the same pass for a table of up to 64
//      rectangles per launch, behind steps 1 and 2 run ONCE for the frame.
// The two min / max words are kept so that ONE memset resets both: word 0 = min of the keys, word 1 = min of the COMPLEMENTED keys.
#include <algorithm>
#include <cmath>

#include "se3tn_internal.h"
#include "depth_fill_common.h"

namespace se3tn {

constexpr int FT_W = 32, FT_H = 16;        // output tile: 600 workgroups at 480 x 640, 16.4 KB of LDS each
constexpr int FT_HALO = 11;
constexpr int FP_W = FT_W + 2 * FT_HALO;   // staged patch 54 x 38
constexpr int FP_H = FT_H + 2 * FT_HALO;

// one morphology step on the patch positions at least MARGIN inside it; (fy0, fx0) = frame coordinates of patch position (0, 0).
// Template arguments as fd_morph_kernel, taps in its order.
template <int OP, int SHAPE, int R, int FILL, int MARGIN>
__device__ __forceinline__ void tile_morph(const float* __restrict__ in, float* __restrict__ out, int fy0, int fx0, int H, int W) {
  constexpr int RW = FP_W - 2 * MARGIN, RH = FP_H - 2 * MARGIN;
  for (int i = threadIdx.x; i < RW * RH; i += 256) {
    const int ly = MARGIN + i / RW, lx = MARGIN + i % RW;
    const int y = fy0 + ly, x = fx0 + lx;
    if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) continue;
    const float centre = in[ly * FP_W + lx];
    if (FILL && !(centre < 0.1f)) { out[ly * FP_W + lx] = centre; continue; }
    float v = OP == 0 ? -INFINITY : INFINITY;
    for (int dy = -R; dy <= R; ++dy) {
      if ((unsigned)(y + dy) >= (unsigned)H) continue;
      const int span = SHAPE == 1 ? R - (dy < 0 ? -dy : dy) : R;
      for (int dx = -span; dx <= span; ++dx) {
        if ((unsigned)(x + dx) >= (unsigned)W) continue;
        const float t = in[(ly + dy) * FP_W + lx + dx];
        v = OP == 0 ? fmaxf(v, t) : fminf(v, t);
      }
    }
    out[ly * FP_W + lx] = v;
  }
}

__global__ __launch_bounds__(256) void fd_fused_chain_kernel(const uint16_t* __restrict__ mm, float* __restrict__ median, int H, int W,
                                                              float max_depth, unsigned* __restrict__ minmax) {
  __shared__ float bufA[FP_H * FP_W], bufB[FP_H * FP_W];
  __shared__ unsigned red[8];
  const int fy0 = blockIdx.y * FT_H - FT_HALO, fx0 = blockIdx.x * FT_W - FT_HALO;
  // prepare (fd_prepare_kernel) for the patch positions inside the frame
  for (int i = threadIdx.x; i < FP_H * FP_W; i += 256) {
    const int ly = i / FP_W, lx = i % FP_W;
    const int y = fy0 + ly, x = fx0 + lx;
    if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) continue;
    float d = (float)((double)mm[(size_t)y * W + x] / 1e3);
    if (d > 0.1f) d = max_depth - d;
    bufA[i] = d;
  }
  __syncthreads();
  tile_morph<0, 1, 2, 0, 2>(bufA, bufB, fy0, fx0, H, W);   // dilate, diamond
  __syncthreads();
  tile_morph<0, 0, 2, 0, 4>(bufB, bufA, fy0, fx0, H, W);   // close = dilate 5x5
  __syncthreads();
  tile_morph<1, 0, 2, 0, 6>(bufA, bufB, fy0, fx0, H, W);   //         then erode 5x5
  __syncthreads();
  tile_morph<0, 0, 3, 1, 9>(bufB, bufA, fy0, fx0, H, W);   // holes := dilate 7x7
  __syncthreads();
  // median of 25 with the coordinates clamped to the frame (fd_median5_kernel); a clamped tap is within 2 of its pixel: margin >= 9
  unsigned lo = 0xffffffffu, hi = 0u;
  for (int i = threadIdx.x; i < FT_H * FT_W; i += 256) {
    const int y = fy0 + FT_HALO + i / FT_W, x = fx0 + FT_HALO + i % FT_W;
    if (y >= H || x >= W) continue;
    float v[25];
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
      const int ly = min(max(y + dy, 0), H - 1) - fy0;
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int lx = min(max(x + dx, 0), W - 1) - fx0;
        v[(dy + 2) * 5 + dx + 2] = bufA[ly * FP_W + lx];
      }
    }
#pragma unroll
    for (int a = 0; a < 13; ++a) {
#pragma unroll
      for (int b = a + 1; b < 25; ++b) {
        const float l = fminf(v[a], v[b]), h = fmaxf(v[a], v[b]);
        v[a] = l; v[b] = h;
      }
    }
    median[(size_t)y * W + x] = v[12];
    const unsigned k = f32_key(v[12]);
    lo = min(lo, k); hi = max(hi, k);
  }
  if (!minmax) return;   // (uniform)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lo; red[4 + (threadIdx.x >> 6)] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {   // integer atomics: the result does not depend on the order the workgroups arrive in
    lo = min(min(red[0], red[1]), min(red[2], red[3]));
    hi = max(max(red[4], red[5]), max(red[6], red[7]));
    atomicMin(&minmax[0], lo);
    atomicMin(&minmax[1], ~hi);
  }
}

// min / max of an image the one-launch-per-step chain left (extrapolate != 0), into the words as kept here
__global__ __launch_bounds__(256) void fd_rect_minmax_kernel(const float* __restrict__ in, int total, unsigned* __restrict__ mm) {
  unsigned lo = 0xffffffffu, hi = 0u;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned k = f32_key(in[i]);
    lo = min(lo, k); hi = max(hi, k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { atomicMin(&mm[0], lo); atomicMin(&mm[1], ~hi); }
}

// the two blurs keep multiply and add separate (as the scalar OpenCV loops and the numpy oracle do)
#pragma clang fp contract(off)

// fd_bilateral_lut_kernel reading the words as kept here
__global__ __launch_bounds__(256) void fd_rect_lut_kernel(const unsigned* __restrict__ mm, float* __restrict__ lut, double gauss_color_coeff) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= BIL_BINS + 2) return;
  const float len = (float)((double)key_f32(~mm[1]) - (double)key_f32(mm[0]));
  const float scale_index = (float)BIL_BINS / len;
  const double val = (double)i / (double)scale_index;
  lut[i] = (float)exp(val * val * gauss_color_coeff);
}

// BLUR as SE3TN_BLUR_*: 0 none, 1 bilateral, 2 gaussian on the valid pixels.  The last pass for frame pixel (y, x): blur, invert back and
// the uint16 conversion -- the one body of fd_rect_kernel and fd_rects_kernel
template <int BLUR>
__device__ __forceinline__ uint16_t fd_rect_pixel(const float* __restrict__ in, int H, int W, int y, int x, const unsigned* __restrict__ mm,
                                                  const float* __restrict__ lut, const BilateralTaps& taps, float max_depth) {
  const float val0 = in[(size_t)y * W + x];
  float d = val0;
  if (BLUR == 1) {   // fd_bilateral5_kernel
    const float vmin = key_f32(mm[0]), vmax = key_f32(~mm[1]);
    if (!(fabs((double)vmin - (double)vmax) < 1.1920928955078125e-07)) {
      const float scale_index = (float)BIL_BINS / (float)((double)vmax - (double)vmin);
      float wsum = 1.f, sum = val0;
      int k = 0;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          if ((dy == 0 && dx == 0) || dy * dy + dx * dx > 4) continue;
          const float sw = taps.w[k++];
          const float val = in[(size_t)reflect101(y + dy, H) * W + reflect101(x + dx, W)];
          float alpha = fabsf(val - val0) * scale_index;
          const int idx = (int)floorf(alpha);
          alpha -= (float)idx;
          const float w = sw * (lut[idx] + alpha * (lut[idx + 1] - lut[idx]));
          sum += val * w;
          wsum += w;
        }
      d = sum / wsum;
    }
  } else if (BLUR == 2) {   // fd_gauss5_kernel<0>, <1> and fd_select_valid_kernel: the five row sums this pixel's column sum reads
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float s = 0.f;
#pragma unroll
    for (int t = -2; t <= 2; ++t) {
      const float* row = in + (size_t)reflect101(y + t, H) * W;
      float rs = 0.f;
#pragma unroll
      for (int u = -2; u <= 2; ++u) rs += row[reflect101(x + u, W)] * k[u + 2];
      s += rs * k[t + 2];
    }
    d = val0 > 0.1f ? s : val0;
  }
  // fd_finish_kernel
  if (d > 0.1f) d = max_depth - d;
  const float mmv = d * 1000.f;
  const int iv = (mmv >= -2147483648.f && mmv < 2147483648.f) ? (int)mmv : (int)0x80000000u;
  return (uint16_t)(unsigned)iv;
}

// One thread per pixel of [cy0, cy0 + ch) x [cx0, cx0 + cw)
template <int BLUR>
__global__ __launch_bounds__(256) void fd_rect_kernel(const float* __restrict__ in, int H, int W, int cx0, int cy0, int cw, int ch,
                                                       const unsigned* __restrict__ mm, const float* __restrict__ lut,
                                                       const BilateralTaps taps, float max_depth, uint16_t* __restrict__ out_full,
                                                       uint16_t* __restrict__ out_sub, int sx0, int sy0, int sx1, int sy1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cw * ch) return;
  const int y = cy0 + i / cw, x = cx0 + i % cw;
  const uint16_t o = fd_rect_pixel<BLUR>(in, H, W, y, x, mm, lut, taps, max_depth);
  if (out_full) out_full[(size_t)y * W + x] = o;
  if (out_sub && x >= sx0 && x < sx1 && y >= sy0 && y < sy1) out_sub[(size_t)(y - sy0) * (sx1 - sx0) + (x - sx0)] = o;
}

// The same for a table of rectangles of ONE frame: grid.y = rectangle, grid.x sized by the largest of the launch (threads past their
// rectangle's area exit).  Rectangle r goes tightly packed to out_base + off[r]; rectangle `full` (if any) to out_full instead.
// Rectangles may overlap or repeat: every pixel value depends on the frame only, and every rectangle has its own output.
template <int BLUR>
__global__ __launch_bounds__(256) void fd_rects_kernel(const float* __restrict__ in, int H, int W, const FillRectTable tab,
                                                        const unsigned* __restrict__ mm, const float* __restrict__ lut,
                                                        const BilateralTaps taps, float max_depth, uint16_t* __restrict__ out_base,
                                                        uint16_t* __restrict__ out_full) {
  const int r = blockIdx.y;   // (uniform: the table is read with scalar loads)
  const int cw = tab.w[r], ch = tab.h[r];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cw * ch) return;
  const int ly = i / cw, lx = i % cw;
  const uint16_t o = fd_rect_pixel<BLUR>(in, H, W, tab.y0[r] + ly, tab.x0[r] + lx, mm, lut, taps, max_depth);
  uint16_t* out = r == tab.full ? out_full : out_base + tab.off[r];
  out[(size_t)ly * cw + lx] = o;
}

// The part in front of the last pass, ONCE per frame: the chain up to the median of the whole frame, the range of that image and the
// table of the bilateral filter
static hipError_t fill_chain_to_median(const FillDepthArgs& f, hipStream_t st, float** median, BilateralTaps& taps) {
  const int total = f.H * f.W;
  if (f.blur == 1)   // min word := 0xffffffff, complemented max word := 0xffffffff
    if (const hipError_t e = hipMemsetAsync(f.minmax, 0xff, 2 * sizeof(unsigned), st)) return e;
  float* med = f.buf0;
  if (!f.extrapolate) {
    hipLaunchKernelGGL(fd_fused_chain_kernel, dim3((f.W + FT_W - 1) / FT_W, (f.H + FT_H - 1) / FT_H), dim3(256), 0, st, f.depth_mm, med,
                       f.H, f.W, (float)f.max_depth, f.blur == 1 ? f.minmax : nullptr);
  } else {   // a per-column pass over the whole frame and a 31 x 31 dilate: the one-launch-per-step chain
    float* spare;
    launch_fill_depth_to_median(f, st, &med, &spare);
    if (f.blur == 1) hipLaunchKernelGGL(fd_rect_minmax_kernel, dim3(64), dim3(256), 0, st, med, total, f.minmax);
  }
  if (f.blur == 1) {
    hipLaunchKernelGGL(fd_rect_lut_kernel, dim3((BIL_BINS + 2 + 255) / 256), dim3(256), 0, st, f.minmax, f.lut,
                       -0.5 / (f.sigma_color * f.sigma_color));
    bilateral_space_taps(f.sigma_space, taps.w);
  }
  *median = med;
  return hipSuccess;
}

hipError_t launch_fill_depth_rect(const FillDepthRectArgs& a, hipStream_t st) {
  const FillDepthArgs& f = a.f;
  float* med;
  BilateralTaps taps{};
  if (const hipError_t e = fill_chain_to_median(f, st, &med, taps)) return e;
  const int cw = a.cx1 - a.cx0, ch = a.cy1 - a.cy0;
  const dim3 grid((unsigned)(((size_t)cw * ch + 255) / 256));
  auto k = f.blur == 1 ? fd_rect_kernel<1> : f.blur == 2 ? fd_rect_kernel<2> : fd_rect_kernel<0>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, (const float*)med, f.H, f.W, a.cx0, a.cy0, cw, ch, (const unsigned*)f.minmax,
                     (const float*)f.lut, taps, (float)f.max_depth, a.out_full, a.out_sub, a.sx0, a.sy0, a.sx1, a.sy1);
  return hipGetLastError();
}

hipError_t launch_fill_depth_rects(const FillDepthRectsArgs& a, hipStream_t st) {
  const FillDepthArgs& f = a.f;
  int live = a.out_full ? 1 : 0;
  for (int i = 0; i < a.n; ++i) live += a.rects[4 * i + 2] > a.rects[4 * i] && a.rects[4 * i + 3] > a.rects[4 * i + 1];
  if (!live) return hipSuccess;   // every rectangle empty: nothing is enqueued
  float* med;
  BilateralTaps taps{};
  if (const hipError_t e = fill_chain_to_median(f, st, &med, taps)) return e;
  auto k = f.blur == 1 ? fd_rects_kernel<1> : f.blur == 2 ? fd_rects_kernel<2> : fd_rects_kernel<0>;
  FillRectTable tab;
  auto flush = [&] {
    size_t mx = 0;
    for (int j = 0; j < tab.n; ++j) mx = std::max(mx, (size_t)tab.w[j] * tab.h[j]);
    hipLaunchKernelGGL(k, dim3((unsigned)((mx + 255) / 256), tab.n), dim3(256), 0, st, (const float*)med, f.H, f.W, tab,
                       (const unsigned*)f.minmax, (const float*)f.lut, taps, (float)f.max_depth, a.out_base, a.out_full);
    tab = FillRectTable{};
  };
  tab = FillRectTable{};
  for (int i = 0; i < a.n; ++i) {
    const int32_t* r = a.rects + 4 * (size_t)i;
    if (r[2] <= r[0] || r[3] <= r[1]) continue;
    const int j = tab.n++;
    tab.x0[j] = r[0]; tab.y0[j] = r[1]; tab.w[j] = r[2] - r[0]; tab.h[j] = r[3] - r[1]; tab.off[j] = (long long)a.offs[i];
    if (tab.n == FillRectTable::MAX) flush();
  }
  if (a.out_full) {   // the whole frame as one more rectangle
    const int j = tab.n++;
    tab.x0[j] = 0; tab.y0[j] = 0; tab.w[j] = f.W; tab.h[j] = f.H; tab.off[j] = 0; tab.full = j;
  }
  if (tab.n) flush();
  return hipGetLastError();
}

}  // namespace se3tn
