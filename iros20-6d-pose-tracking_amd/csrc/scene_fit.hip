// The scene record (se3tn_scene_stats, the last stage of se3tn_scene_fit): n depth layers of one frame composed through a shared depth
// test, per layer the fit record over the pixels where it is the nearest layer, the id image and the composed depth.  The rule is
// scene_fit_rule.h, compiled into this kernel statement by statement; the grid and the sizes are scene_fit_plan.h.  Integers only.
//
// One thread per frame pixel of a 32 x 8 tile, a 1-D grid of plan.tiles_x * plan.tiles_y tiles over the plan's area.  A thread finds
// its pixel's owner in one loop over the n layers (rectangle test, two-byte load), stores ids / scene, then walks the layers again:
// per layer the six counts are ballots + popcounts of the wave, sum |o - m| a wave64 shuffle sum and hidden_by a shuffle OR (both
// skipped when the ballot says no lane has anything to add) -> LDS across the four waves -> the protocol of record_reduce.h in its
// second shape: thread (layer, word) adds its word (OR for hidden_by; zeros are skipped), so every wave waits for its atomics and
// thread 0 takes the ticket behind a barrier; the last workgroup stores the finished records.
#include "record_reduce.h"
#include "se3tn_internal.h"

namespace se3tn {

__global__ __launch_bounds__(SCENE_THREADS) void scene_fit_kernel(const SceneArgs a) {
  __shared__ unsigned part[4][SCENE_MAX_LAYERS][SCENE_WORDS];
  __shared__ int last;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  int bx_tile, by_tile, x, y;
  scene_tile_of(a.plan, blockIdx.x, bx_tile, by_tile);
  scene_thread_pixel(a.plan, bx_tile, by_tile, t, x, y);
  const bool in = x < a.plan.x1 && y < a.plan.y1;   // (the area lies inside the frame: the rectangles do)
  int o = 0, owner = -1, best = 0;
  if (in) {
    const size_t q = (size_t)y * (size_t)a.W + (size_t)x;
    o = a.observed[q];
    for (int i = 0; i < a.n; ++i) scene_offer(i, scene_layer_at(a.l[i], x, y), owner, best);
    if (a.ids) a.ids[q] = (uint8_t)(owner + 1);
    if (a.scene) a.scene[q] = (uint16_t)best;
  }
  for (int i = 0; i < a.n; ++i) {   // (uniform: the layers travel as kernel arguments)
    unsigned ad = 0u, by = 0u, bits = 0u;
    if (in) bits = scene_classify(i, scene_layer_at(a.l[i], x, y), owner, o, a.tol, ad, by);
    unsigned w[SCENE_WORDS];
#pragma unroll
    for (int k = 0; k < SC_COUNTS; ++k) w[k] = (unsigned)__popcll(__ballot((bits >> k) & 1u));
    w[SCENE_SUM] = 0u;
    w[SCENE_BY] = 0u;
    if (w[SC_INLIER] != 0u) w[SCENE_SUM] = wave_sum(ad);   // (uniform over the wave)
    if (w[SC_MODEL] != w[SC_VISIBLE]) {   // some lane's pixel of this layer is hidden
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) by |= __shfl_xor(by, s, 64);
      w[SCENE_BY] = by;
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < SCENE_WORDS; ++k) part[wave][i][k] = w[k];
    }
  }
  __syncthreads();
  {   // thread (layer, word): the four waves' words -> ONE vector atomic into the context's counters
    const int li = t / SCENE_WORDS, k = t - li * SCENE_WORDS;
    if (li < a.n) {
      unsigned* cnt = a.counters + (size_t)li * SCENE_WORDS + k;
      if (k == SCENE_BY) {
        const unsigned s = part[0][li][k] | part[1][li][k] | part[2][li][k] | part[3][li][k];
        if (s != 0u) counter_or(cnt, s);
      } else {
        const unsigned s = part[0][li][k] + part[1][li][k] + part[2][li][k] + part[3][li][k];
        if (s != 0u) counter_add(cnt, s);
      }
    }
  }
  counters_returned();                                 // every wave: its atomics have returned ...
  __syncthreads();                                     // ... before thread 0 takes the workgroup's ticket
  if (t == 0) last = take_ticket(a.counters + SCENE_TICKET);
  __syncthreads();
  if (!last) return;                                   // (uniform: `last` is a shared word)
  // the records' words, one lane each: stored once, plain vector stores
  for (int q = t; q < a.n * SCENE_RECORD_WORDS; q += SCENE_THREADS) {
    const int li = q / SCENE_RECORD_WORDS, k = q - li * SCENE_RECORD_WORDS;
    const unsigned* cnt = a.counters + (size_t)li * SCENE_WORDS;
    auto sum = [&](int j) { return counter_read(cnt + j); };
    unsigned r = 0u;
    switch (k) {   // se3tn_scene_fit: model, visible, hidden, seen, inlier, front, behind, sum_abs_mm, hidden_by, tol_mm, n_objects, 0
      case 0: r = sum(SC_MODEL); break;
      case 1: r = sum(SC_VISIBLE); break;
      case 2: r = sum(SC_MODEL) - sum(SC_VISIBLE); break;
      case 3: r = sum(SC_SEEN); break;
      case 4: r = sum(SC_INLIER); break;
      case 5: r = sum(SC_FRONT); break;
      case 6: r = sum(SC_BEHIND); break;
      case 7: r = sum(SCENE_SUM); break;
      case 8: r = sum(SCENE_BY); break;
      case 9: r = (unsigned)a.tol; break;
      case 10: r = (unsigned)a.n; break;
      default: break;
    }
    reinterpret_cast<unsigned*>(a.out)[q] = r;
  }
  __syncthreads();                                     // every sum has been read: re-arm
  if (t < a.n * SCENE_WORDS) counter_rearm(a.counters + t);
  if (t == 0) counter_rearm(a.counters + SCENE_TICKET);
  __threadfence_system();                              // (the records may live in mapped host memory)
}

hipError_t launch_scene_fit(const SceneArgs& a, hipStream_t st) {
  if (a.n < 1 || a.n > SceneArgs::MAX || a.plan.tiles_x < 1 || a.plan.tiles_y < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scene_fit_kernel, dim3((unsigned)a.plan.tiles_x * (unsigned)a.plan.tiles_y), dim3(SCENE_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace se3tn
