// Tile, chunk and scratch index arithmetic of se3tn_pose_errors (pose_errors.hip, api.cpp).  Host and device; no HIP header is
// needed to read it (tests/c_abi/pose_errors_plan_check.cpp runs it on the host under sanitizers).
//
// A launch covers one CHUNK of up to PE_CHUNK pose pairs: grid = (query tiles of the model, pairs of the chunk).  A workgroup of
// PE_THREADS threads owns PE_QUERY_TILE = PE_THREADS x PE_QPT query points: thread t holds points q0 + s PE_THREADS + t, s < PE_QPT.
// The reference cloud passes through LDS in tiles of PE_REF_TILE points.  Workgroup (tile, pair) leaves two partial sums at
// pe_partial_index(pair, tile, tiles); the finish launch adds a pair's tiles in index order.
#pragma once
#include <stddef.h>

#include "../../include/se3tracknet.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3TN_PE_HD __host__ __device__
#else
#define SE3TN_PE_HD
#endif

namespace se3tn {

constexpr int PE_THREADS = 256;
constexpr int PE_QPT = 4;                               // query points a thread keeps in registers
constexpr int PE_QUERY_TILE = PE_THREADS * PE_QPT;      // 1,024 query points per workgroup
constexpr int PE_REF_TILE = 1024;                       // reference points per LDS tile: 3 x 8 KB, structure of arrays
constexpr int PE_CHUNK = SE3TN_POSE_ERRORS_CHUNK;       // pairs per launch (grid.y)
constexpr int PE_MAX_POINTS = SE3TN_POSE_ERRORS_MAX_POINTS;
static_assert(PE_CHUNK >= 1 && PE_CHUNK <= 65535, "a chunk is grid.y of one launch");

// query tiles of a model of P points (1 <= P <= PE_MAX_POINTS: at most 1,024)
SE3TN_PE_HD inline int pe_query_tiles(int P) { return (int)(((long long)P + PE_QUERY_TILE - 1) / PE_QUERY_TILE); }
// doubles of partial-sum scratch a model of P points needs: [PE_CHUNK][tiles][2] (sum of |a - b| , sum of closest distances)
SE3TN_PE_HD inline size_t pe_scratch_doubles(int P) { return (size_t)PE_CHUNK * (size_t)pe_query_tiles(P) * 2; }
// where workgroup (tile, pair of the chunk) stores its two sums
SE3TN_PE_HD inline size_t pe_partial_index(int pair_in_chunk, int tile, int tiles) {
  return ((size_t)pair_in_chunk * (size_t)tiles + (size_t)tile) * 2;
}
// the chunks of a call of n pairs: chunk c covers pairs [first, first + count)
SE3TN_PE_HD inline int pe_chunks(int n) { return n < 1 ? 0 : (int)(((long long)n + PE_CHUNK - 1) / PE_CHUNK); }
struct PeChunk {
  size_t first;
  int count;
};
SE3TN_PE_HD inline PeChunk pe_chunk(int n, int c) {
  PeChunk k;
  k.first = (size_t)c * PE_CHUNK;
  const size_t left = (size_t)n - k.first;
  k.count = left < (size_t)PE_CHUNK ? (int)left : PE_CHUNK;
  return k;
}
// index of query slot s of thread t in query tile `tile` (may be >= P: that slot is empty)
SE3TN_PE_HD inline long long pe_query_index(int tile, int s, int t) {
  return (long long)tile * PE_QUERY_TILE + (long long)s * PE_THREADS + t;
}
// staging of se3tn_pose_errors_host for n pairs, in doubles: [pred n x 16 | gt n x 16 | add n | adds n]
SE3TN_PE_HD inline size_t pe_stage_doubles(int n) { return (size_t)n * 34; }
SE3TN_PE_HD inline size_t pe_stage_gt(int n) { return (size_t)n * 16; }
SE3TN_PE_HD inline size_t pe_stage_add(int n) { return (size_t)n * 32; }
SE3TN_PE_HD inline size_t pe_stage_adds(int n) { return (size_t)n * 33; }

}  // namespace se3tn
