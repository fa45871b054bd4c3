// Stand-alone host check of csrc/pose_errors_plan.h (built with -fsanitize=address,undefined by tests/test_pose_errors_host.py): the
// tile, chunk, scratch and staging index arithmetic of se3tn_pose_errors, walked the way the launches walk it.  Every buffer is
// malloc'ed with EXACTLY the planned number of doubles, so an index past its end is a sanitizer report.  For model sizes at every
// edge of the tiling (1 .. 2^20 points) and pair counts at every edge of the chunking: every point is the query slot of exactly one
// (tile, slot, thread); every (pair of a chunk, tile) owns two scratch doubles of its own; the chunks cover [0, n) once, in order;
// the four staging regions of the host entry point tile the staging buffer.  Exits non-zero at the first mismatch.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pose_errors_plan.h"

using namespace se3tn;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static int check_model(int P) {
  const int tiles = pe_query_tiles(P);
  CHECK(tiles >= 1 && (long long)tiles * PE_QUERY_TILE >= P && (long long)(tiles - 1) * PE_QUERY_TILE < P);
  // query slots: each point exactly once, every other slot past the end
  std::vector<unsigned char> seen((size_t)P, 0);
  for (int tile = 0; tile < tiles; ++tile)
    for (int s = 0; s < PE_QPT; ++s)
      for (int t = 0; t < PE_THREADS; ++t) {
        const long long j = pe_query_index(tile, s, t);
        CHECK(j >= 0);
        if (j < P) { CHECK(seen[(size_t)j] == 0); seen[(size_t)j] = 1; }
      }
  for (int j = 0; j < P; ++j) CHECK(seen[(size_t)j] == 1);
  // reference tiles as the kernel's loop forms them: cover [0, P) once
  long long covered = 0;
  for (int r0 = 0; r0 < P; r0 += PE_REF_TILE) {
    const int cnt = P - r0 < PE_REF_TILE ? P - r0 : PE_REF_TILE;
    CHECK(cnt >= 1 && cnt <= PE_REF_TILE);
    covered += cnt;
  }
  CHECK(covered == P);
  // scratch of one chunk: two doubles per (pair, tile), nobody else's
  const size_t words = pe_scratch_doubles(P);
  double* part = (double*)std::malloc(words * sizeof(double));
  CHECK(part != nullptr);
  for (size_t i = 0; i < words; ++i) part[i] = -1.0;
  for (int pair = 0; pair < PE_CHUNK; ++pair)
    for (int tile = 0; tile < tiles; ++tile) {
      const size_t q = pe_partial_index(pair, tile, tiles);
      CHECK(part[q] == -1.0 && part[q + 1] == -1.0);
      part[q] = pair; part[q + 1] = tile;
    }
  for (size_t i = 0; i < words; ++i) CHECK(part[i] >= 0.0);
  std::free(part);
  return 0;
}

static int check_pairs(int n) {
  const int nch = pe_chunks(n);
  CHECK(nch >= 1);
  double* add = (double*)std::malloc((size_t)n * sizeof(double));
  double* stage = (double*)std::malloc(pe_stage_doubles(n) * sizeof(double));
  CHECK(add != nullptr && stage != nullptr);
  size_t next = 0;
  for (int c = 0; c < nch; ++c) {
    const PeChunk k = pe_chunk(n, c);
    CHECK(k.first == next && k.count >= 1 && k.count <= PE_CHUNK);
    for (int i = 0; i < k.count; ++i) add[k.first + i] = (double)c;   // where the finish launch of chunk c stores
    next = k.first + k.count;
  }
  CHECK(next == (size_t)n);
  // staging: [pred | gt | add | adds] tile the buffer
  CHECK(pe_stage_gt(n) == (size_t)n * 16 && pe_stage_add(n) == pe_stage_gt(n) + (size_t)n * 16);
  CHECK(pe_stage_adds(n) == pe_stage_add(n) + (size_t)n && pe_stage_doubles(n) == pe_stage_adds(n) + (size_t)n);
  for (size_t i = 0; i < (size_t)n * 16; ++i) { stage[i] = 1.0; stage[pe_stage_gt(n) + i] = 2.0; }
  for (size_t i = 0; i < (size_t)n; ++i) { stage[pe_stage_add(n) + i] = 3.0; stage[pe_stage_adds(n) + i] = 4.0; }
  double sum = 0.0;
  for (size_t i = 0; i < pe_stage_doubles(n); ++i) sum += stage[i];
  CHECK(sum == (double)n * (16 + 32 + 3 + 4));
  std::free(add);
  std::free(stage);
  return 0;
}

int main() {
  static_assert(PE_QUERY_TILE == PE_THREADS * PE_QPT, "a workgroup's query tile");
  static_assert(PE_CHUNK == SE3TN_POSE_ERRORS_CHUNK && PE_MAX_POINTS == SE3TN_POSE_ERRORS_MAX_POINTS, "the header's constants");
  const int Ps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2620, 4096, 8000, PE_MAX_POINTS - 1, PE_MAX_POINTS};
  for (int P : Ps)
    if (check_model(P)) { std::fprintf(stderr, "P = %d\n", P); return 1; }
  const int ns[] = {1, 2, 7, PE_CHUNK - 1, PE_CHUNK, PE_CHUNK + 1, 2 * PE_CHUNK, 2 * PE_CHUNK + 1, 2000, 100000};
  for (int n : ns)
    if (check_pairs(n)) { std::fprintf(stderr, "n = %d\n", n); return 1; }
  // the largest call the ABI can express, by arithmetic alone: no overflow in the chunk table or in the pose offsets
  const int big = INT_MAX;
  const int nch = pe_chunks(big);
  const PeChunk last = pe_chunk(big, nch - 1);
  CHECK(last.first + (size_t)last.count == (size_t)big && last.count >= 1 && last.count <= PE_CHUNK);
  CHECK(last.first * 16 / 16 == last.first && pe_stage_doubles(big) / 34 == (size_t)big);
  CHECK(pe_chunks(0) == 0 && pe_chunks(-5) == 0);
  CHECK(pe_query_tiles(PE_MAX_POINTS) == PE_MAX_POINTS / PE_QUERY_TILE);
  std::puts("pose_errors_plan_check: ok");
  return 0;
}
