// The reduction of the record kernels and their arrival-counter protocol, device only: fit_stats_kernel (K7 / K12) and
// scene_fit_kernel (K13) build on every piece, the other kernels on wave_sum alone.  DESIGN.md section 3, "What K7, K12 and K13 share".
//
// A record is integer sums over the workgroups of a launch.  Each workgroup reduces its part (wave64 shuffles, the four waves through
// LDS) and adds it into uint32 counters of the context with ONE returning agent-scope atomic per word: the workgroups run on several
// XCDs, and every access to a counter is an agent-scope atomic, so no L1 holds a stale copy.  Once those atomics have returned the
// workgroup takes a ticket; the workgroup whose ticket is the last one reads the sums, stores the finished record once with plain
// vector stores, zeroes counters and ticket for the next launch (counter_rearm) and ends with __threadfence_system(): the record
// may live in mapped host memory.
#pragma once
#include <hip/hip_runtime.h>

namespace se3tn {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// v[k] summed over the wave, lane 0 parks the sums in its wave's row of LDS (the caller's barrier follows)
template <int N>
__device__ __forceinline__ void wave_sums_to_lds(unsigned (&v)[N], unsigned (*part)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) part[threadIdx.x >> 6][k] = v[k];
  }
}

// ONE vector atomic per word and workgroup, in the returning form: the operation has been performed where the other XCDs' are by
// the time its result is back
__device__ __forceinline__ void counter_add(unsigned* word, unsigned s) {
  const unsigned old = __hip_atomic_fetch_add(word, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(old));
}
__device__ __forceinline__ void counter_or(unsigned* word, unsigned s) {
  const unsigned old = __hip_atomic_fetch_or(word, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(old));
}

// The workgroup's arrival.  Every wave that issued counter atomics calls counters_returned() first: its atomics have come back.
// Then ONE thread of the workgroup calls take_ticket() -- a lane of the only wave that added (K7 / K12), or thread 0 behind a
// barrier when every wave did (K13) -- and stores the result in a shared word, so that `last` is uniform after the next barrier.
__device__ __forceinline__ void counters_returned() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ bool take_ticket(unsigned* ticket) {
  return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
}

// the last workgroup: a finished sum, and the word (a sum or the ticket) zeroed for the next launch
__device__ __forceinline__ unsigned counter_read(const unsigned* word) {
  return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void counter_rearm(unsigned* word) { __hip_atomic_store(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace se3tn
