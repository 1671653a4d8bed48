// What the stages around the match share (deliver, select, inbox, window, route, ack, retry, mqueue
// behind it and rel in front of it): the bounded searches over a CSR's offsets, the wave and block scans, the
// one-block scan of the tile totals, the counter report and the guard of the C ABI.  The first part
// is __host__ __device__ and compiles with a plain C++ compiler; the second is device code.
#pragma once
#include <stdint.h>

#include <new>

#include "../../include/emqx_match.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SC_HD __host__ __device__
#else
#define SC_HD
#endif

namespace emqx {

// The segment of position d: the last k in [0, n) with offsets[k] <= d (n >= 1), 0 when there is
// none.  At most 64 halvings whatever the offsets hold, and every index read lies in [0, n).
SC_HD inline uint64_t csr_find(const uint64_t* offsets, uint64_t n, uint64_t d) {
  uint64_t lo = 0, hi = n;  // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= d) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The first k in [lo, hi) with offsets[k] >= x (csr_lower) or > x (csr_upper), hi when there is
// none.  At most 64 halvings whatever the offsets hold, every index read lies in [lo, hi).
SC_HD inline uint64_t csr_lower(const uint64_t* offsets, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
SC_HD inline uint64_t csr_upper(const uint64_t* offsets, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// No exception (std::bad_alloc of the containers) crosses the C ABI.
template <class F>
int guarded(F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return EMQX_ENOMEM;
  } catch (...) {
    return EMQX_EINVAL;
  }
}

#if defined(__HIPCC__)
// Inclusive prefix sum of x over the wave.
template <class T>
__device__ inline T wave_incl_scan(T x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// Sum of x over the wave, in every lane.
template <class T>
__device__ inline T wave_sum(T x) {
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// Exclusive prefix sum of x over the BLOCK threads of the block; *all: the block's sum, in every
// thread.  `wsum` is [BLOCK / 64] of LDS.  Every thread of the block calls it, in uniform control
// flow.  The barrier contract, two barriers a call: the first stands in front of the write of
// wsum and says that the readers of the call before are done (and, to a caller, that every
// thread has got this far); the second publishes this call's wave sums.  After the return wsum
// is still being read: calls may follow each other directly, but a caller that writes wsum itself
// puts a barrier of its own in front.  A thread reads all BLOCK / 64 wave sums once: the running
// sum is the block's at the end and this thread's `before` when it passes the thread's wave.
template <uint32_t BLOCK, class T>
__device__ inline T block_excl_scan(T x, T* wsum, T* all) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const T incl = wave_incl_scan(x);
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < BLOCK / 64; ++w) {
    if (w == wave) before = sum;
    sum += wsum[w];
  }
  *all = sum;
  return before + incl - x;
}

// Tuning key "scan_chunk": the elements block_scan_in_place takes per carry step, 1..BLOCK.
template <uint32_t BLOCK>
__device__ inline uint32_t scan_chunk_of(uint32_t scan_chunk) {
  return scan_chunk && scan_chunk < BLOCK ? scan_chunk : BLOCK;
}

// One block of BLOCK threads: out[0, m) becomes carry0 plus the exclusive scan of in[0, m), `chunk`
// elements a carry step; returns carry0 plus the sum in every thread.  `in` and `out` may be the
// same array: a thread reads its element before it writes it and touches no other.  A thread at
// or beyond the chunk adds 0 and stores nothing but takes part in the shuffles and barriers.
// T is the accumulator; wsum and the barriers as in block_excl_scan, two a carry step.  The
// stores of the last carry step are ordered for the block's other threads by the next barrier only.
template <uint32_t BLOCK, class T, class In>
__device__ inline T block_scan_in_place(const In* in, T* out, uint64_t m, T* wsum, uint32_t chunk, T carry0 = 0) {
  T carry = carry0;
  for (uint64_t base = 0; base < m; base += chunk) {
    const uint64_t t = base + threadIdx.x;
    const bool mine = threadIdx.x < chunk && t < m;
    const T x = mine ? static_cast<T>(in[t]) : T(0);
    T all;
    const T before = block_excl_scan<BLOCK>(x, wsum, &all);
    if (mine) out[t] = carry + before;
    carry += all;
  }
  return carry;
}

// The block's sums of N per-thread values into ctr[word0 ..], and flag bits into ctr[flags_word].
// Every thread of the block calls it.
template <uint32_t N>
__device__ inline void block_report(unsigned long long* ctr, uint32_t word0, const uint64_t (&v)[N], uint32_t flags,
                                    uint32_t flags_word) {
  __shared__ unsigned long long red[N];
  __shared__ uint32_t red_flags;
  if (threadIdx.x < N) red[threadIdx.x] = 0;
  if (threadIdx.x == 0) red_flags = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t c = 0; c < N; ++c) {
    const uint64_t s = wave_sum(v[c]);
    if ((threadIdx.x & 63u) == 0 && s) atomicAdd(&red[c], static_cast<unsigned long long>(s));
  }
  if (flags) atomicOr(&red_flags, flags);
  __syncthreads();
  if (threadIdx.x < N && red[threadIdx.x]) atomicAdd(ctr + word0 + threadIdx.x, red[threadIdx.x]);
  if (threadIdx.x == N && red_flags) atomicOr(ctr + flags_word, static_cast<unsigned long long>(red_flags));
}
#endif

}  // namespace emqx
