// Kernels of the inbox stage (include/emqx_inbox.h): the message-major
// delivery CSR transposed into a subscriber-major one.
//
// Path 0 is an LSD radix sort of (subscriber, delivery position) on the key bits of sub_limit,
// 8 bits a pass (ib_passes: 1..4), over tiles of IB_TILE deliveries (IB_ROWS rows of IB_BLOCK).
// A pass is three kernels, every dependency a kernel boundary on the stream:
//   inbox_hist_kernel     per tile: the count of each digit (LDS, one add per distinct digit
//                         of a wave), stored digit-major, and the digit totals of the pass.  The
//                         first pass also derives each delivery's message from the offsets (the
//                         lanes of a wave walk the same search path), counts the non-empty
//                         messages and raises BAD_SUB;
//   inbox_scan_kernel     one block a digit: the digit's base (the totals below it) plus the
//                         exclusive scan of its tile counts;
//   inbox_scatter_kernel  per tile, a chunk of consecutive deliveries a wave: a delivery's rank
//                         among the equal digits of its row from eight ballots, the rows and
//                         waves before it from per-wave digit counts in LDS: the stable
//                         position.  The last pass writes the box_* payloads there instead of a
//                         permutation, and the sorted keys for the boundary step.
// The boundaries: a position heads an inbox when its key differs from the one before it.
//   inbox_heads_kernel    heads per tile;
//   inbox_hscan_kernel    one block: their exclusive scan, m;
//   inbox_starts_kernel   head of rank r: starts[r], inbox_subs[r], inbox_offsets[r];
//   inbox_longest_kernel  the longest extent between consecutive starts;
//   inbox_finish_kernel   inbox_offsets[m] and the summary, plain stores.
// Nothing depends on the order in which blocks or atomics run: the atomics are sums, an OR and a
// maximum, and every output position is a function of the input alone.
//
// Path 1 (the yardstick): inbox_prep_kernel pads the keys to cap_in (the count is known on the
// device only; the pad key sub_limit - 1 at the highest positions sorts last under a stable
// sort), rocprim::radix_sort_pairs, inbox_gather_kernel, then the same boundary kernels.
//
// Every index is bounded before use: d < offsets[n] <= cap_in, a message index < n, an output
// position < offsets[n], a tile < ceil(cap_in / IB_TILE), an inbox rank checked against
// cap_boxes.  The delivery count is read on the device; the host sizes the grids by cap_in.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "inbox.h"

namespace emqx {

namespace {

constexpr uint32_t IB_WAVES = IB_BLOCK / 64;
static_assert(IB_RADIX == IB_BLOCK, "thread t owns digit t");

// offsets[n] when it is a delivery count this call may use, else ~0 (the call is refused).
__device__ inline uint64_t ib_total(const IbArgs& a) {
  if (a.n > IB_MAX_TOTAL) return ~0ull;
  if (a.n == 0) return 0;
  const uint64_t t = a.offsets[a.n];
  return (t <= a.cap_in && t <= IB_MAX_TOTAL) ? t : ~0ull;
}

// The total, or ~0 when this kernel has nothing to do: a refused input, or (after the first
// kernel) a bad subscriber.
__device__ inline uint64_t ib_go(const IbArgs& a, bool first) {
  const uint64_t total = ib_total(a);
  if (total == ~0ull) return total;
  if (!first && (a.ctr[IB_S_FLAGS] & IB_F_BAD_SUB)) return ~0ull;
  return total;
}

// The lanes of the wave that are valid and hold the same digit as this lane.
__device__ inline uint64_t ib_peers(uint32_t digit, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < IB_DIGIT_BITS; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// What the first kernel over the input does for delivery d besides its key: the message index,
// the count of first deliveries (one a non-empty message), the subscriber bound.
__device__ inline void ib_first_look(const IbArgs& a, uint64_t d, uint32_t sub, uint32_t* msgs, bool* bad) {
  const uint64_t i = csr_find(a.offsets, a.n, d);
  a.msg_of[d] = static_cast<uint32_t>(i);
  if (a.offsets[i] == d) ++*msgs;
  if (sub >= a.sub_limit) *bad = true;
}

__device__ inline void ib_first_report(const IbArgs& a, uint32_t msgs, bool bad) {
  msgs = wave_sum(msgs);
  const bool any_bad = __any(bad);
  if ((threadIdx.x & 63u) == 0) {
    if (msgs) atomicAdd(a.ctr + IB_S_MSGS, static_cast<unsigned long long>(msgs));
    if (any_bad) atomicOr(a.ctr + IB_S_FLAGS, static_cast<unsigned long long>(IB_F_BAD_SUB));
  }
}

template <bool FIRST>
__global__ __launch_bounds__(IB_BLOCK) void inbox_hist_kernel(IbArgs a, uint32_t pass) {
  __shared__ uint32_t cnt[IB_RADIX];
  const uint64_t total = ib_go(a, FIRST);
  if (total == ~0ull) return;
  const uint64_t tiles = ib_tiles(total);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t* src = FIRST ? a.subs : a.key[(pass - 1) & 1];
  uint32_t msgs = 0;
  bool bad = false;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t key[IB_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < IB_ROWS; ++r) {  // the tile's loads are in flight together
      const uint64_t d = tile * IB_TILE + static_cast<uint64_t>(r) * IB_BLOCK + threadIdx.x;
      key[r] = d < total ? src[d] : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < IB_ROWS; ++r) {
      const uint64_t d = tile * IB_TILE + static_cast<uint64_t>(r) * IB_BLOCK + threadIdx.x;
      const bool valid = d < total;
      if (FIRST && valid) ib_first_look(a, d, key[r], &msgs, &bad);
      const uint32_t digit = ib_digit(key[r], pass);
      const uint64_t m = ib_peers(digit, valid);
      if (valid && (m & ((1ull << lane) - 1ull)) == 0) atomicAdd(&cnt[digit], static_cast<uint32_t>(__popcll(m)));
    }
    __syncthreads();
    const uint32_t c = cnt[threadIdx.x];
    a.tile_hist[static_cast<uint64_t>(threadIdx.x) * tiles + tile] = c;
    if (c) atomicAdd(a.digit_tot + pass * IB_RADIX + threadIdx.x, c);
    __syncthreads();
  }
  if (FIRST) ib_first_report(a, msgs, bad);
}

// Block `digit`: tile_hist[digit][*] becomes the position of the digit's first delivery of each
// tile: the deliveries of the lower digits, then the digit's deliveries of the earlier tiles
// (stage_common.h's block_scan_in_place from that start, scan_chunk tiles a carry step).
__global__ __launch_bounds__(IB_SCAN_BLOCK) void inbox_scan_kernel(IbArgs a, uint32_t pass) {
  __shared__ uint32_t wsum[IB_SCAN_BLOCK / 64];
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint64_t tiles = ib_tiles(total);
  const uint32_t digit = blockIdx.x;
  const uint32_t v = wave_sum(threadIdx.x < digit ? a.digit_tot[pass * IB_RADIX + threadIdx.x] : 0u);
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t below = 0;
  for (uint32_t w = 0; w < IB_SCAN_BLOCK / 64; ++w) below += wsum[w];
  // (the scan's first barrier: every thread has read wsum)
  uint32_t* hist = a.tile_hist + static_cast<uint64_t>(digit) * tiles;
  (void)block_scan_in_place<IB_SCAN_BLOCK>(hist, hist, tiles, wsum, scan_chunk_of<IB_SCAN_BLOCK>(a.scan_chunk), below);
}

// The payloads of the delivery at input position `src` written at inbox position `pos`.
__device__ inline void ib_write_box(const IbArgs& a, uint64_t pos, uint32_t src) {
  a.box_msgs[pos] = a.msg_of[src];
  a.box_filters[pos] = a.filters[src];
  if (a.box_opts) a.box_opts[pos] = a.opts[src];
  if (a.box_subids) a.box_subids[pos] = a.subids[src];
  if (a.box_src) a.box_src[pos] = src;
}

// A wave owns IB_CHUNK consecutive deliveries of the tile, IB_ROWS rows of 64: its loads are in
// flight together, and once the block has turned the waves' digit counts into starts (two
// barriers a tile) a wave ranks its rows on its own.
constexpr uint32_t IB_CHUNK = IB_TILE / IB_WAVES;
static_assert(IB_CHUNK == 64 * IB_ROWS, "a row of a wave is 64 deliveries");

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(IB_BLOCK) void inbox_scatter_kernel(IbArgs a, uint32_t pass) {
  // per wave and digit: the deliveries in the wave's chunk, then the position of its next one
  __shared__ uint32_t w_c[IB_WAVES][IB_RADIX];
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint64_t tiles = ib_tiles(total);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t* ksrc = FIRST ? a.subs : a.key[(pass - 1) & 1];
  const uint32_t* isrc = a.idx[(pass - 1) & 1];  // (not read by the first pass)
  uint32_t* kdst = a.key[pass & 1];
  uint32_t* idst = a.idx[pass & 1];
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (uint32_t w = 0; w < IB_WAVES; ++w) w_c[w][threadIdx.x] = 0;
    const uint64_t d0 = tile * IB_TILE + static_cast<uint64_t>(wave) * IB_CHUNK + lane;
    uint32_t key[IB_ROWS], src[IB_ROWS];
    uint64_t peers[IB_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < IB_ROWS; ++r) {
      const uint64_t d = d0 + r * 64;
      key[r] = d < total ? ksrc[d] : 0u;
      src[r] = FIRST ? static_cast<uint32_t>(d) : (d < total ? isrc[d] : 0u);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < IB_ROWS; ++r) {
      const bool valid = d0 + r * 64 < total;
      const uint32_t digit = ib_digit(key[r], pass);
      peers[r] = ib_peers(digit, valid);
      if (valid && (peers[r] & below) == 0) atomicAdd(&w_c[wave][digit], static_cast<uint32_t>(__popcll(peers[r])));
    }
    __syncthreads();
    {  // digit threadIdx.x: the tile's first position, then the waves' chunks in order
      uint32_t at = a.tile_hist[static_cast<uint64_t>(threadIdx.x) * tiles + tile];
      for (uint32_t w = 0; w < IB_WAVES; ++w) {
        const uint32_t c = w_c[w][threadIdx.x];
        w_c[w][threadIdx.x] = at;
        at += c;
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < IB_ROWS; ++r) {
      const bool valid = d0 + r * 64 < total;
      const uint32_t digit = ib_digit(key[r], pass);
      // deliveries of this digit before d: the earlier tiles, waves and rows, then the wave's
      // earlier lanes.  Every lane reads the digit's position before its first lane moves it on:
      // the wave's LDS operations run in program order.
      const uint64_t pos = static_cast<uint64_t>(valid ? w_c[wave][digit] : 0u) + __popcll(peers[r] & below);
      if (valid && (peers[r] & below) == 0) atomicAdd(&w_c[wave][digit], static_cast<uint32_t>(__popcll(peers[r])));
      if (valid && pos < total) {
        kdst[pos] = key[r];
        if (LAST) {
          if (src[r] < total) ib_write_box(a, pos, src[r]);
        } else {
          idst[pos] = src[r];
        }
      }
    }
    __syncthreads();  // the next tile zeroes the counts
  }
}

// ---- path 1: the library sort -----------------------------------------------------------------

// Keys and positions padded to cap_in: the count is not known on the host, the sort runs over
// the capacity.  The pad key is the largest key there is, at the highest positions: under a
// stable sort the pads end behind every delivery.
__global__ __launch_bounds__(IB_BLOCK) void inbox_prep_kernel(IbArgs a) {
  const uint64_t total = ib_go(a, true);
  if (total == ~0ull) return;
  uint32_t msgs = 0;
  bool bad = false;
  for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * IB_BLOCK + threadIdx.x; d < a.cap_in;
       d += static_cast<uint64_t>(gridDim.x) * IB_BLOCK) {
    uint32_t key = static_cast<uint32_t>(a.sub_limit - 1);
    if (d < total) {
      key = a.subs[d];
      ib_first_look(a, d, key, &msgs, &bad);
    }
    a.key[0][d] = key;
    a.idx[0][d] = static_cast<uint32_t>(d);
  }
  ib_first_report(a, msgs, bad);
}

__global__ __launch_bounds__(IB_BLOCK) void inbox_gather_kernel(IbArgs a) {
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * IB_BLOCK + threadIdx.x; k < total;
       k += static_cast<uint64_t>(gridDim.x) * IB_BLOCK) {
    const uint32_t src = a.idx[1][k];
    if (src < total) ib_write_box(a, k, src);
  }
}

// ---- the inbox boundaries over the sorted keys ------------------------------------------------

// Thread t of a tile owns its positions [t * IB_ROWS, (t + 1) * IB_ROWS): bit j of the result is
// set when position k0 + j heads an inbox.
__device__ inline uint32_t ib_head_bits(const uint32_t* keys, uint64_t total, uint64_t k0, uint32_t* mine) {
  uint32_t bits = 0;
  if (k0 >= total) return 0;
  uint32_t prev = k0 ? keys[k0 - 1] : 0u;
#pragma unroll
  for (uint32_t j = 0; j < IB_ROWS; ++j) {
    const uint64_t k = k0 + j;
    if (k >= total) break;
    const uint32_t key = keys[k];
    mine[j] = key;
    if (k == 0 || key != prev) bits |= 1u << j;
    prev = key;
  }
  return bits;
}

__global__ __launch_bounds__(IB_BLOCK) void inbox_heads_kernel(IbArgs a, const uint32_t* keys) {
  __shared__ uint32_t wsum[IB_WAVES];
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint64_t tiles = ib_tiles(total);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t mine[IB_ROWS];
    const uint32_t bits = ib_head_bits(keys, total, tile * IB_TILE + static_cast<uint64_t>(threadIdx.x) * IB_ROWS, mine);
    const uint32_t c = wave_sum<uint32_t>(__popc(bits));
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (uint32_t w = 0; w < IB_WAVES; ++w) s += wsum[w];
      a.tile_heads[tile] = s;
    }
    __syncthreads();
  }
}

// One block: tile_hbase = exclusive scan of tile_heads; their sum is m.
__global__ __launch_bounds__(IB_SCAN_BLOCK) void inbox_hscan_kernel(IbArgs a) {
  __shared__ uint32_t wsum[IB_SCAN_BLOCK / 64];
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint32_t m = block_scan_in_place<IB_SCAN_BLOCK>(a.tile_heads, a.tile_hbase, ib_tiles(total), wsum,
                                                        scan_chunk_of<IB_SCAN_BLOCK>(a.scan_chunk));
  if (threadIdx.x == 0) a.ctr[IB_S_BOXES] = m;
}

__global__ __launch_bounds__(IB_BLOCK) void inbox_starts_kernel(IbArgs a, const uint32_t* keys, uint32_t* starts) {
  __shared__ uint32_t wsum[IB_WAVES];
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint64_t tiles = ib_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t k0 = tile * IB_TILE + static_cast<uint64_t>(threadIdx.x) * IB_ROWS;
    uint32_t mine[IB_ROWS];
    const uint32_t bits = ib_head_bits(keys, total, k0, mine);
    uint32_t tile_heads;  // (not used: the scan kernel has the tile's base)
    // heads before this thread's first position
    uint64_t r = a.tile_hbase[tile] + block_excl_scan<IB_BLOCK, uint32_t>(__popc(bits), wsum, &tile_heads);
#pragma unroll
    for (uint32_t j = 0; j < IB_ROWS; ++j) {
      if (!(bits & (1u << j))) continue;
      const uint64_t k = k0 + j;
      if (r < total) starts[r] = static_cast<uint32_t>(k);
      if (r < a.cap_boxes) a.inbox_subs[r] = mine[j];
      if (r <= a.cap_boxes) a.inbox_offsets[r] = k;
      ++r;
    }
  }
}

__global__ __launch_bounds__(IB_BLOCK) void inbox_longest_kernel(IbArgs a, const uint32_t* starts) {
  const uint64_t total = ib_go(a, false);
  if (total == ~0ull) return;
  const uint64_t m = a.ctr[IB_S_BOXES] <= total ? a.ctr[IB_S_BOXES] : total;
  unsigned long long best = 0;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * IB_BLOCK + threadIdx.x; r < m;
       r += static_cast<uint64_t>(gridDim.x) * IB_BLOCK) {
    const uint64_t end = r + 1 < m ? starts[r + 1] : total;
    const uint64_t len = end - starts[r];
    if (len > best) best = len;
  }
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, 64);
    if (o > best) best = o;
  }
  if ((threadIdx.x & 63u) == 0 && best) atomicMax(a.ctr + IB_S_LONGEST, best);
}

__global__ void inbox_finish_kernel(IbArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t total = ib_total(a);
  uint64_t s[IB_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  s[IB_S_TOTAL] = (a.n && a.n <= IB_MAX_TOTAL) ? a.offsets[a.n] : 0;
  if (total == ~0ull) {
    s[IB_S_FLAGS] = IB_F_INPUT_REFUSED;
  } else if (a.ctr[IB_S_FLAGS] & IB_F_BAD_SUB) {
    s[IB_S_FLAGS] = IB_F_BAD_SUB;
    s[IB_S_MSGS] = a.ctr[IB_S_MSGS];
  } else {
    const uint64_t m = a.ctr[IB_S_BOXES];
    if (m > a.cap_boxes) s[IB_S_FLAGS] = IB_F_BOX_OVERFLOW;
    else a.inbox_offsets[m] = total;
    s[IB_S_BOXES] = m;
    s[IB_S_LONGEST] = a.ctr[IB_S_LONGEST];
    s[IB_S_MSGS] = a.ctr[IB_S_MSGS];
  }
  for (uint32_t k = 0; k < IB_S_WORDS; ++k) a.summary[k] = s[k];
}

uint32_t sort_end_bit(uint64_t sub_limit) {
  const uint32_t b = ib_key_bits(sub_limit);
  return b ? b : 1u;
}

template <bool FIRST>
void launch_pass(const IbArgs& a, uint32_t pass, bool last, uint32_t blocks, hipStream_t s) {
  inbox_hist_kernel<FIRST><<<dim3(blocks), dim3(IB_BLOCK), 0, s>>>(a, pass);
  inbox_scan_kernel<<<dim3(IB_RADIX), dim3(IB_SCAN_BLOCK), 0, s>>>(a, pass);
  if (last) inbox_scatter_kernel<FIRST, true><<<dim3(blocks), dim3(IB_BLOCK), 0, s>>>(a, pass);
  else inbox_scatter_kernel<FIRST, false><<<dim3(blocks), dim3(IB_BLOCK), 0, s>>>(a, pass);
}

}  // namespace

uint64_t ib_sort_temp_bytes(uint64_t cap_in, uint64_t sub_limit) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                  static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                  static_cast<size_t>(cap_in), 0u, sort_end_bit(sub_limit));
  return bytes;
}

// Enqueues the passes of one call; a.ctr and a.digit_tot must be zero when the stream reaches
// the first of them.
int ib_launch(const IbArgs& a, int path, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t tiles = ib_tiles(a.cap_in);
  const uint32_t cap = a.max_blocks && a.max_blocks < IB_MAX_BLOCKS ? a.max_blocks : IB_MAX_BLOCKS;
  const uint32_t blocks = static_cast<uint32_t>(tiles < cap ? tiles : cap);
  if (a.n && blocks) {
    const uint32_t passes = ib_passes(a.sub_limit);
    const uint32_t* sorted;
    uint32_t* starts;
    if (path == 0) {
      launch_pass<true>(a, 0, passes == 1, blocks, s);
      for (uint32_t p = 1; p < passes; ++p) launch_pass<false>(a, p, p + 1 == passes, blocks, s);
      sorted = a.key[(passes - 1) & 1];
      starts = a.idx[(passes - 1) & 1];  // the last pass reads the other one and writes neither
    } else {
      const uint64_t rows = (a.cap_in + IB_BLOCK - 1) / IB_BLOCK;
      const uint32_t flat = static_cast<uint32_t>(rows < cap ? rows : cap);
      inbox_prep_kernel<<<dim3(flat), dim3(IB_BLOCK), 0, s>>>(a);
      size_t tb = a.sort_temp_bytes;
      const hipError_t e = rocprim::radix_sort_pairs(a.sort_temp, tb, a.key[0], a.key[1], a.idx[0], a.idx[1],
                                                     static_cast<size_t>(a.cap_in), 0u, sort_end_bit(a.sub_limit), s);
      if (e != hipSuccess) return static_cast<int>(e);
      inbox_gather_kernel<<<dim3(flat), dim3(IB_BLOCK), 0, s>>>(a);
      sorted = a.key[1];
      starts = a.idx[0];
    }
    inbox_heads_kernel<<<dim3(blocks), dim3(IB_BLOCK), 0, s>>>(a, sorted);
    inbox_hscan_kernel<<<dim3(1), dim3(IB_SCAN_BLOCK), 0, s>>>(a);
    inbox_starts_kernel<<<dim3(blocks), dim3(IB_BLOCK), 0, s>>>(a, sorted, starts);
    const uint64_t rows = (a.cap_in + IB_BLOCK - 1) / IB_BLOCK;
    const uint32_t lcap = cap < IB_LONGEST_BLOCKS ? cap : IB_LONGEST_BLOCKS;
    inbox_longest_kernel<<<dim3(static_cast<uint32_t>(rows < lcap ? rows : lcap)), dim3(IB_BLOCK), 0, s>>>(a, starts);
  }
  inbox_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
