// Kernels of the batched select stage (include/emqx_select.h).
//
// Work is distributed BY CSR ENTRY, as deliver_kernels.hip distributes by delivery: a lane per
// entry, a tile of SL_TILE consecutive entries per block step, so a message that matched 5 000
// filters between empty ones spreads over 20 blocks.  A lane finds its message by a bounded
// binary search over the offsets (csr_find) and evaluates sl_entry (select.h, the code the
// host evaluator runs): the owners its entry adds to the message's set, deduplicated by looking
// back over the earlier entries of the same message, across wave and tile boundaries, back to
// offsets[i].  The entry count is read on the device as offsets[n]: the host sizes the grid by
// cap_in only and the blocks stride over the tiles that exist.
//
// An entry adds any number of owners, so the ranks are prefix sums of counts (stage_common.h's
// block_excl_scan), not ballots.  The passes, each a kernel
// boundary on the stream (no inter-block waiting):
//   1  select_count_kernel    by entry: entry_kept[d], the tile's sum, the summary counters (one
//                             atomic a counter a block);
//   2  select_macount_kernel  by message: the match-all owners that apply to each message (by
//                             the snapshot's per-class counts), their prefix within the tile of
//                             messages, the tile's sum;
//   3  select_scan_kernel     one block: exclusive scans, in place, of the entry tiles and of the
//                             message tiles; the totals;
//   4  select_write_kernel    by entry: position = the match-all owners of the messages up to
//                             and including its own + the owners of the earlier entries; writes
//                             the entry's owners; the first entry of a message writes
//                             out_offsets[i] and the message's match-all owners;
//   5  select_empty_kernel    by message: out_offsets and match-all owners of the messages
//                             without entries, and out_offsets[n];
//   6  select_finish_kernel   one block: per-message counts ([4], [7]), then the summary with
//                             plain stores from one lane (it may be host-pinned memory).
// Every index is bounded before use: an entry d < offsets[n] <= cap_in, a message index < n
// (<= n for out_offsets), a filter id < n_filters, an owner id < n_owners, a posting
// < n_postings, an output position < cap_out, a tile < ceil(cap_in / SL_TILE), a message tile
// < ceil(n / SL_TILE).  The only atomics are on the counters.
#include <hip/hip_runtime.h>

#include "select.h"

namespace emqx {

namespace {

constexpr uint32_t SL_WAVES = SL_TILE / 64;
constexpr uint32_t SL_MSG_BLOCKS = 16384;  // grid cap of the by-message passes

// offsets[n] when it is an entry count this call may use, else ~0 (the call is refused).
__device__ inline uint64_t sl_total(const SlArgs& a) {
  if (a.n == 0) return 0;
  const uint64_t t = a.offsets[a.n];
  return t <= a.cap_in ? t : ~0ull;
}

__device__ inline uint32_t sl_mask(const SlArgs& a, uint64_t i) { return a.msg_classes ? a.msg_classes[i] : 0xFFFFFFFFu; }

__global__ __launch_bounds__(SL_TILE) void select_count_kernel(SlArgs a) {
  __shared__ uint64_t part[4][SL_WAVES];
  const uint64_t total = sl_total(a);
  if (total == ~0ull) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t acc = 0;  // thread k < 4: kept, examined, dups, unknown of this block
  for (uint64_t tile = blockIdx.x; tile * SL_TILE < total; tile += gridDim.x) {
    const uint64_t d = tile * SL_TILE + threadIdx.x;
    SlCount c{0, 0, 0, 0};
    if (d < total) {
      const uint64_t i = csr_find(a.offsets, a.n, d);
      uint64_t s = a.offsets[i];
      if (s > d) s = d;  // offsets that are no CSR: the look-back stays below d
      c = sl_entry(a.v, a.filters, s, d, sl_mask(a, i), nullptr, 0);
      a.entry_kept[d] = c.kept;
    }
    const uint64_t w[4] = {wave_sum<uint64_t>(c.kept), wave_sum<uint64_t>(c.examined), wave_sum<uint64_t>(c.dups),
                           wave_sum<uint64_t>(c.unknown)};
    if (lane == 0)
      for (uint32_t k = 0; k < 4; ++k) part[k][wave] = w[k];
    __syncthreads();
    if (threadIdx.x < 4) {
      uint64_t s = 0;
      for (uint32_t k = 0; k < SL_WAVES; ++k) s += part[threadIdx.x][k];
      acc += s;
      if (threadIdx.x == 0) a.tile_base[tile] = s;  // scanned in place by pass 3
    }
    __syncthreads();
  }
  if (threadIdx.x >= 1 && threadIdx.x < 4 && acc) {
    const uint32_t word[4] = {0, SL_S_POSTINGS, SL_S_DUPS, SL_S_UNKNOWN};
    atomicAdd(a.ctr + word[threadIdx.x], static_cast<unsigned long long>(acc));
  }
}

__global__ __launch_bounds__(SL_TILE) void select_macount_kernel(SlArgs a) {
  __shared__ uint64_t ws[SL_WAVES];
  if (sl_total(a) == ~0ull) return;
  for (uint64_t tile = blockIdx.x; tile * SL_TILE < a.n; tile += gridDim.x) {
    const uint64_t j = tile * SL_TILE + threadIdx.x;
    const uint64_t c = j < a.n ? sl_match_all_count(a.v, sl_mask(a, j)) : 0;
    uint64_t sum;
    const uint64_t before = block_excl_scan<SL_TILE>(c, ws, &sum);
    if (j < a.n) a.ma_before[j] = before;
    if (threadIdx.x == 0) a.mtile_base[tile] = sum;  // scanned in place by pass 3
  }
}

__global__ __launch_bounds__(SL_SCAN_BLOCK) void select_scan_kernel(SlArgs a) {
  __shared__ uint64_t wsum[SL_SCAN_BLOCK / 64];
  const uint64_t total = sl_total(a);
  if (total == ~0ull) return;
  const uint32_t chunk = scan_chunk_of<SL_SCAN_BLOCK>(a.scan_chunk);
  const uint64_t by_entry =
      block_scan_in_place<SL_SCAN_BLOCK>(a.tile_base, a.tile_base, (total + SL_TILE - 1) / SL_TILE, wsum, chunk);
  const uint64_t by_all =
      block_scan_in_place<SL_SCAN_BLOCK>(a.mtile_base, a.mtile_base, (a.n + SL_TILE - 1) / SL_TILE, wsum, chunk);
  if (threadIdx.x == 0) {
    a.ctr[SL_C_ENTRY_TOTAL] = by_entry;
    a.ctr[SL_S_SELECTED] = by_entry + by_all;
  }
}

__global__ __launch_bounds__(SL_TILE) void select_write_kernel(SlArgs a) {
  __shared__ uint64_t ws[SL_WAVES];
  const uint64_t total = sl_total(a);
  if (total == ~0ull) return;
  const bool write = a.ctr[SL_S_SELECTED] <= a.cap_out;  // complete: pass 3 has finished; else out_offsets only
  for (uint64_t tile = blockIdx.x; tile * SL_TILE < total; tile += gridDim.x) {
    const uint64_t d = tile * SL_TILE + threadIdx.x;
    const bool valid = d < total;
    const uint32_t kept = valid ? a.entry_kept[d] : 0u;
    uint64_t sum;
    const uint64_t before = block_excl_scan<SL_TILE, uint64_t>(kept, ws, &sum);
    if (!valid) continue;  // no barrier follows in this step; every thread reaches the next step's scan
    const uint64_t i = csr_find(a.offsets, a.n, d);
    const uint32_t mask = sl_mask(a, i);
    const uint64_t own = sl_match_all_count(a.v, mask);
    // the owners of every earlier message and of this one's match-all list, then of the earlier entries
    const uint64_t ma = a.mtile_base[i / SL_TILE] + a.ma_before[i];
    const uint64_t pos = ma + own + a.tile_base[tile] + before;
    if (a.offsets[i] == d) {  // the first entry of a non-empty message
      const uint64_t at = pos - own;
      a.out_offsets[i] = at;
      if (write && own && at < a.cap_out) (void)sl_match_all(a.v, mask, a.out_owners + at, a.cap_out - at);
    }
    if (write && kept && pos < a.cap_out) {
      uint64_t s = a.offsets[i];
      if (s > d) s = d;
      (void)sl_entry(a.v, a.filters, s, d, mask, a.out_owners + pos, a.cap_out - pos);
    }
  }
}

// By message, after pass 4: a message without entries starts where the next message with entries
// starts, less the match-all owners in between (or at the end when none follows); index n gets
// the total.
__global__ __launch_bounds__(SL_TILE) void select_empty_kernel(SlArgs a) {
  const uint64_t total = sl_total(a);
  if (total == ~0ull) return;
  const uint64_t selected = a.ctr[SL_S_SELECTED];
  const bool write = selected <= a.cap_out;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * SL_TILE + threadIdx.x; j <= a.n;
       j += static_cast<uint64_t>(gridDim.x) * SL_TILE) {
    if (j == a.n) {
      a.out_offsets[j] = selected;
      continue;
    }
    const uint64_t d = a.offsets[j];
    if (d < total && a.offsets[j + 1] > d) continue;  // it has entries: pass 4 wrote it
    const uint64_t ma = a.mtile_base[j / SL_TILE] + a.ma_before[j];
    uint64_t by_entry = a.ctr[SL_C_ENTRY_TOTAL];  // no entry follows
    if (d < total) {
      const uint64_t i = csr_find(a.offsets, a.n, d);  // the last message that starts at d: the one with entries
      by_entry = a.out_offsets[i] - (a.mtile_base[i / SL_TILE] + a.ma_before[i]);
    }
    const uint64_t at = ma + by_entry;
    a.out_offsets[j] = at;
    if (write && a.v.n_match_all && at < a.cap_out)
      (void)sl_match_all(a.v, sl_mask(a, j), a.out_owners + at, a.cap_out - at);
  }
}

__global__ __launch_bounds__(SL_SCAN_BLOCK) void select_finish_kernel(SlArgs a) {
  __shared__ uint64_t part[2][SL_SCAN_BLOCK / 64];
  const uint64_t total = sl_total(a);
  const bool refused = total == ~0ull;
  uint64_t msgs = 0, most = 0;
  if (!refused)
    for (uint64_t j = threadIdx.x; j < a.n; j += SL_SCAN_BLOCK) {
      const uint64_t lo = a.out_offsets[j], hi = a.out_offsets[j + 1];
      const uint64_t c = hi > lo ? hi - lo : 0;
      msgs += c ? 1u : 0u;
      most = c > most ? c : most;
    }
  msgs = wave_sum(msgs);
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    const uint64_t y = __shfl_xor(most, d);
    most = y > most ? y : most;
  }
  if ((threadIdx.x & 63u) == 0) {
    part[0][threadIdx.x >> 6] = msgs;
    part[1][threadIdx.x >> 6] = most;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  msgs = 0;
  most = 0;
  for (uint32_t w = 0; w < SL_SCAN_BLOCK / 64; ++w) {
    msgs += part[0][w];
    most = part[1][w] > most ? part[1][w] : most;
  }
  uint64_t* s = a.summary;
  const uint64_t selected = refused ? 0 : a.ctr[SL_S_SELECTED];
  uint64_t flags = refused ? SL_F_INPUT_REFUSED : 0u;
  if (!refused && selected > a.cap_out) flags |= SL_F_OUT_OVERFLOW;
  s[SL_S_FLAGS] = flags;
  s[SL_S_ENTRIES] = a.n ? a.offsets[a.n] : 0;
  s[SL_S_POSTINGS] = refused ? 0 : a.ctr[SL_S_POSTINGS];
  s[SL_S_SELECTED] = selected;
  s[SL_S_MESSAGES] = msgs;
  s[SL_S_DUPS] = refused ? 0 : a.ctr[SL_S_DUPS];
  s[SL_S_UNKNOWN] = refused ? 0 : a.ctr[SL_S_UNKNOWN];
  s[SL_S_MAX] = most;
}

}  // namespace

// Enqueues the passes of one call; a.ctr must be zero when the stream reaches the first of them.
int sl_launch(const SlArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t tiles = (a.cap_in + SL_TILE - 1) / SL_TILE;
  const uint32_t cap = a.max_blocks ? a.max_blocks : 1u;
  const uint32_t blocks = static_cast<uint32_t>(tiles < cap ? tiles : cap);
  const uint64_t mtiles = (a.n + 1 + SL_TILE - 1) / SL_TILE;  // index n included
  const uint32_t mblocks = static_cast<uint32_t>(mtiles < SL_MSG_BLOCKS ? mtiles : SL_MSG_BLOCKS);
  if (a.n) {
    if (blocks) select_count_kernel<<<dim3(blocks), dim3(SL_TILE), 0, s>>>(a);
    select_macount_kernel<<<dim3(mblocks), dim3(SL_TILE), 0, s>>>(a);
    select_scan_kernel<<<dim3(1), dim3(SL_SCAN_BLOCK), 0, s>>>(a);
    if (blocks) select_write_kernel<<<dim3(blocks), dim3(SL_TILE), 0, s>>>(a);
  }
  select_empty_kernel<<<dim3(mblocks), dim3(SL_TILE), 0, s>>>(a);
  select_finish_kernel<<<dim3(1), dim3(SL_SCAN_BLOCK), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
