// Kernels of the batched enrich stage (include/emqx_deliver.h).
//
// Work is distributed BY DELIVERY: a lane per delivery, a tile of DV_TILE consecutive deliveries
// per block step, so a 10 K-subscriber message between empty ones spreads over 40 blocks instead
// of serialising on one wave.  A lane finds its message by a bounded binary search over the
// offsets (csr_find); the lanes of a wave mostly walk the same path, so the loads coalesce
// into broadcasts.  The delivery count is read on the device as offsets[n]: the host sizes the
// grid by cap_in only and the blocks stride over the tiles that exist.
//
// Compaction is the count / scan / write pattern of fanout_kernels.hip (fanout_count_kernel,
// fo_blocks_excl_scan, fanout_partials_kernel), by tile:
//   pass 1  deliver_eval_kernel     evaluates every delivery with dv_enrich (deliver.h, the code
//           the host evaluator runs), writes out_opts / out_subids, the tile's kept count (ballot
//           + popcount) and the summary counters (one atomic a counter a block);
//   pass 2  deliver_scan_kernel     one block: exclusive scan of the tile counts;
//   pass 3  deliver_scatter_kernel  writes each kept delivery at tile base + rank within the
//           tile; the lane whose delivery index equals offsets[i] writes kept_offsets[i]
//           (deliveries are ordered by message, so the stable global compaction is the
//           per-message one);
//   last    deliver_finish_kernel   by message: kept_offsets of the empty messages and of index
//           n, then the summary, with plain stores (it may be host-pinned memory).
// No inter-block waiting: every dependency is a kernel boundary on the stream.  Every index is
// bounded before use: d < offsets[n] <= cap_in, a message index < n, a kept position < cap_kept,
// a tile < ceil(cap_in / DV_TILE), a slot < n_slots.
#include <hip/hip_runtime.h>

#include "deliver.h"

namespace emqx {

namespace {

constexpr uint32_t DV_WAVES = DV_TILE / 64;

// offsets[n] when it is a delivery count this call may use, else ~0 (the call is refused).
__device__ inline uint64_t dv_total(const DvArgs& a) {
  if (a.n == 0) return 0;
  const uint64_t t = a.offsets[a.n];
  return t <= a.cap_in ? t : ~0ull;
}

__global__ __launch_bounds__(DV_TILE) void deliver_eval_kernel(DvArgs a) {
  __shared__ uint32_t part[6][DV_WAVES];
  const uint64_t total = dv_total(a);
  if (total == ~0ull) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t acc = 0;  // thread k < 6: counter k (kept, dropped, no_subopts, kept at qos 0 / 1 / 2) of this block
  for (uint64_t tile = blockIdx.x; tile * DV_TILE < total; tile += gridDim.x) {
    const uint64_t d = tile * DV_TILE + threadIdx.x;
    const bool valid = d < total;
    uint32_t o = 0;
    if (valid) {
      const uint64_t i = csr_find(a.offsets, a.n, d);
      uint32_t subid;
      o = dv_enrich(a.v, a.subs[d], a.filters[d], a.msg_qos[i], a.msg_flags[i],
                    a.msg_from ? a.msg_from[i] : DV_NO_SENDER, &subid);
      a.out_opts[d] = static_cast<uint8_t>(o);
      if (a.out_subids) a.out_subids[d] = subid;
    }
    const bool kept = valid && !(o & DV_OUT_DROP);
    const bool counted = kept && !(o & DV_OUT_BAD);
    const uint32_t c[6] = {
        static_cast<uint32_t>(__popcll(__ballot(kept))),
        static_cast<uint32_t>(__popcll(__ballot(valid && (o & DV_OUT_DROP)))),
        static_cast<uint32_t>(__popcll(__ballot(valid && (o & DV_OUT_NO_SUBOPTS)))),
        static_cast<uint32_t>(__popcll(__ballot(counted && (o & 3u) == 0u))),
        static_cast<uint32_t>(__popcll(__ballot(counted && (o & 3u) == 1u))),
        static_cast<uint32_t>(__popcll(__ballot(counted && (o & 3u) == 2u))),
    };
    if (lane == 0)
      for (uint32_t k = 0; k < 6; ++k) part[k][wave] = c[k];
    __syncthreads();
    if (threadIdx.x < 6) {
      uint32_t s = 0;
      for (uint32_t w = 0; w < DV_WAVES; ++w) s += part[threadIdx.x][w];
      acc += s;
      if (threadIdx.x == 0 && a.kept_offsets) a.tile_kept[tile] = s;
    }
    __syncthreads();
  }
  if (threadIdx.x < 6 && acc) atomicAdd(a.ctr + DV_S_KEPT + threadIdx.x, static_cast<unsigned long long>(acc));
}

// One block: tile_base = exclusive scan of tile_kept over the tiles of this call, scan_chunk
// tiles a carry step (stage_common.h's block_scan_in_place).
__global__ __launch_bounds__(DV_SCAN_BLOCK) void deliver_scan_kernel(DvArgs a) {
  __shared__ uint64_t wsum[DV_SCAN_BLOCK / 64];
  const uint64_t total = dv_total(a);
  if (total == ~0ull) return;
  (void)block_scan_in_place<DV_SCAN_BLOCK>(a.tile_kept, a.tile_base, (total + DV_TILE - 1) / DV_TILE, wsum,
                                           scan_chunk_of<DV_SCAN_BLOCK>(a.scan_chunk));
}

__global__ __launch_bounds__(DV_TILE) void deliver_scatter_kernel(DvArgs a) {
  __shared__ uint32_t wkept[DV_WAVES];
  const uint64_t total = dv_total(a);
  if (total == ~0ull) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t n_kept = a.ctr[DV_S_KEPT];  // complete: pass 1 has finished
  const bool write = n_kept <= a.cap_kept;   // else kept_offsets only
  for (uint64_t tile = blockIdx.x; tile * DV_TILE < total; tile += gridDim.x) {
    const uint64_t d = tile * DV_TILE + threadIdx.x;
    const bool valid = d < total;
    const uint32_t o = valid ? a.out_opts[d] : 0u;
    const bool kept = valid && !(o & DV_OUT_DROP);
    const unsigned long long b = __ballot(kept);
    if (lane == 0) wkept[wave] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < DV_WAVES; ++w)
      if (w < wave) before += wkept[w];
    // deliveries kept before d: the tile's base, the tile's earlier waves, the wave's earlier lanes
    const uint64_t pos = a.tile_base[tile] + before + static_cast<uint32_t>(__popcll(b & ((1ull << lane) - 1ull)));
    if (valid) {
      const uint64_t i = csr_find(a.offsets, a.n, d);
      if (a.offsets[i] == d) a.kept_offsets[i] = pos;  // the first delivery of a non-empty message
      if (kept && write && pos < a.cap_kept) {
        a.kept_subs[pos] = a.subs[d];
        a.kept_filters[pos] = a.filters[d];
        a.kept_opts[pos] = static_cast<uint8_t>(o);
        if (a.kept_subids) a.kept_subids[pos] = a.out_subids ? a.out_subids[d] : 0u;
      }
    }
    __syncthreads();
  }
}

// By message, after pass 3: an empty message's kept offset is that of the next non-empty one
// (found by the same search from its own offset), or the kept count when none follows; index n
// gets the kept count.  Then the summary.
__global__ __launch_bounds__(DV_TILE) void deliver_finish_kernel(DvArgs a) {
  const uint64_t total = dv_total(a);
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * DV_TILE + threadIdx.x;
  if (j == 0) {
    uint64_t* s = a.summary;
    const bool refused = total == ~0ull;
    const uint64_t kept = refused ? 0 : a.ctr[DV_S_KEPT];
    uint64_t flags = refused ? DV_F_INPUT_REFUSED : 0u;
    if (!refused && a.kept_offsets && kept > a.cap_kept) flags |= DV_F_KEPT_OVERFLOW;
    s[DV_S_FLAGS] = flags;
    s[DV_S_TOTAL] = a.n ? a.offsets[a.n] : 0;
    for (uint32_t k = DV_S_KEPT; k < DV_S_WORDS; ++k) s[k] = refused ? 0 : a.ctr[k];
  }
  if (total == ~0ull || !a.kept_offsets || j > a.n) return;
  const uint64_t n_kept = a.ctr[DV_S_KEPT];
  if (j == a.n) {
    a.kept_offsets[j] = n_kept;
    return;
  }
  const uint64_t d = a.offsets[j];
  if (d >= total) {
    a.kept_offsets[j] = n_kept;  // no delivery follows
  } else if (a.offsets[j + 1] <= d) {
    const uint64_t i = csr_find(a.offsets, a.n, d);  // the last message that starts at d: the non-empty one
    if (i != j) a.kept_offsets[j] = a.kept_offsets[i];
  }
}

}  // namespace

// Enqueues the passes of one call; a.ctr must be zero when the stream reaches the first of them.
int dv_launch(const DvArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t tiles = (a.cap_in + DV_TILE - 1) / DV_TILE;
  const uint32_t cap = a.max_blocks && a.max_blocks < DV_MAX_BLOCKS ? a.max_blocks : DV_MAX_BLOCKS;
  const uint32_t blocks = static_cast<uint32_t>(tiles < cap ? tiles : cap);
  if (a.n && blocks) {
    deliver_eval_kernel<<<dim3(blocks), dim3(DV_TILE), 0, s>>>(a);
    if (a.kept_offsets) {
      deliver_scan_kernel<<<dim3(1), dim3(DV_SCAN_BLOCK), 0, s>>>(a);
      deliver_scatter_kernel<<<dim3(blocks), dim3(DV_TILE), 0, s>>>(a);
    }
  }
  const uint64_t fin = a.kept_offsets ? (a.n + 1 + DV_TILE - 1) / DV_TILE : 1;
  if (fin > 0x7FFFFFFFull) return static_cast<int>(hipErrorInvalidValue);
  deliver_finish_kernel<<<dim3(static_cast<uint32_t>(fin)), dim3(DV_TILE), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
