// Kernels of the window stage (include/emqx_window.h): inflight and mqueue
// admission of every inbox of a batch.
//
// An opts byte alone says whether a delivery is live with q > 0 or live with q = 0.  One global
// exclusive prefix count of both indicators over all deliveries removes the segments: the counts
// of inbox k are the prefix at its end minus the prefix at its head, and a delivery's ranks are
// its own prefix minus the prefix at its inbox's head.  Tiles of WN_TILE deliveries, WN_ROWS
// consecutive ones a thread, every dependency a kernel boundary on the stream:
//   window_heads_kernel    per tile: the block scan of the indicators; the tile's totals; for
//                          every inbox whose head lies in the tile (the extent of inbox indices
//                          from two binary searches in inbox_offsets) the prefix between the
//                          tile's start and the head;
//   window_scan_kernel     one block: the exclusive scan of the tile totals; zeroes the counters;
//   window_verdict_kernel  per tile: the heads in the tile marked in LDS with their inbox index,
//                          the block scan again, now also ranking the heads, so that a delivery
//                          knows the slot of its inbox; a thread a slot loads the session record
//                          once (two 16-byte loads), derives the inbox's plan in closed form
//                          (wn_plan) and leaves it in LDS; the slot whose head lies in the tile
//                          writes the record after the batch and the counts; then every lane
//                          takes its verdict and id from the plan and its ranks (wn_verdict) and
//                          stores 8 + 16 bytes a thread;
//   window_writeback_kernel  only with update_table: the records after the batch go back to the
//                          table (behind the kernel in which every tile of a long inbox read the
//                          record at entry);
//   window_finish_kernel   the summary, plain stores.
// Path 1 (the yardstick): window_zero_kernel, then window_wave_kernel, one wave an inbox walking it
// twice; the same bytes for offsets that start at 0 and do not decrease.
// On path 0 no thread or wave iterates over an inbox: the time of a call does not depend on how the
// deliveries are spread over the inboxes.  Nothing depends on the order in which blocks or atomics
// run: the atomics are sums and an OR, every output byte is a function of the input alone.
//
// Every index is bounded before use: a position < inbox_offsets[m] <= cap_in, an inbox index
// <= m <= cap_boxes, a subscriber id < sub_limit, a tile < max(1, ceil(cap_in / WN_TILE)), a slot
// < WN_TILE.  Both counts are read on the device; the host sizes the grids by cap_in.
#include <hip/hip_runtime.h>

#include "window.h"

namespace emqx {

namespace {

constexpr uint32_t WN_WAVES = WN_BLOCK / 64;
constexpr uint32_t WN_NONE = ~0u;

// m and inbox_offsets[m] when this call may use them; false: the call is refused.
__device__ inline bool wn_counts(const WnArgs& a, uint64_t* m, uint64_t* total) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  *total = 0;
  if (*m > a.cap_boxes || *m > WN_MAX_TOTAL) return false;
  *total = a.inbox_offsets[*m];
  return *total <= a.cap_in && *total <= WN_MAX_TOTAL;
}

__device__ inline uint64_t wn_tiles_eff(uint64_t total) {  // a call without deliveries still has its inboxes
  const uint64_t t = wn_tiles(total);
  return t ? t : 1;
}

// The opts bytes of positions p0 .. p0 + WN_ROWS; behind `total`: a byte that is not live.
__device__ inline void wn_load_opts(const uint8_t* opts, uint64_t p0, uint64_t total, uint8_t o[WN_ROWS]) {
  if (p0 + WN_ROWS <= total && ((reinterpret_cast<uintptr_t>(opts) + p0) & 7u) == 0) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(opts + p0);
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) o[j] = static_cast<uint8_t>(w >> (8 * j));
  } else {
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) o[j] = p0 + j < total ? opts[p0 + j] : WN_O_BAD;
  }
}

// What a delivery adds to the block scans: three packed 16-bit fields, whose sums never carry (a
// tile holds 2048 deliveries).
constexpr uint64_t WN_ONE_A = 1ull, WN_ONE_Z = 1ull << 16, WN_ONE_H = 1ull << 32;
__device__ inline uint64_t wn_indicator(uint8_t o) {
  const uint32_t l = wn_live(o);
  return l == 2 ? WN_ONE_A : (l == 1 ? WN_ONE_Z : 0ull);
}
// tile-local packing (16-bit fields) to the global one (q > 0 low, q = 0 high)
__device__ inline uint64_t wn_widen(uint64_t x) { return (x & 0xFFFFu) | (((x >> 16) & 0xFFFFu) << 32); }

// The global prefix at the head of inbox k (k <= m): the tile's base plus the part inside it.
__device__ inline uint64_t wn_base(const WnArgs& a, uint64_t k, uint64_t total, uint64_t tiles) {
  const uint64_t off = a.inbox_offsets[k];
  const uint64_t p = off < total ? off : total;
  uint64_t t = p / WN_TILE;
  if (t >= tiles) t = tiles - 1;
  return a.tile_tot[t] + a.head_pre[k];
}

__global__ __launch_bounds__(WN_BLOCK) void window_heads_kernel(WnArgs a) {
  __shared__ uint32_t pre[WN_TILE + 1];  // exclusive prefix at every position of the tile, and at its end
  __shared__ uint64_t wsum[WN_WAVES];
  uint64_t m, total;
  if (!wn_counts(a, &m, &total)) return;
  const uint64_t tiles = wn_tiles_eff(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * WN_TILE;
    const bool last = tile + 1 == tiles;
    uint8_t o[WN_ROWS];
    wn_load_opts(a.box_opts, ts + static_cast<uint64_t>(threadIdx.x) * WN_ROWS, total, o);
    uint64_t x = 0;
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) x += wn_indicator(o[j]);
    uint64_t all;
    uint64_t run = block_excl_scan<WN_BLOCK>(x, wsum, &all);
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) {
      pre[threadIdx.x * WN_ROWS + j] = static_cast<uint32_t>(run);
      run += wn_indicator(o[j]);
    }
    if (threadIdx.x == 0) {
      pre[WN_TILE] = static_cast<uint32_t>(all);
      a.tile_tot[tile] = wn_widen(all);
    }
    __syncthreads();
    // the inboxes whose head lies in [ts, ts + WN_TILE); the last tile also takes the heads at
    // its end (inboxes without deliveries behind the last delivery, and inbox_offsets[m] itself)
    const uint64_t k_lo = csr_lower(a.inbox_offsets, 0, m + 1, ts);
    const uint64_t k_hi = last ? m + 1 : csr_lower(a.inbox_offsets, 0, m + 1, ts + WN_TILE);
    for (uint64_t k = k_lo + threadIdx.x; k < k_hi; k += WN_BLOCK) {
      const uint64_t off = a.inbox_offsets[k];
      const uint64_t p = off < total ? off : total;
      if (p >= ts && p - ts <= (last ? WN_TILE : WN_TILE - 1)) a.head_pre[k] = wn_widen(pre[p - ts]);
    }
    __syncthreads();  // the next tile writes pre
  }
}

// One block: tile_tot becomes its exclusive scan (neither half reaches 2^32: no carry between them),
// scan_chunk tiles a carry step (stage_common.h's block_scan_in_place).
__global__ __launch_bounds__(WN_SCAN_BLOCK) void window_scan_kernel(WnArgs a) {
  __shared__ uint64_t wsum[WN_SCAN_BLOCK / 64];
  if (threadIdx.x < WN_S_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m, total;
  if (!wn_counts(a, &m, &total)) return;
  (void)block_scan_in_place<WN_SCAN_BLOCK>(a.tile_tot, a.tile_tot, wn_tiles_eff(total), wsum,
                                           scan_chunk_of<WN_SCAN_BLOCK>(a.scan_chunk));
}

__device__ inline WnRec wn_load_rec(const WnRec* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  WnRec r;
  r.inflight = lo.x;
  r.inflight_max = lo.y;
  r.mq_len = lo.z;
  r.mq_max = lo.w;
  r.next_pkt_id = hi.x;
  r.flags = hi.y;
  r.dropped = static_cast<uint64_t>(hi.z) | (static_cast<uint64_t>(hi.w) << 32);
  return r;
}

__device__ inline void wn_store_rec(WnRec* p, const WnRec& r) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(r.inflight, r.inflight_max, r.mq_len, r.mq_max);
  q[1] = make_uint4(r.next_pkt_id, r.flags, static_cast<uint32_t>(r.dropped), static_cast<uint32_t>(r.dropped >> 32));
}

// Per-thread sums of the inboxes this thread wrote.
struct WnAcc {
  uint64_t v[5] = {0, 0, 0, 0, 0};  // sends, sends0, queued, drops, wrapped
  bool bad = false;
};

// Inbox k (k < m) with A and Z live deliveries: its plan; when `own`, also its outputs.
__device__ inline WnPlan wn_inbox(const WnArgs& a, uint64_t k, uint32_t A, uint32_t Z, bool own, WnAcc* acc) {
  const uint32_t sub = a.inbox_subs[k];
  const bool ok = sub < a.sub_limit;
  WnRec rec{0, 0, 0, 0, 0, 0, 0};
  if (ok) rec = wn_load_rec(a.sessions + sub);
  WnTotals t;
  const WnPlan p = wn_plan(ok, &rec, A, Z, &t);
  if (own) {
    wn_store_rec(a.out_sessions + k, rec);
    *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = make_uint4(t.sends, t.sends0, t.queued, t.evicted_old);
    acc->v[0] += t.sends;
    acc->v[1] += t.sends0;
    acc->v[2] += t.queued;
    acc->v[3] += t.drops;
    acc->v[4] += t.wrapped;
    if (!ok) acc->bad = true;
  }
  return p;
}

// The block's sums into the counters.  Every thread of the block calls it.
__device__ inline void wn_report(const WnArgs& a, const WnAcc& acc) {
  block_report<5>(a.ctr, WN_S_SENDS, acc.v, acc.bad ? WN_F_BAD_SUB : 0u, WN_S_FLAGS);
}

__global__ __launch_bounds__(WN_BLOCK) void window_verdict_kernel(WnArgs a) {
  // hk: first the inbox index + 1 of the head at each position, then of each slot
  __shared__ uint32_t hk[WN_TILE];
  __shared__ uint32_t s_ba[WN_TILE], s_bz[WN_TILE], s_sends[WN_TILE], s_qd[WN_TILE], s_ev[WN_TILE], s_pm[WN_TILE];
  __shared__ uint64_t wsum[WN_WAVES];
  uint64_t m, total;
  if (!wn_counts(a, &m, &total)) return;
  const uint64_t tiles = wn_tiles_eff(total);
  WnAcc acc;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * WN_TILE;
    const bool last = tile + 1 == tiles;
    const uint32_t valid = static_cast<uint32_t>(total - ts < WN_TILE ? total - ts : WN_TILE);
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) hk[j * WN_BLOCK + threadIdx.x] = 0;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * WN_ROWS;
    uint8_t o[WN_ROWS];
    wn_load_opts(a.box_opts, p0, total, o);
    const uint64_t tile_base = a.tile_tot[tile];
    __syncthreads();
    // the inboxes whose head lies in the tile: one with deliveries marks its head; one without
    // has no delivery that would need its plan and is finished here
    const uint64_t k_lo = csr_lower(a.inbox_offsets, 0, m, ts);
    const uint64_t k_hi = last ? m : csr_lower(a.inbox_offsets, 0, m, ts + WN_TILE);
    for (uint64_t k = k_lo + threadIdx.x; k < k_hi; k += WN_BLOCK) {
      const uint64_t off = a.inbox_offsets[k], nxt = a.inbox_offsets[k + 1];
      const uint64_t p = off < total ? off : total, pn = nxt < total ? nxt : total;
      if (p < ts || (!last && p - ts >= WN_TILE)) continue;
      if (pn > p && p - ts < valid) atomicMax(&hk[p - ts], static_cast<uint32_t>(k + 1));
      else (void)wn_inbox(a, k, 0, 0, true, &acc);
    }
    __syncthreads();
    uint32_t hv[WN_ROWS];
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) hv[j] = hk[threadIdx.x * WN_ROWS + j];
    if (threadIdx.x == 0 && hv[0] == 0 && valid) {
      // the inbox that reaches into the tile: the last one whose head is at or before ts
      hv[0] = static_cast<uint32_t>(csr_lower(a.inbox_offsets, 0, m, ts + 1));
    }
    uint64_t x = 0;
#pragma unroll
    for (uint32_t j = 0; j < WN_ROWS; ++j) x += wn_indicator(o[j]) + (hv[j] ? WN_ONE_H : 0ull);
    uint64_t all;
    const uint64_t excl = block_excl_scan<WN_BLOCK>(x, wsum, &all);  // (its first barrier: every hk has been read)
    {
      uint64_t run = excl;
#pragma unroll
      for (uint32_t j = 0; j < WN_ROWS; ++j) {
        if (hv[j]) hk[static_cast<uint32_t>(run >> 32)] = hv[j];  // slot = heads before this one
        run += wn_indicator(o[j]) + (hv[j] ? WN_ONE_H : 0ull);
      }
    }
    const uint32_t slots = static_cast<uint32_t>(all >> 32);
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < slots; r += WN_BLOCK) {
      const uint64_t k = hk[r] - 1u;  // (k < m: a marked head or the search's result - 1)
      const uint64_t b0 = wn_base(a, k, total, tiles), b1 = wn_base(a, k + 1, total, tiles);
      const uint32_t A = static_cast<uint32_t>(b1) - static_cast<uint32_t>(b0);
      const uint32_t Z = static_cast<uint32_t>(b1 >> 32) - static_cast<uint32_t>(b0 >> 32);
      const WnPlan p = wn_inbox(a, k, A, Z, a.inbox_offsets[k] >= ts, &acc);
      s_ba[r] = static_cast<uint32_t>(b0);
      s_bz[r] = static_cast<uint32_t>(b0 >> 32);
      s_sends[r] = p.sends;
      s_qd[r] = p.qd;
      s_ev[r] = p.ev;
      s_pm[r] = p.pkt0 | (p.mode << 16);
    }
    __syncthreads();
    if (p0 < total) {
      uint8_t v[WN_ROWS];
      uint16_t id[WN_ROWS];
      uint64_t run = excl;
      const uint32_t ga = static_cast<uint32_t>(tile_base), gz = static_cast<uint32_t>(tile_base >> 32);
#pragma unroll
      for (uint32_t j = 0; j < WN_ROWS; ++j) {
        const uint32_t r = static_cast<uint32_t>(run >> 32) + (hv[j] ? 1u : 0u) - 1u;  // heads up to here, less one
        WnPlan p{WN_M_NONE, 0, 0, 0, WN_NONE};
        uint32_t ra = 0, rz = 0;
        if (r < WN_TILE) {  // (no inbox holds this position otherwise: the offsets do not start at 0)
          const uint32_t pm = s_pm[r];
          p = WnPlan{pm >> 16, s_sends[r], pm & 0xFFFFu, s_qd[r], s_ev[r]};
          ra = ga + static_cast<uint32_t>(run & 0xFFFFu) - s_ba[r];
          rz = gz + static_cast<uint32_t>((run >> 16) & 0xFFFFu) - s_bz[r];
        }
        v[j] = wn_verdict(p, o[j], ra, rz, &id[j]);
        run += wn_indicator(o[j]) + (hv[j] ? WN_ONE_H : 0ull);
      }
      const bool full = p0 + WN_ROWS <= total;
      if (full && ((reinterpret_cast<uintptr_t>(a.verdicts) + p0) & 7u) == 0) {
        uint64_t w = 0;
#pragma unroll
        for (uint32_t j = 0; j < WN_ROWS; ++j) w |= static_cast<uint64_t>(v[j]) << (8 * j);
        *reinterpret_cast<uint64_t*>(a.verdicts + p0) = w;
      } else {
#pragma unroll
        for (uint32_t j = 0; j < WN_ROWS; ++j)
          if (p0 + j < total) a.verdicts[p0 + j] = v[j];
      }
      if (full && ((reinterpret_cast<uintptr_t>(a.pkt_ids) + 2 * p0) & 15u) == 0) {
        *reinterpret_cast<uint4*>(a.pkt_ids + p0) =
            make_uint4(id[0] | (static_cast<uint32_t>(id[1]) << 16), id[2] | (static_cast<uint32_t>(id[3]) << 16),
                       id[4] | (static_cast<uint32_t>(id[5]) << 16), id[6] | (static_cast<uint32_t>(id[7]) << 16));
      } else {
#pragma unroll
        for (uint32_t j = 0; j < WN_ROWS; ++j)
          if (p0 + j < total) a.pkt_ids[p0 + j] = id[j];
      }
    }
    __syncthreads();  // the next tile zeroes hk and rewrites the plans
  }
  wn_report(a, acc);
}

// ---- path 1: the yardstick, one wave an inbox --------------------------------------------------

__global__ void window_zero_kernel(WnArgs a) {
  if (blockIdx.x == 0 && threadIdx.x < WN_S_WORDS) a.ctr[threadIdx.x] = 0;
}

// A wave walks its inbox twice, 64 deliveries a step: once for the two live counts, once for the
// verdicts, the ranks from ballots.  Its time grows with the inbox: what path 0 is measured against.
__global__ __launch_bounds__(WN_BLOCK) void window_wave_kernel(WnArgs a) {
  uint64_t m, total;
  if (!wn_counts(a, &m, &total)) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * WN_WAVES;
  WnAcc acc, none;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * WN_WAVES + (threadIdx.x >> 6); k < m; k += waves) {
    const uint64_t off = a.inbox_offsets[k], nxt = a.inbox_offsets[k + 1];
    const uint64_t lo = off < total ? off : total;
    const uint64_t hi = nxt < lo ? lo : (nxt < total ? nxt : total);
    uint32_t A = 0, Z = 0;
    for (uint64_t base = lo; base < hi; base += 64) {
      const uint32_t l = base + lane < hi ? wn_live(a.box_opts[base + lane]) : 0u;
      A += static_cast<uint32_t>(__popcll(__ballot(l == 2)));
      Z += static_cast<uint32_t>(__popcll(__ballot(l == 1)));
    }
    const WnPlan p = wn_inbox(a, k, A, Z, lane == 0, lane == 0 ? &acc : &none);
    uint32_t ra = 0, rz = 0;
    for (uint64_t base = lo; base < hi; base += 64) {
      const bool valid = base + lane < hi;
      const uint8_t o = valid ? a.box_opts[base + lane] : WN_O_BAD;
      const uint32_t l = wn_live(o);
      const uint64_t ba = __ballot(l == 2), bz = __ballot(l == 1);
      uint16_t id;
      const uint8_t v = wn_verdict(p, o, ra + static_cast<uint32_t>(__popcll(ba & below)),
                                   rz + static_cast<uint32_t>(__popcll(bz & below)), &id);
      if (valid) {
        a.verdicts[base + lane] = v;
        a.pkt_ids[base + lane] = id;
      }
      ra += static_cast<uint32_t>(__popcll(ba));
      rz += static_cast<uint32_t>(__popcll(bz));
    }
  }
  wn_report(a, acc);
}

// update_table: the record after the batch of every inbox that is neither NO_SESSION nor PASS goes
// back to the table.  A kernel of its own: an inbox that spans tiles has its record at entry read
// by every one of them, so no tile may replace it.
__global__ __launch_bounds__(WN_BLOCK) void window_writeback_kernel(WnArgs a) {
  uint64_t m, total;
  if (!wn_counts(a, &m, &total)) return;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * WN_BLOCK + threadIdx.x; k < m;
       k += static_cast<uint64_t>(gridDim.x) * WN_BLOCK) {
    const uint32_t sub = a.inbox_subs[k];
    if (sub >= a.sub_limit) continue;
    const WnRec rec = wn_load_rec(a.out_sessions + k);
    if ((rec.flags & WN_PRESENT) && !(rec.flags & WN_PASSF)) wn_store_rec(a.sessions + sub, rec);
  }
}

__global__ void window_finish_kernel(WnArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = wn_counts(a, &m, &total);
  s[WN_S_BOXES] = m;
  if (!go) {
    s[WN_S_FLAGS] = WN_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= WN_MAX_TOTAL) s[WN_S_TOTAL] = a.inbox_offsets[m];
  } else {
    s[WN_S_TOTAL] = total;
    s[WN_S_FLAGS] = a.ctr[WN_S_FLAGS];
    for (uint32_t k = WN_S_SENDS; k < WN_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < WN_S_WORDS; ++k) a.summary[k] = s[k];
}

}  // namespace

// Enqueues the passes of one call.
int wn_launch(const WnArgs& a, int path, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  // below its maximum the key caps every grid; at it (the default) the wave kernel keeps its own cap
  const bool capped = a.max_blocks && a.max_blocks < WN_MAX_BLOCKS;
  const uint32_t cap = capped ? a.max_blocks : WN_MAX_BLOCKS, wave_cap = capped ? a.max_blocks : WN_WAVE_BLOCKS;
  if (path == 0) {
    const uint64_t tiles = wn_tiles(a.cap_in) ? wn_tiles(a.cap_in) : 1;
    const uint32_t blocks = static_cast<uint32_t>(tiles < cap ? tiles : cap);
    window_heads_kernel<<<dim3(blocks), dim3(WN_BLOCK), 0, s>>>(a);
    window_scan_kernel<<<dim3(1), dim3(WN_SCAN_BLOCK), 0, s>>>(a);
    window_verdict_kernel<<<dim3(blocks), dim3(WN_BLOCK), 0, s>>>(a);
  } else {
    const uint64_t rows = (a.cap_boxes + WN_WAVES - 1) / WN_WAVES;
    window_zero_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
    if (rows) window_wave_kernel<<<dim3(static_cast<uint32_t>(rows < wave_cap ? rows : wave_cap)), dim3(WN_BLOCK), 0, s>>>(a);
  }
  if (a.update_table && a.cap_boxes) {
    const uint64_t rows = (a.cap_boxes + WN_BLOCK - 1) / WN_BLOCK;
    window_writeback_kernel<<<dim3(static_cast<uint32_t>(rows < cap ? rows : cap)), dim3(WN_BLOCK), 0, s>>>(a);
  }
  window_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
