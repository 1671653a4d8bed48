// Kernels of the retry stage (include/emqx_retry.h).
//
// Every pass over the rows has the shape of the ack stage's rows kernels: W / 2 lanes a row, one
// 16-byte load of two slots and one of their two stamps per lane, 256-thread blocks, 512 / W rows
// a block and trip (a "tile"), the grid capped by max_blocks and the blocks striding beyond it.
// W / 2 divides 64, so a row's lanes never straddle a wave and the row's sums, maxima and key
// broadcasts are shuffles.
// Stamp (behind every record and run call):
//   retry_init_kernel   zeroes the counters;
//   retry_stamp_kernel  load, rt_stamp_next per slot, a 16-byte store only where a stamp changed.
// Sweep (retry/1 or replay/1 of m sessions):
//   retry_count_kernel  rt_is_item per slot, the tile's item count into tile_tot;
//   retry_scan_kernel   one block: tile_tot becomes its exclusive scan; the total into
//                       out_offsets[m]; whether it exceeds cap_out; zeroes the counters;
//   retry_emit_kernel   rt_eval per slot again; the row's counts by shuffles, the rows of a tile
//                       scanned in the block, out_offsets[k]; an item's rank is the number of the
//                       row's keys below its own, found by broadcasting every lane's two keys
//                       round the row's lanes (W compares per item, no LDS, no sort); a wave in
//                       which no row has an item skips the ranking.  Items, the rewritten slots and
//                       stamps (only where they changed) and sessions[].inflight are stored unless
//                       the call is full; counts, status and timer always.
//   retry_finish_kernel the summary.
// A row is read and written by its own lanes only, and the count and emit pass evaluate the same
// predicate on the same bytes: nothing rewrites a row between them.  The atomics are sums and an
// OR: every output byte is a function of the input alone.
//
// Every index is bounded before use: a session index < m <= cap_boxes, a subscriber id < sub_limit,
// a ref < ref_limit, an item position < cap_out, a tile < rt_tiles(cap_boxes, w).  The count is read
// on the device; the host sizes the grids by cap_boxes.
#include <hip/hip_runtime.h>

#include "retry.h"

namespace emqx {

namespace {

constexpr uint32_t RT_WAVES = AK_BLOCK / 64;

// m when this call may use it; false: the call is refused.
__device__ inline bool rt_count(const uint64_t* n_boxes, uint64_t m_arg, uint64_t cap_boxes, const uint32_t* subs, uint64_t sub_limit,
                                uint64_t* m) {
  *m = n_boxes ? *n_boxes : m_arg;
  return *m <= cap_boxes && *m <= AK_MAX_TOTAL && (subs || *m <= sub_limit);
}

// ---- stamp -------------------------------------------------------------------------------------

__global__ void retry_init_kernel(unsigned long long* ctr) {
  if (blockIdx.x == 0 && threadIdx.x < RT_C_WORDS) ctr[threadIdx.x] = 0;
}

__global__ __launch_bounds__(AK_BLOCK) void retry_stamp_kernel(RtStampArgs a) {
  uint64_t m;
  if (!rt_count(a.n_boxes, a.m, a.cap_boxes, a.subs, a.sub_limit, &m)) return;
  const uint32_t lanes = a.w / 2, per_block = AK_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  uint64_t acc[4] = {0, 0, 0, 0};  // rows, (the row count m: the finish kernel), stamped, cleared
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    if (k >= m) continue;  // (no shuffle and no barrier in this loop)
    const uint64_t sub = a.subs ? a.subs[k] : k;
    if (sub >= a.sub_limit) {
      if (j == 0) flags |= RT_F_BAD_SUB;
      continue;
    }
    const uint4 s = reinterpret_cast<const uint4*>(a.slots)[sub * lanes + j];
    ulonglong2* at = reinterpret_cast<ulonglong2*>(a.stamps) + sub * lanes + j;
    const ulonglong2 t = *at;
    const uint64_t n0 = rt_stamp_next(s.x, t.x, a.now_ms), n1 = rt_stamp_next(s.z, t.y, a.now_ms);
    if (n0 != t.x) acc[n0 ? 2 : 3] += 1;
    if (n1 != t.y) acc[n1 ? 2 : 3] += 1;
    if (n0 != t.x || n1 != t.y) *at = make_ulonglong2(n0, n1);
    if (j == 0) acc[0] += 1;
  }
  block_report<4>(a.ctr, RT_S_ROWS, acc, flags, RT_S_FLAGS);
}

__global__ void retry_stamp_finish_kernel(RtStampArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m;
  uint64_t s[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = rt_count(a.n_boxes, a.m, a.cap_boxes, a.subs, a.sub_limit, &m);
  if (!go) {
    s[RT_S_FLAGS] = RT_F_INPUT_REFUSED;
  } else {
    s[RT_S_FLAGS] = a.ctr[RT_S_FLAGS];
    s[RT_S_ROWS] = a.ctr[RT_S_ROWS];
    s[RT_T_STAMPED] = a.ctr[RT_T_STAMPED];
    s[RT_T_CLEARED] = a.ctr[RT_T_CLEARED];
  }
  s[RT_S_BOXES] = m;
  for (uint32_t k = 0; k < RT_S_WORDS; ++k) a.summary[k] = s[k];
}

// ---- sweep -------------------------------------------------------------------------------------

__device__ inline bool rt_sweep_count(const RtSweepArgs& a, uint64_t* m) {
  return rt_count(a.n_boxes, a.m, a.cap_boxes, a.subs, a.sub_limit, m);
}

// Session k: its subscriber id, its interval and 0, or the status that keeps it out of the sweep.
__device__ inline uint8_t rt_session_of(const RtSweepArgs& a, uint64_t k, uint64_t* sub, uint32_t* interval) {
  *sub = a.subs ? a.subs[k] : k;
  *interval = 0;
  const bool ok = *sub < a.sub_limit;
  const uint8_t dead = ak_session(ok, ok ? a.sessions[*sub * AK_REC_WORDS + AK_REC_FLAGS] : 0u);
  if (!dead && a.mode != RT_MODE_REPLAY) *interval = rt_interval(a.intervals, *sub, a.interval_ms);
  return dead;
}

// The two stamps of lane j of row `sub` (0 in replay mode, which reads none).
__device__ inline ulonglong2 rt_load_stamps(const RtSweepArgs& a, uint64_t sub, uint32_t lanes, uint32_t j) {
  if (a.mode == RT_MODE_REPLAY || !a.stamps) return make_ulonglong2(0, 0);
  return reinterpret_cast<const ulonglong2*>(a.stamps)[sub * lanes + j];
}

// a.w / 2 lanes a row.  The loop is uniform over the block: the barriers see every thread.
__global__ __launch_bounds__(AK_BLOCK) void retry_count_kernel(RtSweepArgs a) {
  __shared__ uint32_t wsum[RT_WAVES];
  uint64_t m;
  if (!rt_sweep_count(a, &m)) return;
  const uint32_t lanes = a.w / 2, per_block = AK_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    uint32_t c = 0;
    if (k < m) {
      uint64_t sub;
      uint32_t interval;
      if (!rt_session_of(a, k, &sub, &interval)) {
        const uint4 s = reinterpret_cast<const uint4*>(a.slots)[sub * lanes + j];
        const ulonglong2 t = rt_load_stamps(a, sub, lanes, j);
        c = (rt_is_item(a.mode, s.x, t.x, a.now_ms, interval) ? 1u : 0u) + (rt_is_item(a.mode, s.z, t.y, a.now_ms, interval) ? 1u : 0u);
      }
    }
    c = wave_sum(c);
    __syncthreads();  // the readers of the trip before are done
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
      for (uint32_t w = 0; w < RT_WAVES; ++w) all += wsum[w];
      a.tile_tot[base / per_block] = all;  // (base < m <= cap_boxes: a tile of the scratch)
    }
  }
}

// One block: tile_tot becomes its exclusive scan, scan_chunk tiles a carry step
// (stage_common.h's block_scan_in_place).
__global__ __launch_bounds__(AK_SCAN_BLOCK) void retry_scan_kernel(RtSweepArgs a) {
  __shared__ uint64_t wsum[AK_SCAN_BLOCK / 64];
  if (threadIdx.x < RT_C_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m;
  if (!rt_sweep_count(a, &m)) return;
  const uint64_t total = block_scan_in_place<AK_SCAN_BLOCK>(a.tile_tot, a.tile_tot, rt_tiles(m, a.w), wsum,
                                                            scan_chunk_of<AK_SCAN_BLOCK>(a.scan_chunk));
  __syncthreads();  // the zeroing above
  if (threadIdx.x == 0) {
    a.ctr[RT_C_TOTAL] = total;
    a.ctr[RT_C_FULL] = total > a.cap_out ? 1ull : 0ull;
    a.out_offsets[m] = total;
  }
}

// a.w / 2 lanes a session.  The loop is uniform over the block: the shuffles and the barriers see
// every lane.
__global__ __launch_bounds__(AK_BLOCK) void retry_emit_kernel(RtSweepArgs a) {
  __shared__ uint32_t wsum[RT_WAVES];
  uint64_t m;
  if (!rt_sweep_count(a, &m)) return;
  const bool full = a.ctr[RT_C_FULL] != 0;
  const bool replay = a.mode == RT_MODE_REPLAY;
  const uint32_t lanes = a.w / 2, per_block = AK_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  const uint32_t head = (threadIdx.x & 63u) - j;  // the row's first lane in its wave
  uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};        // OK sessions, -, -, publishes, pubrels, expired, unstamped
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    uint64_t sub = 0;
    uint32_t interval = 0;
    const uint8_t dead = valid ? rt_session_of(a, k, &sub, &interval) : AK_NO_SESSION;
    uint4 s = make_uint4(0, 0, 0, 0);
    ulonglong2 t = make_ulonglong2(0, 0);
    RtSlot e[2] = {{0, 0, RT_NO_KEY, 0, false, false, false}, {0, 0, RT_NO_KEY, 0, false, false, false}};
    if (!dead) {
      s = reinterpret_cast<const uint4*>(a.slots)[sub * lanes + j];
      t = rt_load_stamps(a, sub, lanes, j);
      e[0] = rt_eval(a.mode, s.x, s.y, t.x, a.now_ms, interval, a.deadlines, a.ref_limit);
      e[1] = rt_eval(a.mode, s.z, s.w, t.y, a.now_ms, interval, a.deadlines, a.ref_limit);
    }
    // of the row: items, publishes << 8, pubrels << 16, expired << 24 (each at most 64);
    // entries, unstamped << 8, bad refs << 16; the largest age of a young slot
    uint32_t packed = 0, packed2 = 0, young_age = e[0].young_age > e[1].young_age ? e[0].young_age : e[1].young_age;
#pragma unroll
    for (uint32_t i = 0; i < 2; ++i) {
      if (e[i].kind) packed += 1u + (1u << (8 * e[i].kind));
      packed2 += (e[i].nonempty ? 1u : 0u) + (e[i].unstamped ? 1u << 8 : 0u) + (e[i].bad_ref ? 1u << 16 : 0u);
    }
    for (uint32_t d = 1; d < lanes; d <<= 1) {
      packed += __shfl_xor(packed, d, 64);
      packed2 += __shfl_xor(packed2, d, 64);
      const uint32_t y = __shfl_xor(young_age, d, 64);
      young_age = y > young_age ? y : young_age;
    }
    const uint32_t items = packed & 0xFFu;
    uint32_t tile_items;  // (not used: the scan kernel has the tile's base)
    const uint32_t pre = block_excl_scan<AK_BLOCK>(j == 0 ? items : 0u, wsum, &tile_items);
    const uint64_t off = a.tile_tot[base / per_block] + __shfl(pre, head, 64);
    // the rank of an item among its row's items: the keys below its own, ties by slot index
    uint32_t rank[2] = {0, 0};
    if (__ballot(items != 0) != 0) {
      for (uint32_t l = 0; l < lanes; ++l) {
        const uint64_t o0 = __shfl(static_cast<unsigned long long>(e[0].key), head + l, 64);
        const uint64_t o1 = __shfl(static_cast<unsigned long long>(e[1].key), head + l, 64);
#pragma unroll
        for (uint32_t i = 0; i < 2; ++i) {
          const uint32_t mine = 2 * j + i;
          rank[i] += (o0 < e[i].key || (o0 == e[i].key && 2 * l < mine)) ? 1u : 0u;
          rank[i] += (o1 < e[i].key || (o1 == e[i].key && 2 * l + 1 < mine)) ? 1u : 0u;
        }
      }
    }
    if (!dead && !full) {
      const uint32_t w0[2] = {s.x, s.z}, w1[2] = {s.y, s.w};
#pragma unroll
      for (uint32_t i = 0; i < 2; ++i) {
        const uint64_t pos = off + rank[i];
        if (e[i].kind && pos < a.cap_out) a.out_items[pos] = make_uint2(rt_item_word0(w0[i], e[i].kind), w1[i]);
      }
      if (!replay) {
        if (e[0].kind == RT_EXPIRED || e[1].kind == RT_EXPIRED) {
          const bool x0 = e[0].kind == RT_EXPIRED, x1 = e[1].kind == RT_EXPIRED;
          reinterpret_cast<uint4*>(a.slots)[sub * lanes + j] = make_uint4(x0 ? 0u : s.x, x0 ? 0u : s.y, x1 ? 0u : s.z, x1 ? 0u : s.w);
        }
        if (e[0].stamp_after != t.x || e[1].stamp_after != t.y)
          reinterpret_cast<ulonglong2*>(a.stamps)[sub * lanes + j] = make_ulonglong2(e[0].stamp_after, e[1].stamp_after);
      }
    }
    if (valid && j == 0) {
      uint4 counts = make_uint4(0, 0, 0, 0);
      uint32_t timer = RT_NO_TIMER;
      if (!dead) {
        const uint32_t expired = packed >> 24;
        uint32_t* rec = a.sessions + sub * AK_REC_WORDS;
        const uint32_t after = ak_inflight_after(rec[AK_REC_INFLIGHT], expired);
        counts = make_uint4((packed >> 8) & 0xFFu, (packed >> 16) & 0xFFu, expired, after);
        timer = rt_timer(a.mode, (packed2 & 0xFFu) != 0, interval, young_age);
        if (a.update_table && !full && expired) rec[AK_REC_INFLIGHT] = after;
        acc[0] += 1;
        acc[3] += counts.x;
        acc[4] += counts.y;
        acc[5] += expired;
        acc[6] += (packed2 >> 8) & 0xFFu;
        if (packed2 & 0xFF00u) flags |= RT_F_UNSTAMPED;
        if (packed2 >> 16) flags |= RT_F_BAD_REF;
      }
      a.out_offsets[k] = off;
      a.out_status[k] = dead ? dead : AK_OK;
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = counts;
      a.out_timers[k] = timer;
      if (sub >= a.sub_limit) flags |= RT_F_BAD_SUB;
    }
  }
  block_report<7>(a.ctr, RT_S_ROWS, acc, flags, RT_S_FLAGS);
}

__global__ void retry_sweep_finish_kernel(RtSweepArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m;
  uint64_t s[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = rt_sweep_count(a, &m);
  if (!go) {
    s[RT_S_FLAGS] = RT_F_INPUT_REFUSED;
  } else {
    for (uint32_t k = 0; k < RT_S_WORDS; ++k) s[k] = a.ctr[k];
    s[RT_W_ITEMS] = a.ctr[RT_C_TOTAL];
    if (a.ctr[RT_C_FULL]) s[RT_S_FLAGS] |= RT_F_OUTPUT_FULL;
  }
  s[RT_S_BOXES] = m;
  for (uint32_t k = 0; k < RT_S_WORDS; ++k) a.summary[k] = s[k];
}

// The grid over `units` groups of rows; the blocks stride beyond the cap.
uint32_t rt_grid(uint64_t units, uint32_t max_blocks) {
  const uint32_t cap = max_blocks && max_blocks < AK_MAX_BLOCKS ? max_blocks : AK_MAX_BLOCKS;
  if (units == 0) units = 1;
  return static_cast<uint32_t>(units < cap ? units : cap);
}

}  // namespace

// Enqueues the passes of one stamp call.
int rt_launch_stamp(const RtStampArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t rows = rt_grid(rt_tiles(a.cap_boxes, a.w), a.max_blocks);
  retry_init_kernel<<<dim3(1), dim3(64), 0, s>>>(a.ctr);
  retry_stamp_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  retry_stamp_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

// Enqueues the passes of one sweep call.
int rt_launch_sweep(const RtSweepArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t rows = rt_grid(rt_tiles(a.cap_boxes, a.w), a.max_blocks);
  retry_count_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  retry_scan_kernel<<<dim3(1), dim3(AK_SCAN_BLOCK), 0, s>>>(a);
  retry_emit_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  retry_sweep_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
