// Kernels of the mqueue stage (include/emqx_mqueue.h).
//
// Put (behind the window stage): the r-th EMQX_W_QUEUED delivery of an inbox goes to logical index
// L - ev + r of its session's ring, the j-th EMQX_W_EVICTS delivery reports the old entry j.  One
// global exclusive prefix count of the three indicators (QUEUED, EVICTS, QUEUED_DROPPED) over all
// deliveries gives every delivery its ranks (its prefix minus the prefix at its inbox's head), as
// ack_rec_* ranks its sends:
//   mq_put_heads_kernel  per tile: the block scan of the indicators (three 16-bit fields of one
//                        word, a tile holds 1024 deliveries), the tile's totals, the prefix at every
//                        inbox head that lies in the tile;
//   mq_put_scan_kernel   one block: the exclusive scans of the tile totals; zeroes the counters;
//   mq_put_evict_kernel  per tile: the scan again; an evicting delivery finds its inbox by a binary
//                        search narrowed to the tile's inboxes and copies the old entry of its rank
//                        into out_evicted; every other position gets {NO_REF, 0};
//   mq_put_rows_kernel   one thread an inbox: the three counts, the plan (mq_put_plan) into the
//                        scratch, out_unstored, the new header, the counters;
//   mq_put_store_kernel  per tile: the scan again; a QUEUED delivery of rank r below the plan's room
//                        stores its entry at (start + r) % Q with one 8-byte store.
// THE HAZARD: when a row is full (L = Q) the survivors land exactly on the positions of the evicted
// entries, and the plan replaces the header the evict pass reads.  So every read for out_evicted
// (ring and heads) completes in mq_put_evict_kernel, a launch before the one that rewrites the
// headers and two before the one that stores into rings; the store pass reads the plan in the
// scratch, never a header or a ring.
//
// Take (dequeue/1 of m sessions): G = min(Q / 2, 8) lanes a session (queues are short where the
// load is: a wider group idles most of its lanes), one 16-byte load of two entries a lane and trip,
// 256 / G sessions a block and trip (a "tile"), the grid capped by max_blocks and the blocks
// striding beyond it.  G divides 64, so a session's lanes never straddle
// a wave and its prefix counts are shuffles.  A lane's pair is physically aligned: trip c, lane j
// loads pair (head / 2 + c * G + j) % (Q / 2), whose entries have the logical indices 2p - (head &
// 1) and one more (p = c * G + j); an index outside [0, len) is predicated off.  The trips of a
// session carry the prefix count; the trip loop is uniform over the wave (a ballot), so the shuffles
// see every lane, runs only while some session of the wave has live entries and budget left, and
// holds no barrier.  The loop over the tiles is uniform over the block: the barriers see every
// thread.
//   mq_take_count_kernel  the consumed entries of every session into out_offsets[k], the tile's sum
//                         into tile_tot;
//   mq_take_scan_kernel   one block: tile_tot becomes its exclusive scan; the total into
//                         out_offsets[m]; whether it exceeds cap_out; zeroes the counters;
//   mq_take_emit_kernel   the sessions of a tile scanned in the block, out_offsets[k]; the fold again,
//                         a consumed entry of logical index i is item out_offsets[k] + i; the four
//                         counts and the status always; items, the header and the record unless the
//                         call is full;
//   mq_take_finish_kernel the summary.
// A ring row is only read here; a header and a record are read and written by their session's own
// lanes, and the count and the emit pass evaluate the same predicate on the same bytes: nothing
// rewrites a header or a record between them.  The atomics are sums and an OR: every output byte is
// a function of the input alone.  No thread walks an inbox or a queue.
//
// Every index is bounded before use: a position < offsets[m] <= cap_in, an inbox or session index
// < m <= cap_boxes, a subscriber id < sub_limit, a ring index masked by Q - 1 (a pair by Q / 2 - 1),
// a ref < ref_limit, an item position < cap_out, a tile < max(1, ceil(cap_in / MQ_TILE)) or
// < mq_take_tiles(cap_boxes, q).  The counts are read on the device; the host sizes the grids by
// cap_in and cap_boxes.
#include <hip/hip_runtime.h>

#include "mqueue.h"

namespace emqx {

namespace {

constexpr uint32_t MQ_WAVES = AK_BLOCK / 64;
constexpr uint64_t MQ_NONE = 0xFFFFFFFFull;

// ---- put ---------------------------------------------------------------------------------------

// m and offsets[m] when this call may use them; false: the call is refused.
__device__ inline bool mq_put_counts(const MqPutArgs& a, uint64_t* m, uint64_t* total) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  *total = 0;
  if (*m > a.cap_boxes || *m > AK_MAX_TOTAL) return false;
  *total = a.inbox_offsets[*m];
  return *total <= a.cap_in && *total <= AK_MAX_TOTAL;
}

__device__ inline uint64_t mq_tiles_eff(uint64_t total) {  // a call without positions still has its inboxes
  const uint64_t t = mq_tiles(total);
  return t ? t : 1;
}

// The inboxes a tile's positions can belong to, as bounds of csr_upper: thread 0 and 1 search the
// whole array once a tile.  ext[0] <= ext[1] <= m + 1.
__device__ inline void mq_tile_extent(const uint64_t* offsets, uint64_t m, uint64_t ts, uint64_t total, uint64_t* ext) {
  __syncthreads();  // the readers of the tile before are done
  if (threadIdx.x == 0) ext[0] = csr_upper(offsets, 0, m + 1, ts);
  if (threadIdx.x == 1) {
    const uint64_t end = total - ts < MQ_TILE ? total : ts + MQ_TILE;  // (ts < total)
    ext[1] = csr_upper(offsets, 0, m + 1, end - 1);
  }
  __syncthreads();
}

// The inbox of position d: the last k with offsets[k] <= d, MQ_NONE when the offsets name none.
// k_at: the answer for the position before, tried first.
__device__ inline uint64_t mq_box_of(const uint64_t* offsets, uint64_t m, const uint64_t* ext, uint64_t d, uint64_t k_at) {
  if (k_at < m && offsets[k_at] <= d && d < offsets[k_at + 1]) return k_at;
  const uint64_t lo = ext[0], hi = ext[1] < lo ? lo : ext[1];
  const uint64_t u = csr_upper(offsets, lo, hi, d);
  return (u >= 1 && u <= m) ? u - 1 : MQ_NONE;
}

// The three indicators of positions p0 .. p0 + MQ_ROWS as bits: QUEUED, EVICTS << 8, QUEUED_DROPPED << 16.
__device__ inline uint32_t mq_load_bits(const uint8_t* verdicts, uint64_t p0, uint64_t total) {
  uint32_t bits = 0;
  uint32_t w = 0;
  if (p0 + MQ_ROWS <= total && ((reinterpret_cast<uintptr_t>(verdicts) + p0) & 3u) == 0) {
    w = *reinterpret_cast<const uint32_t*>(verdicts + p0);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < MQ_ROWS; ++j)
      if (p0 + j < total) w |= static_cast<uint32_t>(verdicts[p0 + j]) << (8 * j);  // (0: none of the three)
  }
#pragma unroll
  for (uint32_t j = 0; j < MQ_ROWS; ++j) {
    const uint8_t v = static_cast<uint8_t>(w >> (8 * j));
    bits |= (mq_is_queued(v) ? 1u : 0u) << j | (mq_evicts(v) ? 0x100u : 0u) << j | (mq_is_qdropped(v) ? 0x10000u : 0u) << j;
  }
  return bits;
}

// The counts of the bits as three 16-bit fields of one word (a tile's sums are at most 1024 each).
__device__ inline uint64_t mq_pack_counts(uint32_t bits) {
  return static_cast<uint64_t>(__popc(bits & 0xFFu)) | static_cast<uint64_t>(__popc(bits & 0xFF00u)) << 16 |
         static_cast<uint64_t>(__popc(bits & 0xFF0000u)) << 32;
}

// The global prefixes at the head of inbox k (k <= m), modulo 2^32 each: QUEUED, EVICTS, QUEUED_DROPPED.
struct MqBase {
  uint32_t s, x, qd;
};
__device__ inline MqBase mq_base(const MqPutArgs& a, uint64_t k, uint64_t total, uint64_t tiles) {
  const uint64_t off = a.inbox_offsets[k];
  const uint64_t p = off < total ? off : total;
  uint64_t t = p / MQ_TILE;
  if (t >= tiles) t = tiles - 1;
  const uint64_t sx = a.tile_sx[t], hp = a.head_pre[k];
  return MqBase{static_cast<uint32_t>(sx) + static_cast<uint32_t>(hp & 0xFFFFu),
                static_cast<uint32_t>(sx >> 32) + static_cast<uint32_t>((hp >> 16) & 0xFFFFu),
                a.tile_qd[t] + static_cast<uint32_t>((hp >> 32) & 0xFFFFu)};
}

__global__ __launch_bounds__(AK_BLOCK) void mq_put_heads_kernel(MqPutArgs a) {
  __shared__ uint64_t pre[MQ_TILE + 1];  // packed exclusive prefix at every position of the tile, and at its end
  __shared__ uint64_t wsum[MQ_WAVES];
  uint64_t m, total;
  if (!mq_put_counts(a, &m, &total)) return;
  const uint64_t tiles = mq_tiles_eff(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * MQ_TILE;
    const bool last = tile + 1 == tiles;
    const uint32_t bits = mq_load_bits(a.verdicts, ts + static_cast<uint64_t>(threadIdx.x) * MQ_ROWS, total);
    uint64_t all;
    uint64_t run = block_excl_scan<AK_BLOCK>(mq_pack_counts(bits), wsum, &all);
#pragma unroll
    for (uint32_t j = 0; j < MQ_ROWS; ++j) {
      pre[threadIdx.x * MQ_ROWS + j] = run;
      run += static_cast<uint64_t>((bits >> j) & 1u) | static_cast<uint64_t>((bits >> (8 + j)) & 1u) << 16 |
             static_cast<uint64_t>((bits >> (16 + j)) & 1u) << 32;
    }
    if (threadIdx.x == 0) {
      pre[MQ_TILE] = all;
      a.tile_sx[tile] = (all & 0xFFFFu) | ((all >> 16) & 0xFFFFu) << 32;
      a.tile_qd[tile] = static_cast<uint32_t>((all >> 32) & 0xFFFFu);
    }
    __syncthreads();
    // the inboxes whose head lies in [ts, ts + MQ_TILE); the last tile also takes the heads at its
    // end (inboxes without deliveries behind the last delivery, and inbox_offsets[m] itself)
    const uint64_t k_lo = csr_lower(a.inbox_offsets, 0, m + 1, ts);
    const uint64_t k_hi = last ? m + 1 : csr_lower(a.inbox_offsets, 0, m + 1, ts + MQ_TILE);
    for (uint64_t k = k_lo + threadIdx.x; k < k_hi; k += AK_BLOCK) {
      const uint64_t off = a.inbox_offsets[k];
      const uint64_t p = off < total ? off : total;
      if (p >= ts && p - ts <= (last ? MQ_TILE : MQ_TILE - 1)) a.head_pre[k] = pre[p - ts];
    }
    __syncthreads();  // the next tile writes pre
  }
}

// One block: tile_sx and tile_qd become their exclusive scans, scan_chunk tiles a carry step
// (stage_common.h's block_scan_in_place).
__global__ __launch_bounds__(AK_SCAN_BLOCK) void mq_put_scan_kernel(MqPutArgs a) {
  __shared__ uint64_t wsum[AK_SCAN_BLOCK / 64];
  __shared__ uint32_t wsum_qd[AK_SCAN_BLOCK / 64];
  if (threadIdx.x < MQ_C_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m, total;
  if (!mq_put_counts(a, &m, &total)) return;
  const uint32_t chunk = scan_chunk_of<AK_SCAN_BLOCK>(a.scan_chunk);
  (void)block_scan_in_place<AK_SCAN_BLOCK>(a.tile_sx, a.tile_sx, mq_tiles_eff(total), wsum, chunk);
  (void)block_scan_in_place<AK_SCAN_BLOCK>(a.tile_qd, a.tile_qd, mq_tiles_eff(total), wsum_qd, chunk);
}

__global__ __launch_bounds__(AK_BLOCK) void mq_put_evict_kernel(MqPutArgs a) {
  __shared__ uint32_t wsum[MQ_WAVES];
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!mq_put_counts(a, &m, &total)) return;
  const uint64_t tiles = mq_tiles(total);
  const uint32_t qm = a.q - 1;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * MQ_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * MQ_ROWS;
    const uint32_t bits = mq_load_bits(a.verdicts, p0, total) >> 8;  // EVICTS in the low byte
    uint32_t all;
    uint32_t run = static_cast<uint32_t>(a.tile_sx[tile] >> 32) + block_excl_scan<AK_BLOCK>(static_cast<uint32_t>(__popc(bits & 0xFFu)), wsum, &all);
    mq_tile_extent(a.inbox_offsets, m, ts, total, ext);
    uint64_t k = MQ_NONE;
#pragma unroll
    for (uint32_t j = 0; j < MQ_ROWS; ++j) {
      const uint64_t d = p0 + j;
      if (d >= total) continue;
      uint2 old = make_uint2(MQ_NO_REF, 0u);
      if ((bits >> j) & 1u) {
        const uint32_t g = run++;
        k = mq_box_of(a.inbox_offsets, m, ext, d, k);
        if (k != MQ_NONE) {
          const uint32_t rank = g - mq_base(a, k, total, tiles).x;
          const uint32_t sub = a.inbox_subs[k];
          if (sub < a.sub_limit) {
            const uint2 hd = a.heads[sub];
            uint32_t h, L;
            bool bad;
            mq_header(hd.x, hd.y, a.q, &h, &L, &bad);
            if (rank < L) old = a.ring[static_cast<uint64_t>(sub) * a.q + ((h + rank) & qm)];
          }
        }
      }
      a.out_evicted[d] = old;
    }
  }
}

// One thread an inbox.
__global__ __launch_bounds__(AK_BLOCK) void mq_put_rows_kernel(MqPutArgs a) {
  uint64_t m, total;
  if (!mq_put_counts(a, &m, &total)) return;
  const uint64_t tiles = mq_tiles_eff(total);
  uint64_t acc[5] = {0, 0, 0, 0, 0};  // stored, evicted, unstored, full rows, len mismatches
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * AK_BLOCK; base < m; base += static_cast<uint64_t>(gridDim.x) * AK_BLOCK) {
    const uint64_t k = base + threadIdx.x;
    if (k >= m) continue;  // (no shuffle and no barrier in this loop)
    const uint32_t sub = a.inbox_subs[k];
    const bool ok = sub < a.sub_limit;
    const MqBase b0 = mq_base(a, k, total, tiles), b1 = mq_base(a, k + 1, total, tiles);
    uint32_t h = 0, L = 0;
    bool bad = false;
    if (ok) {
      const uint2 hd = a.heads[sub];
      mq_header(hd.x, hd.y, a.q, &h, &L, &bad);
    }
    const MqPlan p = mq_put_plan(ok, h, L, a.q, b1.s - b0.s, b1.x - b0.x, b1.qd - b0.qd);
    a.plans[k] = make_uint2(p.start, p.room);
    a.out_unstored[k] = p.unstored;
    acc[0] += p.stored;
    acc[1] += p.ev;
    acc[2] += p.unstored;
    if (ok) {
      a.heads[sub] = make_uint2(p.head, p.len);
      if (p.unstored) {
        acc[3] += 1;
        flags |= MQ_F_ROW_FULL;
      }
      if (bad) flags |= MQ_F_BAD_RING;
      if (a.sessions && a.sessions[static_cast<uint64_t>(sub) * AK_REC_WORDS + MQ_REC_MQ_LEN] != p.len) {
        acc[4] += 1;
        flags |= MQ_F_LEN_MISMATCH;
      }
    } else {
      flags |= MQ_F_BAD_SUB;
    }
  }
  block_report<5>(a.ctr, MQ_P_STORED, acc, flags, MQ_S_FLAGS);
}

__global__ __launch_bounds__(AK_BLOCK) void mq_put_store_kernel(MqPutArgs a) {
  __shared__ uint32_t wsum[MQ_WAVES];
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!mq_put_counts(a, &m, &total)) return;
  const uint64_t tiles = mq_tiles(total);
  const uint32_t qm = a.q - 1;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * MQ_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * MQ_ROWS;
    const uint32_t bits = mq_load_bits(a.verdicts, p0, total) & 0xFFu;  // QUEUED
    uint32_t all;
    uint32_t run = static_cast<uint32_t>(a.tile_sx[tile]) + block_excl_scan<AK_BLOCK>(static_cast<uint32_t>(__popc(bits)), wsum, &all);
    mq_tile_extent(a.inbox_offsets, m, ts, total, ext);
    uint64_t k = MQ_NONE;
#pragma unroll
    for (uint32_t j = 0; j < MQ_ROWS; ++j) {
      if (!((bits >> j) & 1u)) continue;  // (a set bit: p0 + j < total)
      const uint64_t d = p0 + j;
      const uint32_t g = run++;
      k = mq_box_of(a.inbox_offsets, m, ext, d, k);
      if (k == MQ_NONE) continue;
      const uint32_t r = g - mq_base(a, k, total, tiles).s;
      const uint2 plan = a.plans[k];  // (room 0 for a subscriber id that is not below sub_limit)
      if (r >= plan.y) continue;
      const uint32_t sub = a.inbox_subs[k];
      if (sub >= a.sub_limit) continue;
      a.ring[static_cast<uint64_t>(sub) * a.q + ((plan.x + r) & qm)] =
          make_uint2(a.refs ? a.refs[d] : static_cast<uint32_t>(d), mq_word1(a.box_opts[d]));
    }
  }
}

__global__ void mq_put_finish_kernel(MqPutArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = mq_put_counts(a, &m, &total);
  s[MQ_S_BOXES] = m;
  if (!go) {
    s[MQ_S_FLAGS] = MQ_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= AK_MAX_TOTAL) s[MQ_S_TOTAL] = a.inbox_offsets[m];
  } else {
    s[MQ_S_TOTAL] = total;
    s[MQ_S_FLAGS] = a.ctr[MQ_S_FLAGS];
    for (uint32_t k = MQ_P_STORED; k < MQ_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < MQ_S_WORDS; ++k) a.summary[k] = s[k];
}

// ---- take --------------------------------------------------------------------------------------

// m when this call may use it; false: the call is refused.
__device__ inline bool mq_take_count(const MqTakeArgs& a, uint64_t* m) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  return *m <= a.cap_boxes && *m <= AK_MAX_TOTAL && (a.subs || *m <= a.sub_limit);
}

// What the fold needs of session k, in every lane of its group.
struct MqRow {
  uint64_t sub;
  uint32_t h, L, n, next_pkt, inflight, mq_len;
  uint8_t dead;  // 0, or the status that keeps the session out of the call
  bool bad_ring;
};
__device__ inline MqRow mq_row_of(const MqTakeArgs& a, uint64_t k, bool valid) {
  MqRow r{0, 0, 0, 0, 0, 0, 0, AK_NO_SESSION, false};
  if (!valid) return r;
  r.sub = a.subs ? a.subs[k] : k;
  const bool ok = r.sub < a.sub_limit;
  const uint32_t* rec = a.sessions + r.sub * AK_REC_WORDS;
  r.dead = ak_session(ok, ok ? rec[AK_REC_FLAGS] : 0u);
  if (r.dead) return r;
  const uint2 hd = a.heads[r.sub];
  mq_header(hd.x, hd.y, a.q, &r.h, &r.L, &r.bad_ring);
  r.inflight = rec[AK_REC_INFLIGHT];
  r.n = mq_budget(rec[AK_REC_INFLIGHT_MAX], r.inflight);
  r.mq_len = rec[MQ_REC_MQ_LEN];
  r.next_pkt = rec[MQ_REC_NEXT_PKT];
  return r;
}

// What a lane found in its pairs: consumed entries, and of those the sends with id, the sends
// QoS 0 and the expired (each at most 1024 in a row: 16-bit fields), and whether one had a bad ref.
struct MqFound {
  uint32_t items_sends, sends0_expired, bad_ref;
};

// The fold over the row of one session by the G lanes of its group; j the lane's place in the
// group, lane0 the group's first lane in its wave.  EMIT: the items go to position off + i.
// Uniform over the wave: every lane of the wave calls it, dead and invalid rows with L = 0.
template <bool EMIT>
__device__ inline MqFound mq_fold(const MqTakeArgs& a, const MqRow& r, uint32_t G, uint32_t j, uint32_t lane0, uint64_t off) {
  MqFound f{0, 0, 0};
  const uint32_t odd = r.h & 1u, pair0 = r.h >> 1, pm = a.q / 2 - 1;
  const uint32_t need = r.dead ? 0u : (r.L + odd + 1) / 2;  // pairs that hold the live entries
  const uint4* row = reinterpret_cast<const uint4*>(a.ring) + r.sub * (a.q / 2);
  uint32_t carry = 0;  // counting entries of the trips before
  for (uint32_t c = 0; __ballot(c * G < need && carry < r.n) != 0; ++c) {
    const uint32_t p = c * G + j;
    const bool active = p < need && carry < r.n;
    uint4 e = make_uint4(0, 0, 0, 0);
    if (active) e = row[(pair0 + p) & pm];
    const uint32_t i1 = 2 * p + 1 - odd;  // the logical index of the pair's second entry; the first is i1 - 1
    const bool v0 = active && i1 >= 1 && i1 - 1 < r.L, v1 = active && i1 < r.L;
    bool b0 = false, b1 = false;
    const bool x0 = v0 && mq_expired(e.x, a.now_ms, a.deadlines, a.ref_limit, &b0);
    const bool x1 = v1 && mq_expired(e.z, a.now_ms, a.deadlines, a.ref_limit, &b1);
    const uint32_t c0 = v0 && mq_counting(static_cast<uint8_t>(e.y), x0) ? 1u : 0u;
    const uint32_t c1 = v1 && mq_counting(static_cast<uint8_t>(e.w), x1) ? 1u : 0u;
    uint32_t incl = c0 + c1;
    for (uint32_t d = 1; d < G; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d, 64);
      if (j >= d) incl += y;
    }
    const uint32_t trip = __shfl(incl, lane0 + G - 1, 64);
    const uint32_t before0 = carry + incl - c0 - c1, before1 = before0 + c0;
    const bool take0 = v0 && mq_consumed(before0, r.n), take1 = v1 && mq_consumed(before1, r.n);
    if (take0) {
      f.items_sends += 1u + (c0 << 16);
      f.sends0_expired += x0 ? 1u << 16 : (c0 ? 0u : 1u);
      f.bad_ref |= b0 ? 1u : 0u;
    }
    if (take1) {
      f.items_sends += 1u + (c1 << 16);
      f.sends0_expired += x1 ? 1u << 16 : (c1 ? 0u : 1u);
      f.bad_ref |= b1 ? 1u : 0u;
    }
    if (EMIT) {
      const uint32_t ref[2] = {e.x, e.z}, opt[2] = {e.y, e.w}, before[2] = {before0, before1};
      const bool take[2] = {take0, take1}, expired[2] = {x0, x1};
#pragma unroll
      for (uint32_t i = 0; i < 2; ++i) {
        const uint64_t pos = off + (i1 - 1 + i);
        if (!take[i] || pos >= a.cap_out) continue;
        uint16_t id;
        const uint8_t verdict = mq_item(static_cast<uint8_t>(opt[i]), expired[i], r.next_pkt, before[i], &id);
        a.out_opts[pos] = static_cast<uint8_t>(opt[i]);
        a.out_verdicts[pos] = verdict;
        a.out_pkt_ids[pos] = id;
        a.out_refs[pos] = ref[i];
      }
    }
    carry += trip;
  }
  for (uint32_t d = 1; d < G; d <<= 1) {
    f.items_sends += __shfl_xor(f.items_sends, d, 64);
    f.sends0_expired += __shfl_xor(f.sends0_expired, d, 64);
    f.bad_ref |= __shfl_xor(f.bad_ref, d, 64);
  }
  return f;
}

__global__ __launch_bounds__(AK_BLOCK) void mq_take_count_kernel(MqTakeArgs a) {
  __shared__ uint32_t wsum[MQ_WAVES];
  uint64_t m;
  if (!mq_take_count(a, &m)) return;
  const uint32_t G = mq_group(a.q), per_block = AK_BLOCK / G;
  const uint32_t group = threadIdx.x / G, j = threadIdx.x % G, lane0 = (threadIdx.x & 63u) - j;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const MqRow r = mq_row_of(a, k, valid);
    const MqFound f = mq_fold<false>(a, r, G, j, lane0, 0);
    const uint32_t items = f.items_sends & 0xFFFFu;
    if (valid && j == 0) a.out_offsets[k] = items;  // (the emit pass turns the counts into offsets)
    const uint32_t c = wave_sum(j == 0 ? items : 0u);
    __syncthreads();  // the readers of the trip before are done
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
      for (uint32_t w = 0; w < MQ_WAVES; ++w) all += wsum[w];
      a.tile_tot[base / per_block] = all;  // (base < m <= cap_boxes: a tile of the scratch)
    }
  }
}

// One block: tile_tot becomes its exclusive scan, scan_chunk tiles a carry step.
__global__ __launch_bounds__(AK_SCAN_BLOCK) void mq_take_scan_kernel(MqTakeArgs a) {
  __shared__ uint64_t wsum[AK_SCAN_BLOCK / 64];
  if (threadIdx.x < MQ_C_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m;
  if (!mq_take_count(a, &m)) return;
  const uint64_t total = block_scan_in_place<AK_SCAN_BLOCK>(a.tile_tot, a.tile_tot, mq_take_tiles(m, a.q), wsum,
                                                            scan_chunk_of<AK_SCAN_BLOCK>(a.scan_chunk));
  __syncthreads();  // the zeroing above
  if (threadIdx.x == 0) {
    a.ctr[MQ_C_TOTAL] = total;
    a.ctr[MQ_C_FULL] = total > a.cap_out ? 1ull : 0ull;
    a.out_offsets[m] = total;
  }
}

__global__ __launch_bounds__(AK_BLOCK) void mq_take_emit_kernel(MqTakeArgs a) {
  __shared__ uint32_t wsum[MQ_WAVES];
  uint64_t m;
  if (!mq_take_count(a, &m)) return;
  const bool full = a.ctr[MQ_C_FULL] != 0;
  const uint32_t G = mq_group(a.q), per_block = AK_BLOCK / G;
  const uint32_t group = threadIdx.x / G, j = threadIdx.x % G, lane0 = (threadIdx.x & 63u) - j;
  uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};  // OK sessions, -, -, sends, sends QoS 0, expired, len mismatches
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const MqRow r = mq_row_of(a, k, valid);
    const uint32_t counted = (valid && j == 0) ? static_cast<uint32_t>(a.out_offsets[k]) : 0u;  // (the count pass's)
    uint32_t tile_items;  // (not used: the scan kernel has the tile's base)
    const uint32_t pre = block_excl_scan<AK_BLOCK>(counted, wsum, &tile_items);
    const uint64_t off = a.tile_tot[base / per_block] + __shfl(pre, lane0, 64);
    MqFound f{0, 0, 0};
    if (full) f = mq_fold<false>(a, r, G, j, lane0, off);
    else f = mq_fold<true>(a, r, G, j, lane0, off);
    if (valid && j == 0) {
      uint4 counts = make_uint4(0, 0, 0, 0);
      if (!r.dead) {
        const uint32_t items = f.items_sends & 0xFFFFu, sends = f.items_sends >> 16;
        counts = make_uint4(sends, f.sends0_expired & 0xFFFFu, f.sends0_expired >> 16, r.L - items);
        acc[0] += 1;
        acc[3] += counts.x;
        acc[4] += counts.y;
        acc[5] += counts.z;
        if (r.mq_len != r.L) {
          acc[6] += 1;
          flags |= MQ_F_LEN_MISMATCH;
        }
        if (r.bad_ring) flags |= MQ_F_BAD_RING;
        if (f.bad_ref) flags |= MQ_F_BAD_REF;
        if (a.update_table && !full) {
          uint32_t* rec = a.sessions + r.sub * AK_REC_WORDS;
          a.heads[r.sub] = make_uint2((r.h + items) & (a.q - 1), r.L - items);
          rec[MQ_REC_MQ_LEN] = r.L - items;
          if (sends) {
            rec[AK_REC_INFLIGHT] = wn_sat32(static_cast<uint64_t>(r.inflight) + sends);
            rec[MQ_REC_NEXT_PKT] = mq_next_pkt(r.next_pkt, sends);
          }
        }
      }
      a.out_offsets[k] = off;
      a.out_status[k] = r.dead ? r.dead : AK_OK;
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = counts;
      if (r.sub >= a.sub_limit) flags |= MQ_F_BAD_SUB;
    }
  }
  block_report<7>(a.ctr, MQ_T_OKS, acc, flags, MQ_S_FLAGS);
}

__global__ void mq_take_finish_kernel(MqTakeArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m;
  uint64_t s[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = mq_take_count(a, &m);
  if (!go) {
    s[MQ_S_FLAGS] = MQ_F_INPUT_REFUSED;
  } else {
    for (uint32_t k = 0; k < MQ_S_WORDS; ++k) s[k] = a.ctr[k];
    s[MQ_T_ITEMS] = a.ctr[MQ_C_TOTAL];
    if (a.ctr[MQ_C_FULL]) s[MQ_S_FLAGS] |= MQ_F_OUTPUT_FULL;
  }
  s[MQ_S_BOXES] = m;
  for (uint32_t k = 0; k < MQ_S_WORDS; ++k) a.summary[k] = s[k];
}

// The grid over `units` tiles; the blocks stride beyond the cap.
uint32_t mq_grid(uint64_t units, uint32_t max_blocks) {
  const uint32_t cap = max_blocks && max_blocks < AK_MAX_BLOCKS ? max_blocks : AK_MAX_BLOCKS;
  if (units == 0) units = 1;
  return static_cast<uint32_t>(units < cap ? units : cap);
}

}  // namespace

// Enqueues the passes of one put call.
int mq_launch_put(const MqPutArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t tiles = mq_grid(mq_tiles(a.cap_in), a.max_blocks);
  const uint32_t rows = mq_grid((a.cap_boxes + AK_BLOCK - 1) / AK_BLOCK, a.max_blocks);
  mq_put_heads_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  mq_put_scan_kernel<<<dim3(1), dim3(AK_SCAN_BLOCK), 0, s>>>(a);
  mq_put_evict_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  mq_put_rows_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  mq_put_store_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  mq_put_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

// Enqueues the passes of one take call.
int mq_launch_take(const MqTakeArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t rows = mq_grid(mq_take_tiles(a.cap_boxes, a.q), a.max_blocks);
  mq_take_count_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  mq_take_scan_kernel<<<dim3(1), dim3(AK_SCAN_BLOCK), 0, s>>>(a);
  mq_take_emit_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  mq_take_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
