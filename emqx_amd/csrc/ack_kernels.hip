// Kernels of the ack stage (include/emqx_ack.h).
//
// Record (behind the window stage): the r-th EMQX_W_SEND of an inbox goes into the r-th EMPTY slot
// of its session's row as the row was at entry.  One global exclusive prefix count of the SEND
// indicator over all deliveries gives every send its rank (its prefix minus the prefix at its
// inbox's head), as the window stage ranks its live deliveries:
//   ack_rec_heads_kernel  per tile: the block scan of the indicator, the tile's total, the prefix
//                         at every inbox head that lies in the tile;
//   ack_rec_scan_kernel   one block: the exclusive scan of the tile totals; zeroes the counters;
//   ack_rec_rows_kernel   W / 2 lanes a row, one 16-byte load a lane: the mask of the row's EMPTY
//                         slots at entry into the scratch, out_unrecorded, the counters;
//   ack_rec_place_kernel  per tile: the scan again; a send finds its inbox by a binary search
//                         narrowed to the tile's inboxes, takes the r-th set bit of the mask and
//                         stores its slot with one 8-byte store.  It reads the masks, never the
//                         rows other sends of the same launch are filling.
// Run (a batch of acks): three ack-parallel passes over tiles of all acks and one per slot,
//   ack_run_init_kernel     first[] and comp[] of the m rows to AK_NONE; zeroes the counters;
//   ack_run_first_kernel    an ack finds its session (the narrowed search) and its slot (the row,
//                           16 bytes a load); a PUBACK or PUBREC does atomicMin on first[];
//   ack_run_comp_kernel     a PUBCOMP that can complete its slot (ak_comp_counts) does atomicMin
//                           on comp[];
//   ack_run_verdict_kernel  what the ack sees in its slot (ak_phase_at), its verdict and ref;
//   ack_run_rows_kernel     W / 2 lanes a row: the phase of every slot behind the last ack, the
//                           row rewritten, the four counts, sessions[].inflight with update_table.
// Between the first and the verdict pass an ack's slot index rides in verdicts[] (one byte an
// ack; tuning key "rematch" matches it against the row again in every pass instead).  No kernel
// rewrites rows while another block of the same launch reads them: the rows change in
// ack_run_rows_kernel alone, where a row is read and written by its own lanes only.
// No thread iterates over an inbox or an ack list.  The atomics are minima, sums and an OR: every
// output byte is a function of the input alone.
//
// Every index is bounded before use: a position < offsets[m] <= cap_in, an inbox or session index
// < m <= cap_boxes, a subscriber id < sub_limit, a slot < w, a tile < max(1, ceil(cap_in /
// AK_TILE)).  The counts are read on the device; the host sizes the grids by cap_in and cap_boxes.
#include <hip/hip_runtime.h>

#include "ack.h"

namespace emqx {

namespace {

constexpr uint32_t AK_WAVES = AK_BLOCK / 64;
constexpr uint8_t AK_NO_SLOT = 0xFF;

// m and offsets[m] when this call may use them; false: the call is refused.
__device__ inline bool ak_counts(const uint64_t* n_boxes, uint64_t m_arg, uint64_t cap_boxes, const uint64_t* offsets,
                                 uint64_t cap_in, uint64_t max_total, uint64_t* m, uint64_t* total) {
  *m = n_boxes ? *n_boxes : m_arg;
  *total = 0;
  if (*m > cap_boxes || *m > AK_MAX_TOTAL) return false;
  *total = offsets[*m];
  return *total <= cap_in && *total <= max_total;
}

__device__ inline uint64_t ak_tiles_eff(uint64_t total) {  // a call without positions still has its rows
  const uint64_t t = ak_tiles(total);
  return t ? t : 1;
}

// The inboxes a tile's positions can belong to, as bounds of csr_upper: thread 0 and 1 search the
// whole array once a tile.  ext[0] <= ext[1] <= m + 1.
__device__ inline void ak_tile_extent(const uint64_t* offsets, uint64_t m, uint64_t ts, uint64_t total, uint64_t* ext) {
  __syncthreads();  // the readers of the tile before are done
  if (threadIdx.x == 0) ext[0] = csr_upper(offsets, 0, m + 1, ts);
  if (threadIdx.x == 1) {
    const uint64_t end = total - ts < AK_TILE ? total : ts + AK_TILE;  // (ts < total)
    ext[1] = csr_upper(offsets, 0, m + 1, end - 1);
  }
  __syncthreads();
}

// The inbox of position d: the last k with offsets[k] <= d.  AK_NONE when the offsets name none
// (they do not start at 0).  *k_at: the answer for the position before, tried first.
__device__ inline uint64_t ak_box_of(const uint64_t* offsets, uint64_t m, const uint64_t* ext, uint64_t d, uint64_t k_at) {
  if (k_at < m && offsets[k_at] <= d && d < offsets[k_at + 1]) return k_at;
  const uint64_t lo = ext[0], hi = ext[1] < lo ? lo : ext[1];
  const uint64_t u = csr_upper(offsets, lo, hi, d);
  return (u >= 1 && u <= m) ? u - 1 : AK_NONE;
}

// ---- record ------------------------------------------------------------------------------------

__device__ inline bool ak_rec_counts(const AkRecArgs& a, uint64_t* m, uint64_t* total) {
  return ak_counts(a.n_boxes, a.m, a.cap_boxes, a.inbox_offsets, a.cap_in, AK_MAX_TOTAL, m, total);
}

// The SEND indicators of positions p0 .. p0 + AK_ROWS as bits.
__device__ inline uint32_t ak_load_sends(const uint8_t* verdicts, uint64_t p0, uint64_t total) {
  uint32_t bits = 0;
  if (p0 + AK_ROWS <= total && ((reinterpret_cast<uintptr_t>(verdicts) + p0) & 3u) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(verdicts + p0);
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) bits |= (((w >> (8 * j)) & AK_W_MASK) == AK_W_SEND ? 1u : 0u) << j;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j)
      if (p0 + j < total && (verdicts[p0 + j] & AK_W_MASK) == AK_W_SEND) bits |= 1u << j;
  }
  return bits;
}

// The global prefix at the head of inbox k (k <= m).
__device__ inline uint32_t ak_base(const AkRecArgs& a, uint64_t k, uint64_t total, uint64_t tiles) {
  const uint64_t off = a.inbox_offsets[k];
  const uint64_t p = off < total ? off : total;
  uint64_t t = p / AK_TILE;
  if (t >= tiles) t = tiles - 1;
  return a.tile_tot[t] + a.head_pre[k];
}

__global__ __launch_bounds__(AK_BLOCK) void ack_rec_heads_kernel(AkRecArgs a) {
  __shared__ uint32_t pre[AK_TILE + 1];  // exclusive prefix at every position of the tile, and at its end
  __shared__ uint32_t wsum[AK_WAVES];
  uint64_t m, total;
  if (!ak_rec_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles_eff(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * AK_TILE;
    const bool last = tile + 1 == tiles;
    const uint32_t bits = ak_load_sends(a.verdicts, ts + static_cast<uint64_t>(threadIdx.x) * AK_ROWS, total);
    uint32_t all;
    uint32_t run = block_excl_scan<AK_BLOCK>(static_cast<uint32_t>(__popc(bits)), wsum, &all);
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) {
      pre[threadIdx.x * AK_ROWS + j] = run;
      run += (bits >> j) & 1u;
    }
    if (threadIdx.x == 0) {
      pre[AK_TILE] = all;
      a.tile_tot[tile] = all;
    }
    __syncthreads();
    // the inboxes whose head lies in [ts, ts + AK_TILE); the last tile also takes the heads at its
    // end (inboxes without deliveries behind the last delivery, and inbox_offsets[m] itself)
    const uint64_t k_lo = csr_lower(a.inbox_offsets, 0, m + 1, ts);
    const uint64_t k_hi = last ? m + 1 : csr_lower(a.inbox_offsets, 0, m + 1, ts + AK_TILE);
    for (uint64_t k = k_lo + threadIdx.x; k < k_hi; k += AK_BLOCK) {
      const uint64_t off = a.inbox_offsets[k];
      const uint64_t p = off < total ? off : total;
      if (p >= ts && p - ts <= (last ? AK_TILE : AK_TILE - 1)) a.head_pre[k] = pre[p - ts];
    }
    __syncthreads();  // the next tile writes pre
  }
}

// One block: tile_tot becomes its exclusive scan, scan_chunk tiles a carry step
// (stage_common.h's block_scan_in_place).
__global__ __launch_bounds__(AK_SCAN_BLOCK) void ack_rec_scan_kernel(AkRecArgs a) {
  __shared__ uint32_t wsum[AK_SCAN_BLOCK / 64];
  if (threadIdx.x < AK_S_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m, total;
  if (!ak_rec_counts(a, &m, &total)) return;
  (void)block_scan_in_place<AK_SCAN_BLOCK>(a.tile_tot, a.tile_tot, ak_tiles_eff(total), wsum,
                                           scan_chunk_of<AK_SCAN_BLOCK>(a.scan_chunk));
}

// a.w / 2 lanes a row.  The loop is uniform over the block: the shuffles see every lane.
__global__ __launch_bounds__(AK_BLOCK) void ack_rec_rows_kernel(AkRecArgs a) {
  uint64_t m, total;
  if (!ak_rec_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles_eff(total);
  const uint32_t lanes = a.w / 2, per_block = AK_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  uint64_t acc[4] = {0, 0, 0, 0};  // sends, recorded, unrecorded, full rows
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const uint32_t sub = valid ? a.inbox_subs[k] : 0u;
    const bool ok = valid && sub < a.sub_limit;
    uint64_t part = 0;
    if (ok) {
      const uint4 s = reinterpret_cast<const uint4*>(a.slots)[static_cast<uint64_t>(sub) * lanes + j];
      part = static_cast<uint64_t>((ak_phase(s.x) == AK_EMPTY ? 1u : 0u) | (ak_phase(s.z) == AK_EMPTY ? 2u : 0u)) << (2 * j);
    }
    for (uint32_t d = 1; d < lanes; d <<= 1) part |= __shfl_xor(part, d, 64);
    if (valid && j == 0) {
      const uint32_t sends = ak_base(a, k + 1, total, tiles) - ak_base(a, k, total, tiles);
      const uint32_t nfree = static_cast<uint32_t>(__popcll(part));
      const uint32_t rec = sends < nfree ? sends : nfree;
      a.masks[k] = part;
      a.out_unrecorded[k] = sends - rec;
      acc[0] += sends;
      acc[1] += rec;
      acc[2] += sends - rec;
      if (ok && sends > rec) {
        acc[3] += 1;
        flags |= AK_F_ROW_FULL;
      }
      if (!ok) flags |= AK_F_BAD_SUB;
    }
  }
  block_report<4>(a.ctr, AK_R_SENDS, acc, flags, AK_S_FLAGS);
}

__global__ __launch_bounds__(AK_BLOCK) void ack_rec_place_kernel(AkRecArgs a) {
  __shared__ uint32_t wsum[AK_WAVES];
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!ak_rec_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * AK_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * AK_ROWS;
    const uint32_t bits = ak_load_sends(a.verdicts, p0, total);
    uint32_t all;
    uint32_t run = a.tile_tot[tile] + block_excl_scan<AK_BLOCK>(static_cast<uint32_t>(__popc(bits)), wsum, &all);
    ak_tile_extent(a.inbox_offsets, m, ts, total, ext);
    uint64_t k = AK_NONE;
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) {
      if (!((bits >> j) & 1u)) continue;  // (a set bit: p0 + j < total)
      const uint64_t d = p0 + j;
      const uint32_t g = run++;
      k = ak_box_of(a.inbox_offsets, m, ext, d, k);
      if (k == AK_NONE) continue;
      const uint32_t r = g - ak_base(a, k, total, tiles);
      const uint64_t mask = a.masks[k];  // (0 for a subscriber id that is not below sub_limit)
      if (r >= static_cast<uint32_t>(__popcll(mask))) continue;
      const uint32_t slot = ak_nth_set(mask, r);  // (< a.w: the mask has no bit beyond)
      const uint32_t sub = a.inbox_subs[k];
      if (sub >= a.sub_limit || slot >= a.w) continue;
      a.slots[static_cast<uint64_t>(sub) * a.w + slot] =
          make_uint2(ak_word0(a.pkt_ids[d], AK_MSG, a.box_opts[d] & AK_O_QOS), a.refs ? a.refs[d] : static_cast<uint32_t>(d));
    }
  }
}

__global__ void ack_rec_finish_kernel(AkRecArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = ak_rec_counts(a, &m, &total);
  s[AK_S_BOXES] = m;
  if (!go) {
    s[AK_S_FLAGS] = AK_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= AK_MAX_TOTAL) s[AK_S_TOTAL] = a.inbox_offsets[m];
  } else {
    s[AK_S_TOTAL] = total;
    s[AK_S_FLAGS] = a.ctr[AK_S_FLAGS];
    for (uint32_t k = AK_R_SENDS; k < AK_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < AK_S_WORDS; ++k) a.summary[k] = s[k];
}

// ---- run ---------------------------------------------------------------------------------------

__device__ inline bool ak_run_counts(const AkRunArgs& a, uint64_t* m, uint64_t* total) {
  return ak_counts(a.n_boxes, a.m, a.cap_boxes, a.ack_offsets, a.cap_in, AK_MAX_ACKS, m, total);
}

__global__ __launch_bounds__(AK_BLOCK) void ack_run_init_kernel(AkRunArgs a) {
  if (blockIdx.x == 0 && threadIdx.x < AK_S_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m, total;
  if (!ak_run_counts(a, &m, &total)) return;
  const uint64_t quads = m * a.w / 4;  // (w is a multiple of 8; both arrays are 16-byte aligned)
  const uint4 none = make_uint4(AK_NONE, AK_NONE, AK_NONE, AK_NONE);
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * AK_BLOCK + threadIdx.x; i < quads; i += static_cast<uint64_t>(gridDim.x) * AK_BLOCK) {
    reinterpret_cast<uint4*>(a.first)[i] = none;
    reinterpret_cast<uint4*>(a.comp)[i] = none;
  }
}

// The acks of positions p0 .. p0 + AK_ROWS (0, a bad kind, behind `total`).
__device__ inline void ak_load_acks(const uint32_t* acks, uint64_t p0, uint64_t total, uint32_t v[AK_ROWS]) {
  if (p0 + AK_ROWS <= total && ((reinterpret_cast<uintptr_t>(acks) + 4 * p0) & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(acks + p0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) v[j] = p0 + j < total ? acks[p0 + j] : 0u;
  }
}

__device__ inline bool ak_kind_ok(uint32_t ack) { return (ack >> 16) >= AK_PUBACK && (ack >> 16) <= AK_PUBCOMP; }

// The session of list k: its subscriber id and 0, or the verdict of all its acks.
__device__ inline uint8_t ak_session_of(const AkRunArgs& a, uint64_t k, uint32_t* sub) {
  *sub = a.ack_subs[k];
  const bool ok = *sub < a.sub_limit;
  return ak_session(ok, ok ? a.sessions[static_cast<uint64_t>(*sub) * AK_REC_WORDS + AK_REC_FLAGS] : 0u);
}

// The lowest slot of row `sub` that holds pkt_id, or AK_NO_SLOT.
__device__ inline uint8_t ak_match(const AkRunArgs& a, uint32_t sub, uint32_t pkt_id) {
  const uint4* row = reinterpret_cast<const uint4*>(a.slots + static_cast<uint64_t>(sub) * a.w);
  for (uint32_t j = 0; j < a.w / 2; ++j) {
    const uint4 s = row[j];
    if (ak_hit(s.x, pkt_id)) return static_cast<uint8_t>(2 * j);
    if (ak_hit(s.z, pkt_id)) return static_cast<uint8_t>(2 * j + 1);
  }
  return AK_NO_SLOT;
}

__device__ inline void ak_store_bytes(uint8_t* out, uint64_t p0, uint64_t total, const uint8_t v[AK_ROWS]) {
  if (p0 + AK_ROWS <= total && ((reinterpret_cast<uintptr_t>(out) + p0) & 3u) == 0) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) w |= static_cast<uint32_t>(v[j]) << (8 * j);
    *reinterpret_cast<uint32_t*>(out + p0) = w;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j)
      if (p0 + j < total) out[p0 + j] = v[j];
  }
}

__global__ __launch_bounds__(AK_BLOCK) void ack_run_first_kernel(AkRunArgs a) {
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!ak_run_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * AK_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * AK_ROWS;
    uint32_t ack[AK_ROWS];
    ak_load_acks(a.acks, p0, total, ack);
    ak_tile_extent(a.ack_offsets, m, ts, total, ext);
    uint8_t slot[AK_ROWS];
    uint64_t k = AK_NONE;
    uint32_t sub = 0;
    uint8_t dead = AK_NO_SESSION;
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) {
      slot[j] = AK_NO_SLOT;
      if (p0 + j >= total || !ak_kind_ok(ack[j])) continue;
      const uint64_t k_was = k;
      k = ak_box_of(a.ack_offsets, m, ext, p0 + j, k);
      if (k == AK_NONE) continue;
      if (k != k_was) dead = ak_session_of(a, k, &sub);
      if (dead) continue;
      slot[j] = ak_match(a, sub, ack[j] & 0xFFFFu);
      if (slot[j] == AK_NO_SLOT || (ack[j] >> 16) == AK_PUBCOMP) continue;
      const uint32_t p = static_cast<uint32_t>(p0 + j - a.ack_offsets[k]) & 0x7FFFFFFFu;
      atomicMin(a.first + k * a.w + slot[j], p * 2u + ((ack[j] >> 16) == AK_PUBREC ? 1u : 0u));
    }
    if (!a.rematch && p0 < total) ak_store_bytes(a.verdicts, p0, total, slot);
  }
}

__global__ __launch_bounds__(AK_BLOCK) void ack_run_comp_kernel(AkRunArgs a) {
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!ak_run_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * AK_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * AK_ROWS;
    uint32_t ack[AK_ROWS];
    ak_load_acks(a.acks, p0, total, ack);
    ak_tile_extent(a.ack_offsets, m, ts, total, ext);
    uint64_t k = AK_NONE;
    uint32_t sub = 0;
    uint8_t dead = AK_NO_SESSION;
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) {
      if (p0 + j >= total || (ack[j] >> 16) != AK_PUBCOMP) continue;
      const uint64_t k_was = k;
      k = ak_box_of(a.ack_offsets, m, ext, p0 + j, k);
      if (k == AK_NONE) continue;
      if (k != k_was) dead = ak_session_of(a, k, &sub);
      if (dead) continue;
      const uint8_t slot = a.rematch ? ak_match(a, sub, ack[j] & 0xFFFFu) : a.verdicts[p0 + j];
      if (slot >= a.w) continue;
      const uint32_t p = static_cast<uint32_t>(p0 + j - a.ack_offsets[k]) & 0x7FFFFFFFu;
      const uint32_t s0 = ak_phase(a.slots[static_cast<uint64_t>(sub) * a.w + slot].x);
      if (ak_comp_counts(s0, a.first[k * a.w + slot], p)) atomicMin(a.comp + k * a.w + slot, p);
    }
  }
}

__global__ __launch_bounds__(AK_BLOCK) void ack_run_verdict_kernel(AkRunArgs a) {
  __shared__ uint64_t ext[2];
  uint64_t m, total;
  if (!ak_run_counts(a, &m, &total)) return;
  const uint64_t tiles = ak_tiles(total);
  uint64_t acc[5] = {0, 0, 0, 0, 0};  // OK, (released: the rows kernel), IN_USE, NOT_FOUND, the rest
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * AK_TILE;
    const uint64_t p0 = ts + static_cast<uint64_t>(threadIdx.x) * AK_ROWS;
    uint32_t ack[AK_ROWS];
    ak_load_acks(a.acks, p0, total, ack);
    ak_tile_extent(a.ack_offsets, m, ts, total, ext);
    if (p0 >= total) continue;  // (behind the barriers)
    uint8_t stash[AK_ROWS] = {AK_NO_SLOT, AK_NO_SLOT, AK_NO_SLOT, AK_NO_SLOT};
    if (!a.rematch) {
#pragma unroll
      for (uint32_t j = 0; j < AK_ROWS; ++j)
        if (p0 + j < total) stash[j] = a.verdicts[p0 + j];
    }
    uint8_t v[AK_ROWS];
    uint32_t ref[AK_ROWS];
    uint64_t k = AK_NONE;
    uint32_t sub = 0;
    uint8_t dead = AK_NO_SESSION;
#pragma unroll
    for (uint32_t j = 0; j < AK_ROWS; ++j) {
      v[j] = AK_NO_SESSION;
      ref[j] = AK_NONE;
      if (p0 + j >= total) continue;
      const uint64_t k_was = k;
      k = ak_box_of(a.ack_offsets, m, ext, p0 + j, k);
      if (k != AK_NONE && k != k_was) dead = ak_session_of(a, k, &sub);
      if (k == AK_NONE || dead) {
        v[j] = k == AK_NONE ? AK_NO_SESSION : dead;
      } else if (!ak_kind_ok(ack[j])) {
        v[j] = AK_BAD_KIND;
      } else {
        const uint8_t slot = a.rematch ? ak_match(a, sub, ack[j] & 0xFFFFu) : stash[j];
        if (slot >= a.w) {
          v[j] = AK_NOT_FOUND;
        } else {
          const uint2 s = a.slots[static_cast<uint64_t>(sub) * a.w + slot];
          const uint32_t p = static_cast<uint32_t>(p0 + j - a.ack_offsets[k]) & 0x7FFFFFFFu;
          v[j] = ak_verdict(ack[j] >> 16, ak_phase_at(ak_phase(s.x), a.first[k * a.w + slot], a.comp[k * a.w + slot], p));
          if (v[j] == AK_OK) ref[j] = s.y;
        }
      }
      acc[v[j] == AK_OK ? 0 : v[j] == AK_IN_USE ? 2 : v[j] == AK_NOT_FOUND ? 3 : 4] += 1;
    }
    ak_store_bytes(a.verdicts, p0, total, v);
    if (p0 + AK_ROWS <= total && ((reinterpret_cast<uintptr_t>(a.out_refs) + 4 * p0) & 15u) == 0) {
      *reinterpret_cast<uint4*>(a.out_refs + p0) = make_uint4(ref[0], ref[1], ref[2], ref[3]);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < AK_ROWS; ++j)
        if (p0 + j < total) a.out_refs[p0 + j] = ref[j];
    }
  }
  block_report<5>(a.ctr, AK_A_OKS, acc, 0, AK_S_FLAGS);
}

// a.w / 2 lanes a session.  The loop is uniform over the block: the shuffles see every lane.
__global__ __launch_bounds__(AK_BLOCK) void ack_run_rows_kernel(AkRunArgs a) {
  uint64_t m, total;
  if (!ak_run_counts(a, &m, &total)) return;
  const uint32_t lanes = a.w / 2, per_block = AK_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  uint64_t acc[1] = {0};  // released
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    uint32_t sub = 0;
    const uint8_t dead = valid ? ak_session_of(a, k, &sub) : AK_NO_SESSION;
    uint32_t packed = 0;  // released, PUBREC OKs << 8, OKs << 16
    if (!dead) {
      uint4* at = reinterpret_cast<uint4*>(a.slots + static_cast<uint64_t>(sub) * a.w) + j;
      const uint4 s = *at;
      const uint2 f = *reinterpret_cast<const uint2*>(a.first + k * a.w + 2 * j);
      const uint2 c = *reinterpret_cast<const uint2*>(a.comp + k * a.w + 2 * j);
      uint32_t w0[2] = {s.x, s.z}, w1[2] = {s.y, s.w};
      const uint32_t fs[2] = {f.x, f.y}, cs[2] = {c.x, c.y};
      bool changed = false;
#pragma unroll
      for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t s0 = ak_phase(w0[i]);
        const uint32_t end = ak_phase_at(s0, fs[i], cs[i], AK_AT_END);
        if (end == s0) continue;
        changed = true;
        const bool rec = s0 == AK_MSG && (fs[i] & 1u);  // (first is not AK_NONE: the phase moved)
        if (end == AK_EMPTY) {
          packed += 1u + (rec ? (1u << 8) + (2u << 16) : (1u << 16));
          w0[i] = 0;
          w1[i] = 0;
        } else {  // MSG -> PUBREL_AWAIT
          packed += (1u << 8) + (1u << 16);
          w0[i] = ak_with_phase(w0[i], AK_AWAIT);
        }
      }
      if (changed) *at = make_uint4(w0[0], w1[0], w0[1], w1[1]);
    }
    for (uint32_t d = 1; d < lanes; d <<= 1) packed += __shfl_xor(packed, d, 64);
    if (valid && j == 0) {
      uint4 counts = make_uint4(0, 0, 0, 0);
      if (!dead) {
        const uint64_t off = a.ack_offsets[k], nxt = a.ack_offsets[k + 1];
        const uint64_t lo = off < total ? off : total;
        const uint64_t hi = nxt < lo ? lo : (nxt < total ? nxt : total);
        const uint32_t released = packed & 0xFFu, oks = packed >> 16;
        uint32_t* rec = a.sessions + static_cast<uint64_t>(sub) * AK_REC_WORDS;
        const uint32_t after = ak_inflight_after(rec[AK_REC_INFLIGHT], released);
        counts = make_uint4(released, (packed >> 8) & 0xFFu, static_cast<uint32_t>(hi - lo) - oks, ak_room(rec[AK_REC_INFLIGHT_MAX], after));
        if (a.update_table) rec[AK_REC_INFLIGHT] = after;
        acc[0] += released;
      }
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = counts;
      if (sub >= a.sub_limit) flags |= AK_F_BAD_SUB;
    }
  }
  block_report<1>(a.ctr, AK_A_RELEASED, acc, flags, AK_S_FLAGS);
}

__global__ void ack_run_finish_kernel(AkRunArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = ak_run_counts(a, &m, &total);
  s[AK_S_BOXES] = m;
  if (!go) {
    s[AK_S_FLAGS] = AK_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= AK_MAX_TOTAL) s[AK_S_TOTAL] = a.ack_offsets[m];
  } else {
    s[AK_S_TOTAL] = total;
    s[AK_S_FLAGS] = a.ctr[AK_S_FLAGS];
    for (uint32_t k = AK_A_OKS; k < AK_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < AK_S_WORDS; ++k) a.summary[k] = s[k];
}

// The grid over `units` tiles or groups of rows; the blocks stride beyond the cap.
uint32_t ak_grid(uint64_t units, uint32_t max_blocks) {
  const uint32_t cap = max_blocks && max_blocks < AK_MAX_BLOCKS ? max_blocks : AK_MAX_BLOCKS;
  if (units == 0) units = 1;
  return static_cast<uint32_t>(units < cap ? units : cap);
}

}  // namespace

// Enqueues the passes of one record call.
int ak_launch_record(const AkRecArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t tiles = ak_grid(ak_tiles(a.cap_in), a.max_blocks);
  const uint32_t rows = ak_grid((a.cap_boxes + AK_BLOCK / (a.w / 2) - 1) / (AK_BLOCK / (a.w / 2)), a.max_blocks);
  ack_rec_heads_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  ack_rec_scan_kernel<<<dim3(1), dim3(AK_SCAN_BLOCK), 0, s>>>(a);
  ack_rec_rows_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  ack_rec_place_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  ack_rec_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

// Enqueues the passes of one run call.
int ak_launch_run(const AkRunArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t tiles = ak_grid(ak_tiles(a.cap_in), a.max_blocks);
  const uint32_t rows = ak_grid((a.cap_boxes + AK_BLOCK / (a.w / 2) - 1) / (AK_BLOCK / (a.w / 2)), a.max_blocks);
  ack_run_init_kernel<<<dim3(ak_grid((a.cap_boxes * a.w / 4 + AK_BLOCK - 1) / AK_BLOCK, a.max_blocks)), dim3(AK_BLOCK), 0, s>>>(a);
  ack_run_first_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  ack_run_comp_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  ack_run_verdict_kernel<<<dim3(tiles), dim3(AK_BLOCK), 0, s>>>(a);
  ack_run_rows_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  ack_run_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
