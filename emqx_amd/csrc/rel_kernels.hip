// Kernels of the rel stage (include/emqx_rel.h), for gfx950 and wave64.
//
// Run (a batch of inbound PUBLISH / PUBREL grouped by session):
//   rel_init_kernel        zeroes the counters;
//   rel_run_fold_kernel    L lanes a session (max(4, W / 16), tuning key "lanes"): the row lives
//                          in the group's registers, E = W / L consecutive entries a lane, loaded 16
//                          bytes (two entries) at a time.  The session's events are loaded L at a
//                          time, coalesced (with their stamps where ts[] is given, one chunk ahead of
//                          the steps), and stepped through by broadcast within the group.  A
//                          step is an id compare against the lane's E entries, one ballot masked to
//                          the group (who holds the id; the lowest lane holds the lowest slot, the
//                          lanes take consecutive slots) and one broadcast of that lane's entry
//                          index; which slots are taken is a 128-bit mask every lane of the group
//                          keeps, so the count is kept across steps and the lowest empty slot is a
//                          find-first-set.  A lane keeps the verdict of the event it loaded and the
//                          group stores verdicts L at a time.  No LDS.  A lane whose entries changed
//                          stores them once behind the last event; an unchanged row is not stored.
//   rel_route_count_kernel per tile of RL_TILE events: the routed events (OK PUBLISH and DIRECT);
//   rel_route_scan_kernel  one block: the exclusive scan of the tile totals
//                          (stage_common.h's block_scan_in_place); its sum is summary word 3;
//   rel_route_place_kernel per tile: the block scan again, out_route[rank] = src[d] or d;
//   rel_run_finish_kernel  the summary, written last.
// Expire: rel_init_kernel; rel_expire_kernel, W / 2 lanes a session and one 16-byte pair a lane, the
// predicate per entry (rl_expired), the counts by a reduction over the group, only changed pairs
// stored; rel_expire_finish_kernel.
//
// A session of n events costs n dependent steps of its group: one very long session bounds a run
// call from below (measured in DESIGN.md §3.17).
//
// Every index is bounded before use: a session's events are [lo, hi) clamped into [0, total] with
// hi >= lo and total = ev_offsets[m] <= cap_in, so no fold runs past cap_in steps; a session index
// < m <= cap_boxes, a subscriber id < sub_limit, a slot < w, a tile < ceil(total / RL_TILE), a rank
// of the route list < cap_in.  The counts are read on the device; the host sizes the grids by
// cap_in and cap_boxes.
#include <hip/hip_runtime.h>

#include "rel.h"

namespace emqx {

namespace {

constexpr uint32_t RL_WAVES = RL_BLOCK / 64;

// m and ev_offsets[m] when this call may use them; false: the call is refused.
__device__ inline bool rl_run_counts(const RlRunArgs& a, uint64_t* m, uint64_t* total) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  *total = 0;
  if (*m > a.cap_boxes || *m > RL_MAX_TOTAL) return false;
  *total = a.ev_offsets[*m];
  return *total <= a.cap_in && *total <= RL_MAX_EVENTS;
}
__device__ inline bool rl_exp_counts(const RlExpArgs& a, uint64_t* m) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  return *m <= a.cap_boxes && *m <= RL_MAX_TOTAL;
}

__global__ void rel_init_kernel(unsigned long long* ctr) {
  if (blockIdx.x == 0 && threadIdx.x < RL_S_WORDS) ctr[threadIdx.x] = 0;
}

// ---- run: the fold -----------------------------------------------------------------------------

// E entries a lane, L = a.w / E lanes a session.  The loops are uniform over the wave: the
// shuffles and the ballot see every lane.
template <uint32_t E>
__global__ __launch_bounds__(RL_BLOCK) void rel_run_fold_kernel(RlRunArgs a) {
  uint64_t m, total;
  if (!rl_run_counts(a, &m, &total)) return;
  const uint32_t L = a.w / E, per_block = RL_BLOCK / L;
  const uint32_t group = threadIdx.x / L, j = threadIdx.x % L;
  const uint32_t gshift = (threadIdx.x & 63u) & ~(L - 1u);
  const uint64_t gmask = L == 64 ? ~0ull : ((1ull << L) - 1ull);
  uint64_t acc[4] = {0, 0, 0, 0};  // released, IN_USE, NOT_FOUND, EXCEEDED
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    uint32_t sub = 0, limit = 0, n = 0;
    uint64_t lo = 0;
    uint8_t dead = RL_NO_SESSION;
    if (valid) {
      sub = a.ev_subs[k];
      const bool ok = sub < a.sub_limit;
      limit = ok ? (a.maxes ? a.maxes[sub] : a.max_awaiting) : 0u;
      dead = rl_session(ok, ok ? a.sessions[static_cast<uint64_t>(sub) * RL_REC_WORDS + RL_REC_FLAGS] : 0u, limit, a.w);
      const uint64_t off = a.ev_offsets[k], nxt = a.ev_offsets[k + 1];
      lo = off < total ? off : total;
      const uint64_t hi = nxt < lo ? lo : (nxt < total ? nxt : total);
      n = static_cast<uint32_t>(hi - lo);  // (<= total < 2^31)
      if (j == 0) flags |= (ok ? 0u : RL_F_BAD_SUB) | (dead == RL_ROW_SMALL ? RL_F_ROW_SMALL : 0u);
    }
    // the row: entries j * E .. j * E + E - 1 of it in this lane
    uint64_t ent[E];
#pragma unroll
    for (uint32_t e = 0; e < E; ++e) ent[e] = 0;
    ulonglong2* rowp = nullptr;
    if (!dead) {
      rowp = reinterpret_cast<ulonglong2*>(a.rel + static_cast<uint64_t>(sub) * a.w + static_cast<uint64_t>(j) * E);
#pragma unroll
      for (uint32_t i = 0; i < E / 2; ++i) {
        const ulonglong2 q = rowp[i];
        ent[2 * i] = q.x;
        ent[2 * i + 1] = q.y;
      }
    }
    // the slots taken, bit s of occ[s / 64], the same in every lane of the group
    uint64_t occ[2] = {0, 0};
#pragma unroll
    for (uint32_t e = 0; e < E; ++e) {
      const uint32_t s = j * E + e;
      if (ent[e] != 0) occ[s >> 6] |= 1ull << (s & 63u);
    }
    for (uint32_t d = 1; d < L; d <<= 1) {
      occ[0] |= __shfl_xor(occ[0], d, 64);
      occ[1] |= __shfl_xor(occ[1], d, 64);
    }
    uint32_t cnt = static_cast<uint32_t>(__popcll(occ[0]) + __popcll(occ[1]));
    uint32_t nmax = n;  // the longest list of the wave
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
      const uint32_t y = __shfl_xor(nmax, d, 64);
      nmax = y > nmax ? y : nmax;
    }
    uint32_t routed = 0, released = 0, in_use = 0, not_found = 0, exceeded = 0, bad_kind = 0, arm = 0;
    bool dirty = false;
    // the chunk behind the one being stepped through is loaded ahead of it
    uint32_t ev_next = j < n ? a.events[lo + j] : 0u;
    uint64_t ts_next = (j < n && a.ts) ? a.ts[lo + j] : a.now_ms;
    for (uint32_t c0 = 0; c0 < nmax; c0 += L) {
      const bool have = c0 + j < n;
      const uint64_t d_mine = lo + c0 + j;
      const uint32_t ev_mine = ev_next;
      const uint64_t ts_mine = ts_next;
      const bool more = c0 + L + j < n;
      ev_next = more ? a.events[d_mine + L] : 0u;
      ts_next = (more && a.ts) ? a.ts[d_mine + L] : a.now_ms;
      uint8_t v_mine = dead;
      const uint32_t steps = nmax - c0 < L ? nmax - c0 : L;
      for (uint32_t s = 0; s < steps; ++s) {
        const uint32_t ev = __shfl(ev_mine, static_cast<int>(s), static_cast<int>(L));
        const uint64_t ts_ev = __shfl(ts_mine, static_cast<int>(s), static_cast<int>(L));
        const bool live = !dead && c0 + s < n;  // the same in every lane of the group
        const uint32_t kind = ev >> 16, id = ev & 0xFFFFu;
        uint32_t at = E;  // the lowest entry of this lane that holds the id
#pragma unroll
        for (uint32_t e = E; e-- > 0;)
          if (rl_hit(ent[e], id)) at = e;
        const uint64_t holders = (__ballot(live && at < E) >> gshift) & gmask;
        const bool present = holders != 0;
        const uint32_t winner = present ? static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(holders))) - 1u : 0u;
        const uint32_t at_w = __shfl(at, static_cast<int>(winner), static_cast<int>(L));
        if (!live) continue;
        const uint8_t v = rl_verdict(kind, cnt, limit, present);
        if (j == s) v_mine = v;
        if (v == RL_OK && kind == RL_PUBLISH) {
          // (cnt < limit <= w: the row has an empty slot below w)
          const unsigned long long f0 = ~occ[0], f1 = ~occ[1];
          const uint32_t slot = f0 ? static_cast<uint32_t>(__ffsll(f0)) - 1u : 64u + static_cast<uint32_t>(__ffsll(f1)) - 1u;
          if (slot < a.w) {
            bool bad;
            const uint64_t stamp = rl_stamp(ts_ev, &bad);
            if (slot / E == j) {
              const uint64_t x = rl_entry(stamp, id);
#pragma unroll
              for (uint32_t e = 0; e < E; ++e)
                if (e == slot % E) ent[e] = x;
              dirty = true;
              if (bad) flags |= RL_F_BAD_TS;
            }
            occ[slot >> 6] |= 1ull << (slot & 63u);
            ++cnt;
          }
          arm = 1;
          ++routed;
        } else if (v == RL_OK && kind == RL_PUBREL) {
          const uint32_t slot = winner * E + (at_w < E ? at_w : 0u);
          if (j == winner) {
#pragma unroll
            for (uint32_t e = 0; e < E; ++e)
              if (e == at_w) ent[e] = 0;
            dirty = true;
          }
          occ[(slot >> 6) & 1u] &= ~(1ull << (slot & 63u));
          --cnt;
          ++released;
        } else if (v == RL_OK) {
          ++routed;
        } else {
          in_use += v == RL_IN_USE;
          not_found += v == RL_NOT_FOUND;
          exceeded += v == RL_EXCEEDED;
          bad_kind += v == RL_BAD_KIND;
        }
      }
      if (have) a.verdicts[d_mine] = v_mine;
    }
    if (dirty) {  // (a lane of a session that takes events)
#pragma unroll
      for (uint32_t i = 0; i < E / 2; ++i) {
        ulonglong2 q;
        q.x = ent[2 * i];
        q.y = ent[2 * i + 1];
        rowp[i] = q;
      }
    }
    if (valid && j == 0) {
      const uint32_t errors = in_use + not_found + exceeded + bad_kind;
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = dead ? make_uint4(0, 0, 0, 0) : make_uint4(routed, released, errors, cnt);
      a.out_arm[k] = static_cast<uint8_t>(arm);
      acc[0] += released;
      acc[1] += in_use;
      acc[2] += not_found;
      acc[3] += exceeded;
    }
  }
  block_report<4>(a.ctr, RL_R_RELEASED, acc, flags, RL_S_FLAGS);
}

// ---- run: the route list -----------------------------------------------------------------------

// The routed indicators of positions p0 .. p0 + RL_ROWS as bits.
__device__ inline uint32_t rl_load_routed(const RlRunArgs& a, uint64_t p0, uint64_t total) {
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t j = 0; j < RL_ROWS; ++j)
    if (p0 + j < total && rl_routed(a.events[p0 + j] >> 16, a.verdicts[p0 + j])) bits |= 1u << j;
  return bits;
}

__global__ __launch_bounds__(RL_BLOCK) void rel_route_count_kernel(RlRunArgs a) {
  __shared__ uint32_t wsum[RL_WAVES];
  uint64_t m, total;
  if (!rl_run_counts(a, &m, &total)) return;
  const uint64_t tiles = rl_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t bits = rl_load_routed(a, tile * RL_TILE + static_cast<uint64_t>(threadIdx.x) * RL_ROWS, total);
    uint32_t all;
    (void)block_excl_scan<RL_BLOCK>(static_cast<uint32_t>(__popc(bits)), wsum, &all);
    if (threadIdx.x == 0) a.tile_tot[tile] = all;
  }
}

// One block: tile_tot becomes its exclusive scan, scan_chunk tiles a carry step; the sum is the
// length of the route list.
__global__ __launch_bounds__(RL_SCAN_BLOCK) void rel_route_scan_kernel(RlRunArgs a) {
  __shared__ uint32_t wsum[RL_SCAN_BLOCK / 64];
  uint64_t m, total;
  if (!rl_run_counts(a, &m, &total)) return;
  const uint32_t sum = block_scan_in_place<RL_SCAN_BLOCK>(a.tile_tot, a.tile_tot, rl_tiles(total), wsum,
                                                          scan_chunk_of<RL_SCAN_BLOCK>(a.scan_chunk));
  if (threadIdx.x == 0) a.ctr[RL_R_ROUTED] = sum;
}

__global__ __launch_bounds__(RL_BLOCK) void rel_route_place_kernel(RlRunArgs a) {
  __shared__ uint32_t wsum[RL_WAVES];
  uint64_t m, total;
  if (!rl_run_counts(a, &m, &total)) return;
  const uint64_t tiles = rl_tiles(total);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t p0 = tile * RL_TILE + static_cast<uint64_t>(threadIdx.x) * RL_ROWS;
    const uint32_t bits = rl_load_routed(a, p0, total);
    uint32_t all;
    uint32_t run = a.tile_tot[tile] + block_excl_scan<RL_BLOCK>(static_cast<uint32_t>(__popc(bits)), wsum, &all);
#pragma unroll
    for (uint32_t j = 0; j < RL_ROWS; ++j) {
      if (!((bits >> j) & 1u)) continue;  // (a set bit: p0 + j < total)
      const uint32_t g = run++;
      if (g < a.cap_in) a.out_route[g] = a.src ? a.src[p0 + j] : static_cast<uint32_t>(p0 + j);
    }
  }
}

__global__ void rel_run_finish_kernel(RlRunArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = rl_run_counts(a, &m, &total);
  s[RL_S_BOXES] = m;
  if (!go) {
    s[RL_S_FLAGS] = RL_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= RL_MAX_TOTAL) s[RL_S_TOTAL] = a.ev_offsets[m];
  } else {
    s[RL_S_TOTAL] = total;
    s[RL_S_FLAGS] = a.ctr[RL_S_FLAGS];
    for (uint32_t k = RL_R_ROUTED; k < RL_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < RL_S_WORDS; ++k) a.summary[k] = s[k];
}

// ---- expire ------------------------------------------------------------------------------------

// a.w / 2 lanes a session.  The loop is uniform over the block: the shuffles see every lane.
__global__ __launch_bounds__(RL_BLOCK) void rel_expire_kernel(RlExpArgs a) {
  uint64_t m;
  if (!rl_exp_counts(a, &m)) return;
  const uint32_t lanes = a.w / 2, per_block = RL_BLOCK / lanes;
  const uint32_t group = threadIdx.x / lanes, j = threadIdx.x % lanes;
  uint64_t acc[5] = {0, 0, 0, 0, 0};  // OK sessions, (word 2), expired, remaining, armed
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    uint64_t sub = 0;
    uint8_t st = RL_NO_SESSION;
    if (valid) {
      sub = a.subs ? a.subs[k] : k;
      const bool ok = sub < a.sub_limit;
      st = rl_expire_session(ok, ok ? a.sessions[sub * RL_REC_WORDS + RL_REC_FLAGS] : 0u, a.channel_rule != 0);
      if (j == 0 && !ok) flags |= RL_F_BAD_SUB;
    }
    uint32_t packed = 0;  // expired, remaining << 16
    if (valid && st == RL_OK) {
      const uint32_t timeout = a.timeouts ? a.timeouts[sub] : a.timeout_ms;
      ulonglong2* at = reinterpret_cast<ulonglong2*>(a.rel + sub * a.w) + j;
      ulonglong2 q = *at;
      const bool x0 = rl_expired(q.x, a.now_ms, timeout), x1 = rl_expired(q.y, a.now_ms, timeout);
      const uint32_t gone = (x0 ? 1u : 0u) + (x1 ? 1u : 0u), stay = ((!x0 && q.x != 0) ? 1u : 0u) + ((!x1 && q.y != 0) ? 1u : 0u);
      packed = gone + (stay << 16);
      if (x0 || x1) {
        if (x0) q.x = 0;
        if (x1) q.y = 0;
        *at = q;
      }
    }
    for (uint32_t d = 1; d < lanes; d <<= 1) packed += __shfl_xor(packed, d, 64);
    if (valid && j == 0) {
      const uint32_t expired = packed & 0xFFFFu, remaining = packed >> 16;
      a.out_status[k] = st;
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = make_uint4(expired, remaining, remaining > 0 ? 1u : 0u, 0u);
      acc[0] += st == RL_OK;
      acc[2] += expired;
      acc[3] += remaining;
      acc[4] += remaining > 0;
    }
  }
  block_report<5>(a.ctr, RL_X_OK, acc, flags, RL_S_FLAGS);
}

__global__ void rel_expire_finish_kernel(RlExpArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m;
  uint64_t s[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = rl_exp_counts(a, &m);
  if (!go) {
    s[RL_S_FLAGS] = RL_F_INPUT_REFUSED;
  } else {
    s[RL_S_FLAGS] = a.ctr[RL_S_FLAGS];
    s[RL_X_OK] = a.ctr[RL_X_OK];
    for (uint32_t k = RL_X_EXPIRED; k <= RL_X_ARMED; ++k) s[k] = a.ctr[k];
  }
  s[RL_S_BOXES] = m;
  for (uint32_t k = 0; k < RL_S_WORDS; ++k) a.summary[k] = s[k];
}

// The grid over `units` tiles or groups of sessions; the blocks stride beyond the cap.
uint32_t rl_grid(uint64_t units, uint32_t max_blocks) {
  const uint32_t cap = max_blocks && max_blocks < RL_MAX_BLOCKS ? max_blocks : RL_MAX_BLOCKS;
  if (units == 0) units = 1;
  return static_cast<uint32_t>(units < cap ? units : cap);
}

}  // namespace

// Enqueues the passes of one run call.
int rl_launch_run(const RlRunArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t lanes = rl_lanes(a.w, a.lanes), per_block = RL_BLOCK / lanes;
  const dim3 fold(rl_grid((a.cap_boxes + per_block - 1) / per_block, a.max_blocks)), block(RL_BLOCK);
  const dim3 tiles(rl_grid(rl_tiles(a.cap_in), a.max_blocks));
  rel_init_kernel<<<dim3(1), dim3(64), 0, s>>>(a.ctr);
  switch (a.w / lanes) {
    case 2: rel_run_fold_kernel<2><<<fold, block, 0, s>>>(a); break;
    case 4: rel_run_fold_kernel<4><<<fold, block, 0, s>>>(a); break;
    case 8: rel_run_fold_kernel<8><<<fold, block, 0, s>>>(a); break;
    case 16: rel_run_fold_kernel<16><<<fold, block, 0, s>>>(a); break;
    case 32: rel_run_fold_kernel<32><<<fold, block, 0, s>>>(a); break;
    default: return -1;  // (rl_lanes leaves no other quotient)
  }
  rel_route_count_kernel<<<tiles, block, 0, s>>>(a);
  rel_route_scan_kernel<<<dim3(1), dim3(RL_SCAN_BLOCK), 0, s>>>(a);
  rel_route_place_kernel<<<tiles, block, 0, s>>>(a);
  rel_run_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

// Enqueues the passes of one expire call.
int rl_launch_expire(const RlExpArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t per_block = RL_BLOCK / (a.w / 2);
  rel_init_kernel<<<dim3(1), dim3(64), 0, s>>>(a.ctr);
  rel_expire_kernel<<<dim3(rl_grid((a.cap_boxes + per_block - 1) / per_block, a.max_blocks)), dim3(RL_BLOCK), 0, s>>>(a);
  rel_expire_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
