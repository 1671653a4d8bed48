// Kernels of the priority mqueue stage (include/emqx_pmqueue.h).
//
// Both calls give a group of G lanes (tuning key "group": 4..64, a power of two, so a group never
// straddles a wave) to an inbox (put) or a session (take); a block of 256 threads takes 256 / G of
// them a trip, the grid is capped by max_blocks and the blocks stride beyond it.  Every trip loop
// that holds a ballot is uniform over the wave (its condition is a ballot), every loop that holds a
// barrier is uniform over the block.
//
// Put (behind the window stage).  The candidates of an inbox are ranked WITHIN THEIR CLASS by the
// group's own ballots, G deliveries a trip: no global scan, no scratch, and an inbox that spans any
// number of tiles or holds most of a batch is walked by its one group, (deliveries / G) trips (the
// cost is in DESIGN.md §3.18).  Three walks of the inbox:
//   1  the candidates e[c] of every class and the place of its first one (the activations);
//      then the plan of every class (pq_plan) in the registers of every lane of the group;
//   2  every delivery's out_verdicts, out_class and out_evicted; the old entries are READ here;
//   3  the surviving candidates are stored into the class rings.
// THE HAZARD is mqueue's: in a full ring the survivors land on the positions of the evicted entries.
// The group is part of one wave, walk 2's loads have returned before its stores of out_evicted issue,
// and a fence stands between the walks: every read of an old entry is done before a store of walk 3.
// Lane 0 of the group then writes the head, the record and out_counts.  Inboxes name distinct
// sessions, so no two groups touch one row.
//
// Take (dequeue/1 of m sessions).  out/1 has no closed form (the class taken from depends on every
// earlier step), but a step needs only the head words and two bits an entry, expired and QoS 0:
//   A  the group's lanes read the live entries of the session's rings, 16 ring positions a lane and
//      turn, and leave their two bits in LDS, a word per 16 positions (by ring position, so nothing
//      is rotated); deadlines[] is read here;
//   B  every lane of the group runs the fold on the head words in registers (PqState: no array is
//      indexed, no scratch); a step reads one LDS word; step s is WRITTEN by lane s % G, which loads
//      the entry again (off the dependent chain) and stores the item.
//   pq_take_count_kernel  A and B without items: the consumed entries into out_offsets[k], the tile's
//                         sum into tile_tot;
//   pq_take_scan_kernel   one block: tile_tot becomes its exclusive scan; the total, the overflow
//                         decision; zeroes the counters;
//   pq_take_emit_kernel   the sessions of a tile scanned in the block; A and B again with the items;
//                         counts and status always; items, heads and records unless the call is full;
//   pq_take_finish_kernel the summary.
// A ring is only read by take; a head and a record are read and written by their session's own
// lanes, and both passes evaluate the same fold on the same bytes.
//
// Every index is bounded before use: a position < offsets[m] <= cap_in, an inbox or session index
// < m <= cap_boxes, a subscriber id < sub_limit, a table < n_tables, a class < n_classes <= C, a ring
// position masked by Qc - 1, a message < n_msgs, a ref < ref_limit, an item position < cap_out, a
// tile < pq_tiles(cap_boxes, G), an LDS word < (256 / G) * C * pq_words(Qc).
#include <hip/hip_runtime.h>

#include "pmqueue.h"

namespace emqx {

namespace {

constexpr uint32_t PQ_WAVES = AK_BLOCK / 64;

// What a call makes of a session: its status and, for AK_OK, its table and queue.
struct PqSess {
  uint64_t sub;
  const PqTable* tab;
  uint32_t table;
  uint32_t flags;  // what reading it reports
  uint8_t status;
  PqState st;
};
__device__ inline PqSess pq_session(uint64_t sub, bool valid, const uint32_t* sessions, uint64_t sub_limit, const PqHead* heads,
                                    const PqTable* tables, uint64_t n_tables, uint32_t C, uint32_t Qc) {
  PqSess s{sub, nullptr, 0, 0, AK_NO_SESSION, PqState{0, 0, PQ_NO_ORDER, 0, 0, 0, 0, false}};
  if (!valid) return s;
  const bool ok = sub < sub_limit;
  if (!ok) s.flags |= PQ_F_BAD_SUB;
  const uint32_t* rec = sessions + sub * AK_REC_WORDS;
  const uint8_t dead = ak_session(ok, ok ? rec[AK_REC_FLAGS] : 0u);
  s.status = dead ? dead : AK_OK;
  if (dead) return s;
  const PqHead hd = heads[sub];
  s.table = hd.table;
  if (s.table < n_tables) s.tab = tables + s.table;
  if (!s.tab || !pq_table_fit(s.tab, C, Qc)) {
    s.status = PQ_UNFIT;
    s.flags |= PQ_F_UNFIT;
    return s;
  }
  s.st = pq_load(hd, s.tab->n_classes, Qc);
  if (s.st.bad) s.flags |= PQ_F_BAD_HEAD;
  if (rec[PQ_REC_MQ_MAX] != 0) s.flags |= PQ_F_LIMITED;
  return s;
}

// A head's words that the stage writes; rsv stays.
__device__ inline void pq_write_head(PqHead* at, const PqState& s) {
  uint32_t w[8];
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) {
    w[c] = pq_head(s, 2 * c) | pq_head(s, 2 * c + 1) << 16;
    w[4 + c] = pq_len(s, 2 * c) | pq_len(s, 2 * c + 1) << 16;
  }
  uint4* p = reinterpret_cast<uint4*>(at);
  p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p[1] = make_uint4(w[4], w[5], w[6], w[7]);
  uint32_t* q = reinterpret_cast<uint32_t*>(at) + 8;
  q[0] = s.order;
  q[1] = static_cast<uint32_t>(s.credit);
  q[2] = s.last;
}

// The grid over `units` tiles; the blocks stride beyond the cap.
uint32_t pq_grid(uint64_t units, uint32_t max_blocks) {
  const uint32_t cap = max_blocks && max_blocks < AK_MAX_BLOCKS ? max_blocks : AK_MAX_BLOCKS;
  if (units == 0) units = 1;
  return static_cast<uint32_t>(units < cap ? units : cap);
}

// ---- put ---------------------------------------------------------------------------------------

__device__ inline bool pq_put_counts(const PqPutArgs& a, uint64_t* m, uint64_t* total) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  *total = 0;
  if (*m > a.cap_boxes || *m > AK_MAX_TOTAL) return false;
  *total = a.inbox_offsets[*m];
  return *total <= a.cap_in && *total <= AK_MAX_TOTAL;
}

__global__ void pq_zero_kernel(unsigned long long* ctr) {
  if (blockIdx.x == 0 && threadIdx.x < PQ_C_WORDS) ctr[threadIdx.x] = 0;
}

__global__ __launch_bounds__(AK_BLOCK) void pq_put_kernel(PqPutArgs a) {
  uint64_t m, total;
  if (!pq_put_counts(a, &m, &total)) return;
  const uint32_t G = a.group, per_block = AK_BLOCK / G, Qc = a.qc, qm = Qc - 1;
  const uint32_t group = threadIdx.x / G, j = threadIdx.x % G, lane0 = (threadIdx.x & 63u) - j;
  const uint64_t gmask = G == 64 ? ~0ull : (1ull << G) - 1ull, below = (1ull << j) - 1ull;
  uint64_t acc[5] = {0, 0, 0, 0, 0};  // stored, evicted, dropped in batch, unstored, OK inboxes
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const PqSess s = pq_session(valid ? a.inbox_subs[k] : 0, valid, a.sessions, a.sub_limit, a.heads, a.tables, a.n_tables, a.c, Qc);
    flags |= s.flags;
    const bool ok = valid && s.status == AK_OK;
    uint64_t lo = 0, hi = 0;
    if (valid) {
      const uint64_t o0 = a.inbox_offsets[k], o1 = a.inbox_offsets[k + 1];
      lo = o0 < total ? o0 : total;
      hi = o1 < total ? o1 : total;
      if (hi < lo) hi = lo;
    }
    const uint64_t n = hi - lo;
    const uint2* rows = a.ring + (ok ? s.sub * a.c * Qc : 0);
    // whether delivery lo + i of an OK inbox is a candidate, and its class (8: none)
    auto look = [&](uint64_t i, uint32_t* cls) {
      *cls = PQ_MAX_CLASSES;
      if (!ok || i >= n) return false;
      const uint8_t v = a.verdicts[lo + i];
      if (pq_bad_verdict(v)) flags |= PQ_F_BAD_VERDICT;
      if (!pq_candidate(v)) return false;
      bool bad_src;
      *cls = pq_class_of(a.msg_class, a.n_msgs, a.n_tables, s.table, a.box_src[lo + i], s.tab, &bad_src);
      if (bad_src) flags |= PQ_F_BAD_SRC;
      return true;
    };
    // walk 1: the candidates of every class and the place of its first one
    uint32_t e[PQ_MAX_CLASSES], first[PQ_MAX_CLASSES];
#pragma unroll
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) e[c] = first[c] = 0;
    for (uint64_t t = 0; __ballot(ok && t * G < n) != 0; ++t) {
      uint32_t cls;
      const bool cand = look(t * G + j, &cls);
#pragma unroll
      for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
        const uint64_t b = (__ballot(cand && cls == c) >> lane0) & gmask;
        if (b) {
          if (!e[c]) first[c] = static_cast<uint32_t>(t * G) + static_cast<uint32_t>(__builtin_ctzll(b));
          e[c] += static_cast<uint32_t>(__builtin_popcountll(b));
        }
      }
    }
    const uint32_t M = ok ? s.tab->max_len : 2u;
    PqPlan plan[PQ_MAX_CLASSES];
#pragma unroll
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) plan[c] = pq_plan(pq_len(s.st, c), M, Qc, e[c]);
    // walk 2: the outputs of every delivery; the old entries are read here
    uint32_t run[PQ_MAX_CLASSES];
#pragma unroll
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) run[c] = 0;
    for (uint64_t t = 0; __ballot(valid && t * G < n) != 0; ++t) {
      const uint64_t i = t * G + j;
      uint32_t cls;
      const bool cand = look(i, &cls);
      uint8_t verdict = 0;
      uint2 old = make_uint2(MQ_NO_REF, 0u);
#pragma unroll
      for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
        const uint64_t b = (__ballot(cand && cls == c) >> lane0) & gmask;
        if (cand && cls == c) {
          const uint32_t r = run[c] + static_cast<uint32_t>(__builtin_popcountll(b & below));
          const bool evicts = plan[c].thr != PQ_NO_ORDER && r >= plan[c].thr;
          verdict = static_cast<uint8_t>((r < plan[c].qd ? WN_QUEUED_DROPPED : WN_QUEUED) | (evicts ? WN_EVICTS : 0));
          if (evicts && r - plan[c].thr < pq_len(s.st, c)) old = rows[c * Qc + ((pq_head(s.st, c) + r - plan[c].thr) & qm)];
        }
        run[c] += static_cast<uint32_t>(__builtin_popcountll(b));
      }
      if (valid && i < n) {
        a.out_verdicts[lo + i] = verdict;
        a.out_class[lo + i] = cand ? static_cast<uint8_t>(cls) : PQ_NO_CLASS;
        a.out_evicted[lo + i] = old;
      }
    }
    __threadfence_block();  // every old entry is read before the first store into a ring
    // walk 3: the survivors into the rings
#pragma unroll
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) run[c] = 0;
    for (uint64_t t = 0; __ballot(ok && t * G < n) != 0; ++t) {
      const uint64_t i = t * G + j;
      uint32_t cls;
      const bool cand = look(i, &cls);
#pragma unroll
      for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
        const uint64_t b = (__ballot(cand && cls == c) >> lane0) & gmask;
        if (cand && cls == c) {
          const uint32_t r = run[c] + static_cast<uint32_t>(__builtin_popcountll(b & below));
          if (r >= plan[c].qd && r - plan[c].qd < plan[c].stored) {
            const uint64_t d = lo + i;
            a.ring[s.sub * a.c * Qc + c * Qc + ((pq_head(s.st, c) + pq_len(s.st, c) + (r - plan[c].qd)) & qm)] =
                make_uint2(a.refs ? a.refs[d] : static_cast<uint32_t>(d), mq_word1(a.box_opts[d]));
          }
        }
        run[c] += static_cast<uint32_t>(__builtin_popcountll(b));
      }
    }
    // lane 0 of the group: the activations in arrival order, the head, the record, the counts
    if (valid && j == 0) {
      uint4 c0 = make_uint4(0, 0, 0, 0), c1 = make_uint4(0, 0, 0, s.status);
      if (ok) {
        PqState nst = s.st;
        const bool has_inf = pq_has_infinity(s.tab);
        uint32_t pending = 0;
#pragma unroll
        for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c)
          if (e[c] && pq_len(s.st, c) == 0) pending |= 1u << c;
        while (pending) {  // (the first places of two classes differ)
          uint32_t best = 0, best_first = 0xFFFFFFFFu;
#pragma unroll
          for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c)
            if ((pending & (1u << c)) && first[c] < best_first) {
              best = c;
              best_first = first[c];
            }
          nst.order = pq_activate(nst.order, best, has_inf);
          pending &= ~(1u << best);
        }
        nst.heads = nst.lens = 0;
        nst.total = 0;
        uint64_t dropped = 0;
#pragma unroll
        for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
          const uint32_t len = pq_len(s.st, c) - plan[c].ev + plan[c].stored;
          nst.heads |= static_cast<uint64_t>((pq_head(s.st, c) + plan[c].ev) & qm) << (8 * c);
          nst.lens |= static_cast<uint64_t>(len) << (8 * c);
          nst.total += len;
          c0.x += plan[c].stored;
          c0.y += plan[c].ev;
          c0.z += plan[c].qd;
          c0.w += plan[c].unstored;
          dropped += static_cast<uint64_t>(plan[c].ev) + plan[c].qd;
        }
        uint32_t* rec = a.sessions + s.sub * AK_REC_WORDS;
        const uint64_t after = (static_cast<uint64_t>(rec[PQ_REC_DROPPED + 1]) << 32 | rec[PQ_REC_DROPPED]) + dropped;
        c1 = make_uint4(nst.total, static_cast<uint32_t>(after), static_cast<uint32_t>(after >> 32), AK_OK);
        acc[0] += c0.x;
        acc[1] += c0.y;
        acc[2] += c0.z;
        acc[3] += c0.w;
        acc[4] += 1;
        if (c0.w) flags |= PQ_F_ROW_FULL;
        if (a.update_table) {
          pq_write_head(a.heads + s.sub, nst);
          rec[MQ_REC_MQ_LEN] = nst.total;
          rec[PQ_REC_DROPPED] = static_cast<uint32_t>(after);
          rec[PQ_REC_DROPPED + 1] = static_cast<uint32_t>(after >> 32);
        }
      }
      uint4* out = reinterpret_cast<uint4*>(a.out_counts + PQ_COUNT_WORDS * k);
      out[0] = c0;
      out[1] = c1;
    }
  }
  block_report<5>(a.ctr, PQ_P_STORED, acc, flags, PQ_S_FLAGS);
}

__global__ void pq_put_finish_kernel(PqPutArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m, total;
  uint64_t s[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = pq_put_counts(a, &m, &total);
  s[PQ_S_BOXES] = m;
  if (!go) {
    s[PQ_S_FLAGS] = PQ_F_INPUT_REFUSED;
    if (m <= a.cap_boxes && m <= AK_MAX_TOTAL) s[PQ_S_TOTAL] = a.inbox_offsets[m];
  } else {
    s[PQ_S_TOTAL] = total;
    s[PQ_S_FLAGS] = a.ctr[PQ_S_FLAGS];
    for (uint32_t k = PQ_P_STORED; k < PQ_S_WORDS; ++k) s[k] = a.ctr[k];
  }
  for (uint32_t k = 0; k < PQ_S_WORDS; ++k) a.summary[k] = s[k];
}

// ---- take --------------------------------------------------------------------------------------

__device__ inline bool pq_take_count(const PqTakeArgs& a, uint64_t* m) {
  *m = a.n_boxes ? *a.n_boxes : a.m;
  return *m <= a.cap_boxes && *m <= AK_MAX_TOTAL && (a.subs || *m <= a.sub_limit);
}

// Part A: the two bits of every live entry of the group's session into its LDS words.  No barrier.
__device__ inline void pq_take_bits(const PqTakeArgs& a, const PqSess& s, bool ok, uint32_t G, uint32_t j, uint32_t* bits) {
  const uint32_t Qc = a.qc, qm = Qc - 1, W = pq_words(Qc), per = Qc < 16 ? Qc : 16u;
  for (uint32_t it = j; it < a.c * W; it += G) {
    const uint32_t c = it / W, w = it % W;
    uint32_t word = 0;
    if (ok && c < s.tab->n_classes) {
      const uint32_t h = pq_head(s.st, c), L = pq_len(s.st, c);
      const uint2* row = a.ring + (s.sub * a.c + c) * Qc;
      for (uint32_t p = 0; p < per; ++p) {
        const uint32_t pos = 16 * w + p;
        if (((pos - h) & qm) >= L) continue;
        const uint2 en = row[pos];
        bool bad_ref;
        const bool expired = mq_expired(en.x, a.now_ms, a.deadlines, a.ref_limit, &bad_ref);
        word |= ((expired ? 1u : 0u) | ((en.y & AK_O_QOS) == 0 ? 2u : 0u)) << (2 * p);
      }
    }
    bits[it] = word;
  }
}

struct PqFound {
  PqState after;
  uint32_t items, sends, sends0, expired, flags;
};

// Part B: the fold, in every lane of the group.  EMIT: step s is written by lane s % G at off + s
// unless the call is full.
template <bool EMIT>
__device__ inline PqFound pq_take_fold(const PqTakeArgs& a, const PqSess& s, bool ok, uint32_t n, uint32_t next_pkt, uint32_t G, uint32_t j,
                                       const uint32_t* bits, uint64_t off, bool full) {
  PqFound f{s.st, 0, 0, 0, 0, 0};
  if (!ok) return f;
  const uint32_t Qc = a.qc, W = pq_words(Qc), base = s.tab->base, mult = s.tab->mult;
  const uint2* rows = a.ring + s.sub * a.c * Qc;
  while (n > 0 && f.after.total > 0) {
    uint32_t pos;
    const uint32_t c = pq_out(&f.after, s.tab->prio, base, mult, Qc, &pos);
    const uint32_t two = (bits[c * W + (pos >> 4)] >> (2 * (pos & 15u))) & 3u;
    if (EMIT && f.items % G == j) {
      const uint2 en = rows[c * Qc + pos];
      if (a.deadlines && en.x >= a.ref_limit) f.flags |= PQ_F_BAD_REF;
      const uint64_t at = off + f.items;
      if (!full && at < a.cap_out) {
        uint16_t id;
        const uint8_t verdict = mq_item(static_cast<uint8_t>(en.y), (two & 1u) != 0, next_pkt, f.sends, &id);
        a.out_opts[at] = static_cast<uint8_t>(en.y);
        a.out_verdicts[at] = verdict;
        a.out_pkt_ids[at] = id;
        a.out_refs[at] = en.x;
        a.out_class[at] = static_cast<uint8_t>(c);
      }
    }
    f.items += 1;
    if (two == 0) {
      f.sends += 1;
      n -= 1;
    } else if (two & 1u) {
      f.expired += 1;
    } else {
      f.sends0 += 1;
    }
  }
  return f;
}

__global__ __launch_bounds__(AK_BLOCK) void pq_take_count_kernel(PqTakeArgs a) {
  __shared__ uint32_t wsum[PQ_WAVES];
  uint64_t m;
  if (!pq_take_count(a, &m)) return;
  const uint32_t G = a.group, per_block = AK_BLOCK / G;
  const uint32_t group = threadIdx.x / G, j = threadIdx.x % G;
  extern __shared__ uint32_t pq_bits[];  // [256 / G][C][pq_words(Qc)]: two bits a ring position
  uint32_t* bits = pq_bits + group * a.c * pq_words(a.qc);
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const PqSess s = pq_session(valid ? (a.subs ? a.subs[k] : k) : 0, valid, a.sessions, a.sub_limit, a.heads, a.tables, a.n_tables, a.c, a.qc);
    const bool ok = valid && s.status == AK_OK;
    const uint32_t* rec = a.sessions + s.sub * AK_REC_WORDS;
    const uint32_t n = ok ? mq_budget(rec[AK_REC_INFLIGHT_MAX], rec[AK_REC_INFLIGHT]) : 0u;
    pq_take_bits(a, s, ok, G, j, bits);
    __syncthreads();
    const PqFound f = pq_take_fold<false>(a, s, ok, n, 0, G, j, bits, 0, true);
    if (valid && j == 0) a.out_offsets[k] = f.items;  // (the emit pass turns the counts into offsets)
    const uint32_t c = wave_sum(j == 0 ? f.items : 0u);
    __syncthreads();  // the readers of the trip before are done, and this trip's readers of the bits
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
      for (uint32_t w = 0; w < PQ_WAVES; ++w) all += wsum[w];
      a.tile_tot[base / per_block] = all;  // (base < m <= cap_boxes: a tile of the scratch)
    }
  }
}

// One block: tile_tot becomes its exclusive scan, scan_chunk tiles a carry step.
__global__ __launch_bounds__(AK_SCAN_BLOCK) void pq_take_scan_kernel(PqTakeArgs a) {
  __shared__ uint64_t wsum[AK_SCAN_BLOCK / 64];
  if (threadIdx.x < PQ_C_WORDS) a.ctr[threadIdx.x] = 0;
  uint64_t m;
  if (!pq_take_count(a, &m)) return;
  const uint64_t total = block_scan_in_place<AK_SCAN_BLOCK>(a.tile_tot, a.tile_tot, pq_tiles(m, a.group), wsum,
                                                            scan_chunk_of<AK_SCAN_BLOCK>(a.scan_chunk));
  __syncthreads();  // the zeroing above
  if (threadIdx.x == 0) {
    a.ctr[PQ_C_TOTAL] = total;
    a.ctr[PQ_C_FULL] = total > a.cap_out ? 1ull : 0ull;
    a.out_offsets[m] = total;
  }
}

__global__ __launch_bounds__(AK_BLOCK) void pq_take_emit_kernel(PqTakeArgs a) {
  __shared__ uint32_t wsum[PQ_WAVES];
  uint64_t m;
  if (!pq_take_count(a, &m)) return;
  const bool full = a.ctr[PQ_C_FULL] != 0;
  const uint32_t G = a.group, per_block = AK_BLOCK / G;
  const uint32_t group = threadIdx.x / G, j = threadIdx.x % G, lane0 = (threadIdx.x & 63u) - j;
  extern __shared__ uint32_t pq_bits[];  // as in the count pass
  uint32_t* bits = pq_bits + group * a.c * pq_words(a.qc);
  uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};  // OK sessions, -, -, sends, sends QoS 0, expired, unfit sessions
  uint32_t flags = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * per_block; base < m; base += static_cast<uint64_t>(gridDim.x) * per_block) {
    const uint64_t k = base + group;
    const bool valid = k < m;
    const PqSess s = pq_session(valid ? (a.subs ? a.subs[k] : k) : 0, valid, a.sessions, a.sub_limit, a.heads, a.tables, a.n_tables, a.c, a.qc);
    const bool ok = valid && s.status == AK_OK;
    uint32_t* rec = a.sessions + s.sub * AK_REC_WORDS;
    const uint32_t inflight = ok ? rec[AK_REC_INFLIGHT] : 0u, next_pkt = ok ? rec[MQ_REC_NEXT_PKT] : 1u;
    const uint32_t n = ok ? mq_budget(rec[AK_REC_INFLIGHT_MAX], inflight) : 0u;
    const uint32_t counted = (valid && j == 0) ? static_cast<uint32_t>(a.out_offsets[k]) : 0u;  // (the count pass's)
    uint32_t tile_items;  // (not used: the scan kernel has the tile's base)
    const uint32_t pre = block_excl_scan<AK_BLOCK>(counted, wsum, &tile_items);  // (its barriers: the readers of the bits are done)
    const uint64_t off = a.tile_tot[base / per_block] + __shfl(pre, lane0, 64);
    pq_take_bits(a, s, ok, G, j, bits);
    __syncthreads();
    const PqFound f = pq_take_fold<true>(a, s, ok, n, next_pkt, G, j, bits, off, full);
    flags |= f.flags;
    if (valid && j == 0) {
      flags |= s.flags;
      uint4 counts = make_uint4(0, 0, 0, 0);
      if (s.status == PQ_UNFIT) acc[6] += 1;
      if (ok) {
        counts = make_uint4(f.sends, f.sends0, f.expired, f.after.total);
        acc[0] += 1;
        acc[3] += f.sends;
        acc[4] += f.sends0;
        acc[5] += f.expired;
        if (a.update_table && !full) {
          pq_write_head(a.heads + s.sub, f.after);
          rec[MQ_REC_MQ_LEN] = f.after.total;
          if (f.sends) {
            rec[AK_REC_INFLIGHT] = wn_sat32(static_cast<uint64_t>(inflight) + f.sends);
            rec[MQ_REC_NEXT_PKT] = mq_next_pkt(next_pkt, f.sends);
          }
        }
      }
      a.out_offsets[k] = off;
      a.out_status[k] = s.status;
      *reinterpret_cast<uint4*>(a.out_counts + 4 * k) = counts;
    }
  }
  block_report<7>(a.ctr, PQ_T_OKS, acc, flags, PQ_S_FLAGS);
}

__global__ void pq_take_finish_kernel(PqTakeArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t m;
  uint64_t s[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool go = pq_take_count(a, &m);
  if (!go) {
    s[PQ_S_FLAGS] = PQ_F_INPUT_REFUSED;
  } else {
    for (uint32_t k = 0; k < PQ_S_WORDS; ++k) s[k] = a.ctr[k];
    s[PQ_T_ITEMS] = a.ctr[PQ_C_TOTAL];
    if (a.ctr[PQ_C_FULL]) s[PQ_S_FLAGS] |= PQ_F_OUTPUT_FULL;
  }
  s[PQ_S_BOXES] = m;
  for (uint32_t k = 0; k < PQ_S_WORDS; ++k) a.summary[k] = s[k];
}

}  // namespace

// Enqueues the passes of one put call.
int pq_launch_put(const PqPutArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t rows = pq_grid(pq_tiles(a.cap_boxes, a.group), a.max_blocks);
  pq_zero_kernel<<<dim3(1), dim3(64), 0, s>>>(a.ctr);
  pq_put_kernel<<<dim3(rows), dim3(AK_BLOCK), 0, s>>>(a);
  pq_put_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

// Enqueues the passes of one take call.
int pq_launch_take(const PqTakeArgs& a, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t rows = pq_grid(pq_tiles(a.cap_boxes, a.group), a.max_blocks);
  const uint32_t lds = (AK_BLOCK / a.group) * a.c * pq_words(a.qc) * sizeof(uint32_t);
  pq_take_count_kernel<<<dim3(rows), dim3(AK_BLOCK), lds, s>>>(a);
  pq_take_scan_kernel<<<dim3(1), dim3(AK_SCAN_BLOCK), 0, s>>>(a);
  pq_take_emit_kernel<<<dim3(rows), dim3(AK_BLOCK), lds, s>>>(a);
  pq_take_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
