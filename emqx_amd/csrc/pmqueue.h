// Shared pieces of the priority mqueue stage (include/emqx_pmqueue.h): the queue of
// a session as a few words (PqState), the step of emqx_mqueue:out/1 over them (pq_out), what an
// activation does to the order list (pq_activate) and the closed form of emqx_mqueue:in/2 over the
// candidates of one class of an inbox (pq_plan).
//
// The list of {-P, queue} of the reference is the word `order`: one nibble a position, the class
// index in it, 0xF behind the last.  The classes of a table are in descending priority, so a keysort
// of the list is the classes in ascending index, and the only exception of Erlang's term order, the
// atom `infinity` (class 0 when the table has it), is a rule about where class 0 goes: held at the
// head when it is there already, else last.  The heads and lengths of the eight class rings are two
// 64-bit words of eight bytes each (Qc <= 128), so that the fold indexes no array: no scratch.
// Everything here is __host__ __device__: the kernels (pmqueue_kernels.hip) and the host evaluator
// (pmqueue.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "mqueue.h"

#if defined(__HIPCC__)
#define PQ_UNROLL _Pragma("unroll")
#else
#define PQ_UNROLL
#endif

namespace emqx {

constexpr uint32_t PQ_F_INPUT_REFUSED = 2u, PQ_F_BAD_SUB = 4u, PQ_F_OUTPUT_FULL = 8u, PQ_F_BAD_REF = 0x10u, PQ_F_BAD_HEAD = 0x20u,
                   PQ_F_ROW_FULL = 0x40u, PQ_F_UNFIT = 0x80u, PQ_F_BAD_VERDICT = 0x100u, PQ_F_BAD_SRC = 0x200u, PQ_F_LIMITED = 0x400u;
// words of the summaries
enum {
  PQ_S_FLAGS = 0, PQ_S_TOTAL = 1, PQ_S_BOXES = 2,
  PQ_P_STORED = 3, PQ_P_EVICTED = 4, PQ_P_QDROPPED = 5, PQ_P_UNSTORED = 6, PQ_P_OKS = 7,            // put
  PQ_T_OKS = 1, PQ_T_ITEMS = 3, PQ_T_SENDS = 4, PQ_T_SENDS0 = 5, PQ_T_EXPIRED = 6, PQ_T_UNFIT = 7,  // take
  PQ_S_WORDS = 8,
  // behind the counters in the scratch: the take scan's total and its overflow decision
  PQ_C_TOTAL = 8, PQ_C_FULL = 9, PQ_C_WORDS = 10
};

constexpr uint32_t PQ_MAX_CLASSES = 8, PQ_MIN_QC = 8, PQ_MAX_QC = 128, PQ_MAX_MULT = 1024;
constexpr int32_t PQ_INFINITY = 0x7FFFFFFF, PQ_MAX_PRIO = 1000000;
constexpr uint8_t PQ_NO_CLASS = 0xFF, PQ_UNFIT = 7;
constexpr uint32_t PQ_LAST_DEFINED = 1u;
constexpr uint32_t PQ_NO_ORDER = 0xFFFFFFFFu;
constexpr uint32_t PQ_MIN_GROUP = 4, PQ_MAX_GROUP = 64, PQ_DEFAULT_GROUP = 4;
constexpr uint32_t PQ_COUNT_WORDS = 8;  // out_counts of a put: words an inbox
// the session record as eight words (emqx_window_session)
constexpr uint32_t PQ_REC_MQ_MAX = 3, PQ_REC_DROPPED = 6;

// struct emqx_pmqueue_table and struct emqx_pmqueue_head as the stage reads them
struct PqTable {
  uint32_t n_classes, default_class, max_len, mult, base, rsv;
  int32_t prio[8];
};
struct PqHead {
  uint16_t head[8], len[8];
  uint32_t order;
  int32_t credit;
  uint32_t flags, table;
  uint32_t rsv[4];
};

AK_HD inline bool pq_shape_ok(uint64_t c, uint64_t qc) {
  return c >= 1 && c <= PQ_MAX_CLASSES && qc >= PQ_MIN_QC && qc <= PQ_MAX_QC && (qc & (qc - 1)) == 0;
}
AK_HD inline bool pq_group_ok(int64_t g) { return g >= PQ_MIN_GROUP && g <= PQ_MAX_GROUP && (g & (g - 1)) == 0; }

// Whether the stage serves the sessions of this table at C classes of Qc entries.
AK_HD inline bool pq_table_fit(const PqTable* t, uint32_t C, uint32_t Qc) {
  if (t->n_classes < 1 || t->n_classes > PQ_MAX_CLASSES || t->n_classes > C || t->default_class >= t->n_classes) return false;
  if (t->max_len < 2 || t->max_len > Qc || t->mult < 1 || t->mult > PQ_MAX_MULT || t->base > static_cast<uint32_t>(PQ_MAX_PRIO)) return false;
  for (uint32_t c = 0; c < t->n_classes; ++c) {
    const int32_t p = t->prio[c];
    if (p == PQ_INFINITY) {
      if (c != 0) return false;
      continue;
    }
    if (p > PQ_MAX_PRIO || p < -PQ_MAX_PRIO) return false;
    if (c > 0 && t->prio[c - 1] != PQ_INFINITY && p >= t->prio[c - 1]) return false;
  }
  return true;
}
AK_HD inline bool pq_has_infinity(const PqTable* t) { return t->prio[0] == PQ_INFINITY; }

// get_credits/2; every negative value is -1.
AK_HD inline int32_t pq_credit(int32_t prio, uint32_t base, uint32_t mult) {
  const int64_t p = prio == PQ_INFINITY ? 1000000 : prio;
  const int64_t v = (p + static_cast<int64_t>(base) + 1) * static_cast<int64_t>(mult) - 1;
  return v < 0 ? -1 : v > 0x7FFFFFFF ? 0x7FFFFFFF : static_cast<int32_t>(v);
}

// The classes of `mask` in ascending index as an order word.
AK_HD inline uint32_t pq_sorted(uint32_t mask) {
  uint32_t order = PQ_NO_ORDER, at = 0;
  PQ_UNROLL
  for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c)
    if (mask & (1u << c)) {
      order = (order & ~(0xFu << (4 * at))) | (c << (4 * at));
      ++at;
    }
  return order;
}
// The classes an order word lists, and whether it is a list: distinct classes, then 0xF only.
AK_HD inline uint32_t pq_order_mask(uint32_t order, bool* is_list) {
  uint32_t mask = 0;
  bool ended = false, ok = true;
  PQ_UNROLL
  for (uint32_t p = 0; p < PQ_MAX_CLASSES; ++p) {
    const uint32_t nib = (order >> (4 * p)) & 0xFu;
    if (nib == 0xFu) {
      ended = true;
    } else if (ended || nib >= PQ_MAX_CLASSES || (mask & (1u << nib))) {
      ok = false;
    } else {
      mask |= 1u << nib;
    }
  }
  *is_list = ok;
  return mask;
}
// emqx_pqueue:in/3 of a class the list lacks (c is not in `order`, which has a free position).
AK_HD inline uint32_t pq_activate(uint32_t order, uint32_t c, bool has_inf) {
  if (has_inf && c == 0) return (order << 4);  // pushed at the head, no sort
  bool is_list;
  const uint32_t mask = pq_order_mask(order, &is_list) | (1u << c);
  if (!has_inf || !(mask & 1u) || (order & 0xFu) == 0u) return pq_sorted(mask);  // a head `infinity` is the smallest index
  const uint32_t rest = pq_sorted(mask & ~1u);                                   // a non-head `infinity` sorts last
  const uint32_t n = static_cast<uint32_t>(__builtin_popcount(mask & ~1u));
  return (rest & ~(0xFu << (4 * n)));  // class 0 in position n
}

// The queue of a session in registers.
struct PqState {
  uint64_t heads, lens;  // a byte a class
  uint32_t order;
  int32_t credit;
  uint32_t last;   // last_prio is defined
  uint32_t nact;   // classes in `order`
  uint32_t total;  // the sum of the lengths
  bool bad;        // the head was malformed
};
AK_HD inline uint32_t pq_len(const PqState& s, uint32_t c) { return static_cast<uint32_t>(s.lens >> (8 * c)) & 0xFFu; }
AK_HD inline uint32_t pq_head(const PqState& s, uint32_t c) { return static_cast<uint32_t>(s.heads >> (8 * c)) & 0xFFu; }

// A head as the stage reads it (the rule of include/emqx_pmqueue.h).
AK_HD inline PqState pq_load(const PqHead& hd, uint32_t n_classes, uint32_t Qc) {
  PqState s{0, 0, hd.order, hd.credit, hd.flags & PQ_LAST_DEFINED, 0, 0, false};
  uint32_t nonempty = 0;
  PQ_UNROLL
  for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
    uint32_t h = hd.head[c], l = hd.len[c];
    if (h >= Qc || l > Qc || (c >= n_classes && l != 0)) s.bad = true;
    h &= Qc - 1;
    l = c >= n_classes ? 0u : (l < Qc ? l : Qc);
    s.heads |= static_cast<uint64_t>(h) << (8 * c);
    s.lens |= static_cast<uint64_t>(l) << (8 * c);
    s.total += l;
    if (l) {
      nonempty |= 1u << c;
      ++s.nact;
    }
  }
  bool is_list;
  if (pq_order_mask(s.order, &is_list) != nonempty || !is_list) {
    s.order = pq_sorted(nonempty);
    s.bad = true;
  }
  if (s.credit < -1) {
    s.credit = -1;
    s.bad = true;
  }
  if (hd.flags & ~PQ_LAST_DEFINED) s.bad = true;
  return s;
}
AK_HD inline void pq_store(const PqState& s, PqHead* hd) {
  PQ_UNROLL
  for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
    hd->head[c] = static_cast<uint16_t>(pq_head(s, c));
    hd->len[c] = static_cast<uint16_t>(pq_len(s, c));
  }
  hd->order = s.order;
  hd->credit = s.credit;
  hd->flags = s.last;
}

// One emqx_mqueue:out/1 of a queue with total > 0: the class taken from; *pos: the ring position of
// the entry.  `prio` is the table's.
AK_HD inline uint32_t pq_out(PqState* s, const int32_t* prio, uint32_t base, uint32_t mult, uint32_t Qc, uint32_t* pos) {
  if (s->last && s->credit == 0) {  // shift: Rest ++ [Hd]
    const uint32_t hd = s->order & 0xFu, at = 4 * (s->nact - 1);
    const uint32_t rest = (s->order >> 4) | 0xF0000000u;
    s->order = (rest & ~(0xFu << at)) | (hd << at);
    s->last = 0;
  }
  const uint32_t c = s->order & 0x7u;
  if (!s->last) {
    s->last = 1;
    s->credit = pq_credit(prio[c], base, mult);
  } else if (s->credit > 0) {
    s->credit -= 1;
  }
  const uint32_t sh = 8 * c, h = static_cast<uint32_t>(s->heads >> sh) & 0xFFu;
  *pos = h;
  s->heads = (s->heads & ~(0xFFull << sh)) | (static_cast<uint64_t>((h + 1) & (Qc - 1)) << sh);
  s->lens -= 1ull << sh;
  s->total -= 1;
  if (((s->lens >> sh) & 0xFFu) == 0) {  // the head element is deleted
    s->order = (s->order >> 4) | 0xF0000000u;
    s->nact -= 1;
  }
  return c;
}

// in/2 folded over the e candidates of one class that holds L of at most M entries in a ring of Qc.
struct PqPlan {
  uint32_t qd;      // the first qd candidates are queued, then dropped
  uint32_t thr;     // a candidate of rank r >= thr evicts (PQ_NO_ORDER: none does)
  uint32_t ev;      // old entries that leave from the head
  uint32_t stored;  // candidates in the ring after the call
  uint32_t unstored;
};
AK_HD inline PqPlan pq_plan(uint32_t L, uint32_t M, uint32_t Qc, uint32_t e) {
  PqPlan p{0, PQ_NO_ORDER, 0, 0, 0};
  if (L > M) {
    const uint32_t room = Qc - L;
    p.stored = e < room ? e : room;
    p.unstored = e - p.stored;
    return p;
  }
  const uint64_t v = static_cast<uint64_t>(L) + e > M ? static_cast<uint64_t>(L) + e - M : 0;
  p.qd = e > M ? e - M : 0u;
  p.thr = M - L;
  p.ev = v < L ? static_cast<uint32_t>(v) : L;
  p.stored = e - p.qd;
  return p;
}
// The class of a delivery.
AK_HD inline uint32_t pq_class_of(const uint8_t* msg_class, uint64_t n_msgs, uint64_t n_tables, uint32_t table, uint32_t src,
                                  const PqTable* t, bool* bad_src) {
  *bad_src = src >= n_msgs;
  if (*bad_src) return t->default_class;
  const uint32_t c = msg_class[static_cast<uint64_t>(src) * n_tables + table];
  return c < t->n_classes ? c : t->default_class;
}
// Whether a verdict of the window call is one this stage ignores and flags.
AK_HD inline bool pq_bad_verdict(uint8_t v) { return mq_is_qdropped(v) || mq_evicts(v); }
AK_HD inline bool pq_candidate(uint8_t v) { return mq_is_queued(v) && !mq_evicts(v); }

// Sessions a block and trip, and the trips of m sessions or inboxes at group width g.
AK_HD inline uint64_t pq_tiles(uint64_t m, uint32_t g) { return (m + AK_BLOCK / g - 1) / (AK_BLOCK / g); }
// Words of two bits an entry (expired, QoS 0) a class: 16 ring positions a word.
AK_HD inline uint32_t pq_words(uint32_t Qc) { return Qc < 16 ? 1u : Qc / 16; }

#if defined(__HIPCC__)
struct PqPutArgs {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  const uint8_t* verdicts;
  const uint32_t* refs;
  const uint32_t* box_src;
  const uint8_t* msg_class;
  uint64_t n_msgs;
  const PqTable* tables;
  uint64_t n_tables;
  uint32_t* sessions;
  uint64_t sub_limit, update_table;
  uint2* ring;
  PqHead* heads;
  uint32_t c, qc;
  uint8_t* out_verdicts;
  uint8_t* out_class;
  uint2* out_evicted;
  uint32_t* out_counts;
  unsigned long long* ctr;  // [PQ_C_WORDS] counters, zeroed by the first kernel
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks, group;
};
struct PqTakeArgs {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes;
  uint32_t* sessions;
  uint64_t sub_limit, update_table;
  const PqTable* tables;
  uint64_t n_tables;
  const uint2* ring;
  PqHead* heads;
  uint32_t c, qc;
  uint64_t now_ms;
  const uint64_t* deadlines;
  uint64_t ref_limit, cap_out;
  uint64_t* out_offsets;
  uint8_t* out_opts;
  uint8_t* out_verdicts;
  uint16_t* out_pkt_ids;
  uint32_t* out_refs;
  uint8_t* out_class;
  uint8_t* out_status;
  uint32_t* out_counts;
  uint64_t* tile_tot;       // [pq_tiles(cap_boxes, PQ_MAX_GROUP)] items of a tile, then their exclusive scan
  unsigned long long* ctr;  // [PQ_C_WORDS]
  uint64_t* summary;
  uint32_t max_blocks, scan_chunk, group;
};
int pq_launch_put(const PqPutArgs& a, void* stream);
int pq_launch_take(const PqTakeArgs& a, void* stream);
#endif

}  // namespace emqx
