// C ABI of the priority mqueue stage (include/emqx_pmqueue.h): the handle and its device scratch,
// the device entry points of both calls and the host evaluators.  The state, the step of out/1 and
// the closed form of in/2 live in pmqueue.h and are the same code on both sides.  With
// EMQX_PMQUEUE_NO_DEVICE this file compiles with a plain C++ compiler into the host-only part
// (tests/c/test_pmqueue_host.cpp): handles of device EMQX_PMQUEUE_HOST_ONLY alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_PMQUEUE_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/emqx_pmqueue.h"
#include "pmqueue.h"
#include "stage_host.h"

using namespace emqx;

static_assert(PQ_F_INPUT_REFUSED == EMQX_PMQ_F_INPUT_REFUSED && PQ_F_BAD_SUB == EMQX_PMQ_F_BAD_SUB &&
                  PQ_F_OUTPUT_FULL == EMQX_PMQ_F_OUTPUT_FULL && PQ_F_BAD_REF == EMQX_PMQ_F_BAD_REF && PQ_F_BAD_HEAD == EMQX_PMQ_F_BAD_HEAD &&
                  PQ_F_ROW_FULL == EMQX_PMQ_F_ROW_FULL && PQ_F_UNFIT == EMQX_PMQ_F_UNFIT && PQ_F_BAD_VERDICT == EMQX_PMQ_F_BAD_VERDICT &&
                  PQ_F_BAD_SRC == EMQX_PMQ_F_BAD_SRC && PQ_F_LIMITED == EMQX_PMQ_F_LIMITED && PQ_S_WORDS == EMQX_PMQ_SUMMARY_WORDS,
              "flags");
static_assert(PQ_MAX_CLASSES == EMQX_PMQ_MAX_CLASSES && PQ_MIN_QC == EMQX_PMQ_MIN_QC && PQ_MAX_QC == EMQX_PMQ_MAX_QC &&
                  PQ_INFINITY == EMQX_PMQ_PRIO_INFINITY && PQ_MAX_PRIO == EMQX_PMQ_MAX_PRIO && PQ_MAX_MULT == EMQX_PMQ_MAX_MULT &&
                  PQ_NO_CLASS == EMQX_PMQ_NO_CLASS && PQ_UNFIT == EMQX_PMQ_UNFIT && PQ_LAST_DEFINED == EMQX_PMQ_H_LAST_DEFINED &&
                  PQ_UNFIT != AK_OK && PQ_UNFIT != AK_NO_SESSION && PQ_UNFIT != AK_PASS,
              "constants");
static_assert(sizeof(emqx_pmqueue_table) == sizeof(PqTable) && sizeof(PqTable) == 56 && offsetof(emqx_pmqueue_table, prio) == offsetof(PqTable, prio) &&
                  sizeof(emqx_pmqueue_head) == sizeof(PqHead) && sizeof(PqHead) == 64 && offsetof(emqx_pmqueue_head, order) == 32 &&
                  offsetof(PqHead, order) == 32 && offsetof(emqx_pmqueue_head, table) == offsetof(PqHead, table) &&
                  offsetof(emqx_window_session, mq_max) == 4 * PQ_REC_MQ_MAX && offsetof(emqx_window_session, dropped) == 4 * PQ_REC_DROPPED,
              "layout");

static_assert(EMQX_PMQUEUE_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_pmqueue : StageHandle {  // (stage_host.h)
  int64_t max_blocks = AK_MAX_BLOCKS, scan_chunk = AK_SCAN_BLOCK, group = PQ_DEFAULT_GROUP;
  uint64_t cap_in = 0, cap_boxes = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What every form requires of its argument block, whichever memory it points into.
bool batch_ok(const emqx_pmqueue_put_args* b) {
  if (!b || !pq_shape_ok(b->c, b->qc)) return false;
  if (b->cap_in > AK_MAX_TOTAL || b->cap_boxes > AK_MAX_TOTAL || b->sub_limit > MAX_SUB_LIMIT || b->n_tables > AK_MAX_TOTAL ||
      b->n_msgs > AK_MAX_TOTAL)
    return false;
  if (!b->n_boxes && b->m > b->cap_boxes) return false;
  if (!b->inbox_offsets) return false;
  if (b->cap_boxes && (!b->inbox_subs || !b->out_counts)) return false;
  if (b->cap_in && (!b->box_opts || !b->verdicts || !b->box_src || !b->out_verdicts || !b->out_class || !b->out_evicted)) return false;
  if (b->n_msgs && b->n_tables && !b->msg_class) return false;
  if (b->n_tables && !b->tables) return false;
  if (b->sub_limit && (!b->sessions || !b->ring || !b->heads)) return false;
  return true;
}
bool batch_ok(const emqx_pmqueue_take_args* b) {
  if (!b || !pq_shape_ok(b->c, b->qc) || b->now_ms >= MQ_MAX_NOW) return false;
  if (b->cap_boxes > AK_MAX_TOTAL || b->sub_limit > MAX_SUB_LIMIT || b->n_tables > AK_MAX_TOTAL ||
      b->cap_out > AK_MAX_TOTAL * PQ_MAX_QC * PQ_MAX_CLASSES)
    return false;
  if (!b->n_boxes && b->m > b->cap_boxes) return false;
  if (b->n_tables && !b->tables) return false;
  if (b->sub_limit && (!b->sessions || !b->ring || !b->heads)) return false;
  if (!b->out_offsets) return false;
  if (b->cap_out && (!b->out_opts || !b->out_verdicts || !b->out_pkt_ids || !b->out_refs || !b->out_class)) return false;
  if (b->cap_boxes && (!b->out_status || !b->out_counts)) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, PQ_S_WORDS * sizeof(uint64_t));
  if (sum[PQ_S_FLAGS] & PQ_F_INPUT_REFUSED) return EMQX_EINVAL;
  if (sum[PQ_S_FLAGS] & PQ_F_OUTPUT_FULL) return EMQX_EOVERFLOW;
  return (sum[PQ_S_FLAGS] & PQ_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.
bool refused(const emqx_pmqueue_put_args* b, uint64_t m, uint64_t* total, uint64_t* sum) {
  *total = 0;
  sum[PQ_S_BOXES] = m;
  if (m <= b->cap_boxes && m <= AK_MAX_TOTAL) {
    *total = b->inbox_offsets[m];
    sum[PQ_S_TOTAL] = *total;
    if (*total <= b->cap_in && *total <= AK_MAX_TOTAL) return false;
  }
  sum[PQ_S_FLAGS] = PQ_F_INPUT_REFUSED;
  return true;
}
bool refused(const emqx_pmqueue_take_args* b, uint64_t m, uint64_t* sum) {
  sum[PQ_S_BOXES] = m;
  if (m <= b->cap_boxes && m <= AK_MAX_TOTAL && (b->subs || m <= b->sub_limit)) return false;
  sum[PQ_S_FLAGS] = PQ_F_INPUT_REFUSED;
  return true;
}

// ---- the host evaluators -----------------------------------------------------------------------

const emqx_mqueue_entry NO_ENTRY = {MQ_NO_REF, 0, {0, 0, 0}};

// What a call makes of the session `sub` names: its status, and for EMQX_A_OK its table and state.
struct Sess {
  uint8_t status;
  const PqTable* tab;
  uint32_t table;
  PqState st;
};
template <class B>
Sess session_of(const B* b, uint64_t sub, uint64_t* sum) {
  Sess s{AK_OK, nullptr, 0, PqState{}};
  const bool ok = sub < b->sub_limit;
  if (!ok) sum[PQ_S_FLAGS] |= PQ_F_BAD_SUB;
  const uint8_t dead = ak_session(ok, ok ? b->sessions[sub].flags : 0u);
  if (dead) {
    s.status = dead;
    return s;
  }
  const PqHead* hd = reinterpret_cast<const PqHead*>(b->heads + sub);
  s.table = hd->table;
  s.tab = s.table < b->n_tables ? reinterpret_cast<const PqTable*>(b->tables + s.table) : nullptr;
  if (!s.tab || !pq_table_fit(s.tab, static_cast<uint32_t>(b->c), static_cast<uint32_t>(b->qc))) {
    s.status = PQ_UNFIT;
    sum[PQ_S_FLAGS] |= PQ_F_UNFIT;
    return s;
  }
  s.st = pq_load(*hd, s.tab->n_classes, static_cast<uint32_t>(b->qc));
  if (s.st.bad) sum[PQ_S_FLAGS] |= PQ_F_BAD_HEAD;
  if (b->sessions[sub].mq_max != 0) sum[PQ_S_FLAGS] |= PQ_F_LIMITED;
  return s;
}

int put_host(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t total;
  if (refused(b, m, &total, sum)) return status_of(sum, summary_out);
  const uint32_t C = static_cast<uint32_t>(b->c), Qc = static_cast<uint32_t>(b->qc), qm = Qc - 1;
  for (uint64_t d = 0; d < total; ++d) {
    b->out_verdicts[d] = 0;
    b->out_class[d] = PQ_NO_CLASS;
    b->out_evicted[d] = NO_ENTRY;
  }
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = b->inbox_subs[k];
    const uint64_t lo = std::min(b->inbox_offsets[k], total), hi = std::max(lo, std::min(b->inbox_offsets[k + 1], total));
    uint32_t* counts = b->out_counts + PQ_COUNT_WORDS * k;
    std::memset(counts, 0, PQ_COUNT_WORDS * sizeof(uint32_t));
    Sess s = session_of(b, sub, sum);
    counts[7] = s.status;
    if (s.status != AK_OK) continue;
    sum[PQ_P_OKS] += 1;
    const PqTable* t = s.tab;
    emqx_mqueue_entry* rows = b->ring + sub * C * Qc;
    auto class_of = [&](uint64_t d) {
      bool bad_src;
      const uint32_t c = pq_class_of(b->msg_class, b->n_msgs, b->n_tables, s.table, b->box_src[d], t, &bad_src);
      if (bad_src) sum[PQ_S_FLAGS] |= PQ_F_BAD_SRC;
      return c;
    };
    // the candidates of every class and where its first one stands
    uint32_t e[PQ_MAX_CLASSES] = {}, run[PQ_MAX_CLASSES] = {};
    uint64_t first[PQ_MAX_CLASSES] = {};
    for (uint64_t d = lo; d < hi; ++d) {
      if (pq_bad_verdict(b->verdicts[d])) sum[PQ_S_FLAGS] |= PQ_F_BAD_VERDICT;
      if (!pq_candidate(b->verdicts[d])) continue;
      const uint32_t c = class_of(d);
      if (!e[c]++) first[c] = d;
    }
    PqPlan plan[PQ_MAX_CLASSES];
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) plan[c] = pq_plan(pq_len(s.st, c), t->max_len, Qc, e[c]);
    // every read of an old entry stands in front of the stores: with a full ring they share positions
    for (uint64_t d = lo; d < hi; ++d) {
      if (!pq_candidate(b->verdicts[d])) continue;
      const uint32_t c = class_of(d), r = run[c]++;
      const PqPlan& p = plan[c];
      const bool evicts = p.thr != PQ_NO_ORDER && r >= p.thr;
      b->out_verdicts[d] = static_cast<uint8_t>((r < p.qd ? WN_QUEUED_DROPPED : WN_QUEUED) | (evicts ? WN_EVICTS : 0));
      b->out_class[d] = static_cast<uint8_t>(c);
      if (evicts && r - p.thr < pq_len(s.st, c)) b->out_evicted[d] = rows[c * Qc + ((pq_head(s.st, c) + r - p.thr) & qm)];
    }
    std::memset(run, 0, sizeof(run));
    for (uint64_t d = lo; d < hi; ++d) {
      if (!pq_candidate(b->verdicts[d])) continue;
      const uint32_t c = class_of(d), r = run[c]++;
      const PqPlan& p = plan[c];
      if (r < p.qd || r - p.qd >= p.stored) continue;
      emqx_mqueue_entry& en = rows[c * Qc + ((pq_head(s.st, c) + pq_len(s.st, c) + (r - p.qd)) & qm)];
      en.ref = b->refs ? b->refs[d] : static_cast<uint32_t>(d);
      en.opts = b->box_opts[d];
      en.rsv[0] = en.rsv[1] = en.rsv[2] = 0;
    }
    // the activations in arrival order, then the rings' headers
    PqState n = s.st;
    for (;;) {
      uint32_t best = PQ_MAX_CLASSES;
      for (uint32_t c = 0; c < t->n_classes; ++c)
        if (e[c] && pq_len(n, c) == 0 && (best == PQ_MAX_CLASSES || first[c] < first[best])) best = c;
      if (best == PQ_MAX_CLASSES) break;
      n.order = pq_activate(n.order, best, pq_has_infinity(t));
      n.lens |= 1ull << (8 * best);  // (a mark; the length follows)
    }
    n.heads = n.lens = 0;
    n.total = 0;
    uint64_t dropped = 0;
    for (uint32_t c = 0; c < PQ_MAX_CLASSES; ++c) {
      const PqPlan& p = plan[c];
      const uint32_t len = pq_len(s.st, c) - p.ev + p.stored;
      n.heads |= static_cast<uint64_t>((pq_head(s.st, c) + p.ev) & qm) << (8 * c);
      n.lens |= static_cast<uint64_t>(len) << (8 * c);
      n.total += len;
      counts[0] += p.stored;
      counts[1] += p.ev;
      counts[2] += p.qd;
      counts[3] += p.unstored;
      dropped += static_cast<uint64_t>(p.ev) + p.qd;
    }
    emqx_window_session& rec = b->sessions[sub];
    const uint64_t dropped_after = rec.dropped + dropped;
    counts[4] = n.total;
    counts[5] = static_cast<uint32_t>(dropped_after);
    counts[6] = static_cast<uint32_t>(dropped_after >> 32);
    sum[PQ_P_STORED] += counts[0];
    sum[PQ_P_EVICTED] += counts[1];
    sum[PQ_P_QDROPPED] += counts[2];
    sum[PQ_P_UNSTORED] += counts[3];
    if (counts[3]) sum[PQ_S_FLAGS] |= PQ_F_ROW_FULL;
    if (!b->update_table) continue;
    pq_store(n, reinterpret_cast<PqHead*>(b->heads + sub));
    rec.mq_len = n.total;
    rec.dropped = dropped_after;
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

int take_host(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  const uint32_t C = static_cast<uint32_t>(b->c), Qc = static_cast<uint32_t>(b->qc);
  uint64_t scratch_sum[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};  // (the emit pass reports)
  // One consumed entry after the other: f(step, class, entry, expired, before, bad_ref); returns the state after.
  auto fold = [&](const Sess& s, uint64_t sub, auto&& f) {
    PqState st = s.st;
    const emqx_window_session& rec = b->sessions[sub];
    uint32_t n = mq_budget(rec.inflight_max, rec.inflight), before = 0, step = 0;
    while (n > 0 && st.total > 0) {
      uint32_t pos;
      const uint32_t c = pq_out(&st, s.tab->prio, s.tab->base, s.tab->mult, Qc, &pos);
      const emqx_mqueue_entry& e = b->ring[(sub * C + c) * Qc + pos];
      bool bad_ref;
      const bool expired = mq_expired(e.ref, b->now_ms, b->deadlines, b->ref_limit, &bad_ref);
      f(step++, c, e, expired, before, bad_ref);
      if (mq_counting(e.opts, expired)) {
        ++before;
        --n;
      }
    }
    return st;
  };
  // the count pass and the scan of the device form
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; ++k) {
    b->out_offsets[k] = total;
    const uint64_t sub = b->subs ? b->subs[k] : k;
    const Sess s = session_of(b, sub, scratch_sum);
    if (s.status != AK_OK) continue;
    fold(s, sub, [&](uint32_t, uint32_t, const emqx_mqueue_entry&, bool, uint32_t, bool) { ++total; });
  }
  b->out_offsets[m] = total;
  const bool full = total > b->cap_out;
  sum[PQ_T_ITEMS] = total;
  if (full) sum[PQ_S_FLAGS] |= PQ_F_OUTPUT_FULL;
  // the emit pass
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = b->subs ? b->subs[k] : k;
    const Sess s = session_of(b, sub, sum);
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    b->out_status[k] = s.status;
    if (s.status == PQ_UNFIT) sum[PQ_T_UNFIT] += 1;
    if (s.status != AK_OK) continue;
    sum[PQ_T_OKS] += 1;
    emqx_window_session& rec = b->sessions[sub];
    const PqState after = fold(s, sub, [&](uint32_t step, uint32_t c, const emqx_mqueue_entry& e, bool expired, uint32_t before, bool bad_ref) {
      uint16_t id;
      const uint8_t verdict = mq_item(e.opts, expired, rec.next_pkt_id, before, &id);
      counts[verdict == WN_SEND ? 0 : verdict == WN_SEND_QOS0 ? 1 : 2] += 1;
      if (bad_ref) sum[PQ_S_FLAGS] |= PQ_F_BAD_REF;
      if (full) return;
      const uint64_t pos = b->out_offsets[k] + step;
      b->out_opts[pos] = e.opts;
      b->out_verdicts[pos] = verdict;
      b->out_pkt_ids[pos] = id;
      b->out_refs[pos] = e.ref;
      b->out_class[pos] = static_cast<uint8_t>(c);
    });
    counts[3] = after.total;
    sum[PQ_T_SENDS] += counts[0];
    sum[PQ_T_SENDS0] += counts[1];
    sum[PQ_T_EXPIRED] += counts[2];
    if (!b->update_table || full) continue;
    pq_store(after, reinterpret_cast<PqHead*>(b->heads + sub));
    rec.mq_len = after.total;
    if (counts[0]) {
      rec.next_pkt_id = mq_next_pkt(rec.next_pkt_id, counts[0]);
      rec.inflight = wn_sat32(static_cast<uint64_t>(rec.inflight) + counts[0]);
    }
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

#ifndef EMQX_PMQUEUE_NO_DEVICE

// The scratch: take's tile totals, sized for the fewest sessions a block takes (those of the widest
// group); the counters with the take scan's total and decision and the synchronous forms' summary
// behind them.  Put ranks within its lane group and needs the counters alone.
struct Layout {
  uint64_t ctr, bytes;  // the tile totals stand at 0
};
Layout layout_of(uint64_t cap_boxes) {
  Layout l{};
  l.ctr = align256(8 * std::max<uint64_t>(pq_tiles(cap_boxes, PQ_MAX_GROUP), 1));
  l.bytes = l.ctr + align256((PQ_C_WORDS + PQ_S_WORDS) * sizeof(uint64_t));
  return l;
}

// Holds h->mu.  Grows the scratch.
int reserve_locked(emqx_pmqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  uint64_t in = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes);
  const int rc = grow_scratch(h, layout_of(boxes).bytes);
  if (rc != EMQX_OK) in = boxes = 0;  // there is no scratch any more
  h->cap_in = in;
  h->cap_boxes = boxes;
  return rc;
}

bool fits(emqx_pmqueue* h, uint64_t cap_boxes) { return h->d_scratch && cap_boxes <= h->cap_boxes; }

// The device forms move heads 16 bytes at a time and counts 16 bytes at a time.
bool aligned_ok(const emqx_pmqueue_put_args* b) {
  return al(b->inbox_subs, 4) && al(b->inbox_offsets, 8) && al(b->n_boxes, 8) && al(b->refs, 4) && al(b->box_src, 4) && al(b->tables, 4) &&
         al(b->sessions, 16) && al(b->ring, 8) && al(b->heads, 64) && al(b->out_evicted, 8) && al(b->out_counts, 16);
}
bool aligned_ok(const emqx_pmqueue_take_args* b) {
  return al(b->subs, 4) && al(b->n_boxes, 8) && al(b->tables, 4) && al(b->sessions, 16) && al(b->ring, 8) && al(b->heads, 64) &&
         al(b->deadlines, 8) && al(b->out_offsets, 8) && al(b->out_pkt_ids, 2) && al(b->out_refs, 4) && al(b->out_counts, 16);
}

int reserve(emqx_pmqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > AK_MAX_TOTAL || cap_boxes > AK_MAX_TOTAL) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  PqPutArgs a{};
  a.inbox_subs = b->inbox_subs;
  a.inbox_offsets = b->inbox_offsets;
  a.box_opts = b->box_opts;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.verdicts = b->verdicts;
  a.refs = b->refs;
  a.box_src = b->box_src;
  a.msg_class = b->msg_class;
  a.n_msgs = b->n_msgs;
  a.tables = reinterpret_cast<const PqTable*>(b->tables);
  a.n_tables = b->n_tables;
  a.sessions = reinterpret_cast<uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.ring = reinterpret_cast<uint2*>(b->ring);
  a.heads = reinterpret_cast<PqHead*>(b->heads);
  a.c = static_cast<uint32_t>(b->c);
  a.qc = static_cast<uint32_t>(b->qc);
  a.out_verdicts = b->out_verdicts;
  a.out_class = b->out_class;
  a.out_evicted = reinterpret_cast<uint2*>(b->out_evicted);
  a.out_counts = b->out_counts;
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.group = static_cast<uint32_t>(h->group);
  return pq_launch_put(a, s);
}

int launch(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  PqTakeArgs a{};
  a.subs = b->subs;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.tables = reinterpret_cast<const PqTable*>(b->tables);
  a.n_tables = b->n_tables;
  a.ring = reinterpret_cast<const uint2*>(b->ring);
  a.heads = reinterpret_cast<PqHead*>(b->heads);
  a.c = static_cast<uint32_t>(b->c);
  a.qc = static_cast<uint32_t>(b->qc);
  a.now_ms = b->now_ms;
  a.deadlines = b->deadlines;
  a.ref_limit = b->ref_limit;
  a.cap_out = b->cap_out;
  a.out_offsets = b->out_offsets;
  a.out_opts = b->out_opts;
  a.out_verdicts = b->out_verdicts;
  a.out_pkt_ids = b->out_pkt_ids;
  a.out_refs = b->out_refs;
  a.out_class = b->out_class;
  a.out_status = b->out_status;
  a.out_counts = b->out_counts;
  a.tile_tot = reinterpret_cast<uint64_t*>(p);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  a.group = static_cast<uint32_t>(h->group);
  return pq_launch_take(a, s);
}

struct Policy {
  static constexpr size_t WORDS = PQ_S_WORDS;
  template <class B>
  static bool batch_ok(const B* b) {
    return ::batch_ok(b);
  }
  template <class B>
  static bool aligned_ok(const B* b) {
    return ::aligned_ok(b);
  }
  template <class B>
  static bool fits(emqx_pmqueue* h, const B* b) {
    return ::fits(h, b->cap_boxes);
  }
  template <class B>
  static int reserve(emqx_pmqueue* h, const B* b) {
    return reserve_locked(h, 0, b->cap_boxes);
  }
  static Layout layout(const emqx_pmqueue* h) { return layout_of(h->cap_boxes); }
  static uint64_t* own_summary(const emqx_pmqueue* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.ctr) + PQ_C_WORDS;
  }
  template <class B>
  static int launch(emqx_pmqueue* h, const B* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

// The sessions a call names as tables of their own: session k reads row k; a subscriber the table does
// not hold becomes id m, which that table does not hold either.  The zone tables travel whole.
struct Gathered {
  std::vector<uint32_t> subs;
  std::vector<emqx_mqueue_entry> rows;
  std::vector<emqx_pmqueue_head> heads;
  std::vector<emqx_window_session> recs;
};
template <class SubOf>
void gather_rows(uint64_t m, uint64_t row, uint64_t sub_limit, SubOf sub_of, const emqx_mqueue_entry* ring, const emqx_pmqueue_head* heads,
                 const emqx_window_session* sessions, Gathered* g) {
  g->subs.resize(std::max<uint64_t>(m, 1));
  g->rows.assign(std::max<uint64_t>(m * row, 1), emqx_mqueue_entry{0, 0, {0, 0, 0}});
  g->heads.resize(std::max<uint64_t>(m, 1));
  g->recs.resize(std::max<uint64_t>(m, 1));
  std::memset(g->heads.data(), 0, g->heads.size() * sizeof(g->heads[0]));
  std::memset(g->recs.data(), 0, g->recs.size() * sizeof(g->recs[0]));
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = sub_of(k);
    const bool ok = sub < sub_limit;
    g->subs[k] = static_cast<uint32_t>(ok ? k : m);
    if (!ok) continue;
    std::memcpy(g->rows.data() + k * row, ring + sub * row, row * sizeof(emqx_mqueue_entry));
    g->heads[k] = heads[sub];
    g->recs[k] = sessions[sub];
  }
}

int run_batch(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m, row = b->c * b->qc;
  uint64_t sum[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t total;
  if (refused(b, m, &total, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  auto sub_of = [&](uint64_t k) -> uint64_t { return b->inbox_subs[k]; };
  Gathered ga;
  gather_rows(m, row, b->sub_limit, sub_of, b->ring, b->heads, b->sessions, &ga);
  emqx_pmqueue_put_args d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, m)) {
    const int rc = reserve_locked(h, total, m);
    if (rc != EMQX_OK) return rc;
  }
  const uint64_t n_cls = b->n_msgs * b->n_tables;
  Stage st{64};  // (the heads)
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_off = st.place((m + 1) * 8), o_opt = st.place(total), o_ver = st.place(total),
                 o_ref = st.place(b->refs ? total * 4 : 0), o_src = st.place(total * 4), o_cls = st.place(n_cls),
                 o_zone = st.place(b->n_tables * sizeof(emqx_pmqueue_table)), o_tab = st.place(ga.recs.size() * 32),
                 o_row = st.place(ga.rows.size() * 8), o_hd = st.place(ga.heads.size() * 64), o_ov = st.place(total), o_oc = st.place(total),
                 o_evi = st.place(total * 8), o_cnt = st.place(std::max<uint64_t>(m, 1) * 32);
  const int src = stage_reserve(h, st.at, 64);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.inbox_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.inbox_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.box_opts = D + o_opt;
  d.verdicts = D + o_ver;
  d.refs = b->refs ? reinterpret_cast<const uint32_t*>(D + o_ref) : nullptr;
  d.box_src = reinterpret_cast<const uint32_t*>(D + o_src);
  d.msg_class = D + o_cls;
  d.tables = reinterpret_cast<const emqx_pmqueue_table*>(D + o_zone);
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.ring = reinterpret_cast<emqx_mqueue_entry*>(D + o_row);
  d.heads = reinterpret_cast<emqx_pmqueue_head*>(D + o_hd);
  d.out_verdicts = D + o_ov;
  d.out_class = D + o_oc;
  d.out_evicted = reinterpret_cast<emqx_mqueue_entry*>(D + o_evi);
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_off, b->inbox_offsets, (m + 1) * 8);
  cp.up(o_opt, b->box_opts, total);
  cp.up(o_ver, b->verdicts, total);
  if (b->refs) cp.up(o_ref, b->refs, total * 4);
  cp.up(o_src, b->box_src, total * 4);
  cp.up(o_cls, b->msg_class, n_cls);
  cp.up(o_zone, b->tables, b->n_tables * sizeof(emqx_pmqueue_table));
  cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * row * 8);
  cp.up(o_hd, ga.heads.data(), m * 64);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(b->out_verdicts, o_ov, total);
    cp.down(b->out_class, o_oc, total);
    cp.down(b->out_evicted, o_evi, total * 8);
    cp.down(b->out_counts, o_cnt, m * 32);
    cp.down(ga.rows.data(), o_row, m * row * 8);
    cp.down(ga.heads.data(), o_hd, m * 64);
    cp.down(ga.recs.data(), o_tab, m * 32);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  if (!(sum[PQ_S_FLAGS] & PQ_F_INPUT_REFUSED)) {
    for (uint64_t k = 0; k < m; ++k) {
      const uint64_t sub = sub_of(k);
      if (sub >= b->sub_limit || b->out_counts[PQ_COUNT_WORDS * k + 7] != AK_OK) continue;
      std::memcpy(b->ring + sub * row, ga.rows.data() + k * row, row * sizeof(emqx_mqueue_entry));
      if (!b->update_table) continue;
      b->heads[sub] = ga.heads[k];
      b->sessions[sub].mq_len = ga.recs[k].mq_len;
      b->sessions[sub].dropped = ga.recs[k].dropped;
    }
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m, row = b->c * b->qc;
  uint64_t sum[PQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  auto sub_of = [&](uint64_t k) -> uint64_t { return b->subs ? b->subs[k] : k; };
  Gathered ga;
  gather_rows(m, row, b->sub_limit, sub_of, b->ring, b->heads, b->sessions, &ga);
  const uint64_t n_dead = b->deadlines ? b->ref_limit : 0;
  emqx_pmqueue_take_args d = *b;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, m)) {
    const int rc = reserve_locked(h, 0, m);
    if (rc != EMQX_OK) return rc;
  }
  const uint64_t cap = b->cap_out;
  Stage st{64};  // (the heads)
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_zone = st.place(b->n_tables * sizeof(emqx_pmqueue_table)),
                 o_tab = st.place(ga.recs.size() * 32), o_row = st.place(ga.rows.size() * 8), o_hd = st.place(ga.heads.size() * 64),
                 o_ddl = st.place(n_dead * 8), o_off = st.place((m + 1) * 8), o_opt = st.place(cap), o_ver = st.place(cap),
                 o_cls = st.place(cap), o_pkt = st.place(cap * 2), o_ref = st.place(cap * 4), o_sta = st.place(m), o_cnt = st.place(m * 16);
  const int src = stage_reserve(h, st.at, 64);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.tables = reinterpret_cast<const emqx_pmqueue_table*>(D + o_zone);
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.ring = reinterpret_cast<const emqx_mqueue_entry*>(D + o_row);
  d.heads = reinterpret_cast<emqx_pmqueue_head*>(D + o_hd);
  d.deadlines = b->deadlines ? reinterpret_cast<const uint64_t*>(D + o_ddl) : nullptr;  // (ref_limit 0: never read)
  d.out_offsets = reinterpret_cast<uint64_t*>(D + o_off);
  d.out_opts = D + o_opt;
  d.out_verdicts = D + o_ver;
  d.out_class = D + o_cls;
  d.out_pkt_ids = reinterpret_cast<uint16_t*>(D + o_pkt);
  d.out_refs = reinterpret_cast<uint32_t*>(D + o_ref);
  d.out_status = D + o_sta;
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_zone, b->tables, b->n_tables * sizeof(emqx_pmqueue_table));
  cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * row * 8);
  cp.up(o_hd, ga.heads.data(), m * 64);
  cp.up(o_ddl, b->deadlines, n_dead * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;  // the summary says what to bring back
  const bool full = (sum[PQ_S_FLAGS] & PQ_F_OUTPUT_FULL) != 0;
  const bool none = (sum[PQ_S_FLAGS] & PQ_F_INPUT_REFUSED) != 0;
  if (rc == EMQX_OK && !none) {
    cp.down(b->out_offsets, o_off, (m + 1) * 8);
    cp.down(b->out_status, o_sta, m);
    cp.down(b->out_counts, o_cnt, m * 16);
    if (!full) {
      const uint64_t items = std::min<uint64_t>(sum[PQ_T_ITEMS], cap);
      cp.down(b->out_opts, o_opt, items);
      cp.down(b->out_verdicts, o_ver, items);
      cp.down(b->out_class, o_cls, items);
      cp.down(b->out_pkt_ids, o_pkt, items * 2);
      cp.down(b->out_refs, o_ref, items * 4);
      if (b->update_table) {
        cp.down(ga.heads.data(), o_hd, m * 64);
        cp.down(ga.recs.data(), o_tab, m * 32);
      }
    }
    if (!cp.ok) rc = EMQX_EDEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  }
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  if (!none && !full && b->update_table) {
    for (uint64_t k = 0; k < m; ++k) {
      const uint64_t sub = sub_of(k);
      if (sub >= b->sub_limit || b->out_status[k] != AK_OK) continue;
      b->heads[sub] = ga.heads[k];
      b->sessions[sub].inflight = ga.recs[k].inflight;
      b->sessions[sub].mq_len = ga.recs[k].mq_len;
      b->sessions[sub].next_pkt_id = ga.recs[k].next_pkt_id;
    }
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

#endif  // EMQX_PMQUEUE_NO_DEVICE

int pmqueue_set_tuning(emqx_pmqueue* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t hi;
  if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = AK_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = AK_SCAN_BLOCK;
  } else if (std::strcmp(key, "group") == 0) {
    if (!pq_group_ok(value)) return EMQX_EINVAL;
    field = &h->group;
    hi = PQ_MAX_GROUP;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < 1 || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int pmqueue_stats_get(emqx_pmqueue* h, emqx_pmqueue_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_pmqueue_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.cap_boxes = h->cap_boxes;
  s.scratch_bytes = h->scratch_bytes;
  s.group = static_cast<uint64_t>(h->group);
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_pmqueue_create(int32_t device, emqx_pmqueue** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_pmqueue_destroy(emqx_pmqueue* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_pmqueue_reserve(emqx_pmqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  return guarded([&] { return reserve(h, cap_in, cap_boxes); });
}
int emqx_pmqueue_put_batch(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_pmqueue_take_batch(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_pmqueue_put_batch_device(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_pmqueue_put_batch_device_async(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_pmqueue_put_host(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out) {
  return guarded([&] { return put_host(h, b, summary_out); });
}
int emqx_pmqueue_take_batch_device(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_pmqueue_take_batch_device_async(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_pmqueue_take_host(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out) {
  return guarded([&] { return take_host(h, b, summary_out); });
}
int emqx_pmqueue_set_tuning(emqx_pmqueue* h, const char* key, int64_t value) {
  return guarded([&] { return pmqueue_set_tuning(h, key, value); });
}
int emqx_pmqueue_stats_get(emqx_pmqueue* h, emqx_pmqueue_stats* out) {
  return guarded([&] { return pmqueue_stats_get(h, out); });
}

}  // extern "C"
