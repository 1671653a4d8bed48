// C ABI of the mqueue stage (include/emqx_mqueue.h): the handle and its device scratch, the device
// entry points of both calls and the host evaluators.  The closed forms live in mqueue.h and are the
// same code on both sides.  With EMQX_MQUEUE_NO_DEVICE this file compiles with a plain C++ compiler
// into the host-only part (tests/c/test_mqueue_host.cpp): handles of device EMQX_MQUEUE_HOST_ONLY
// alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_MQUEUE_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/emqx_mqueue.h"
#include "mqueue.h"
#include "stage_host.h"

using namespace emqx;

static_assert(MQ_F_INPUT_REFUSED == EMQX_MQ_F_INPUT_REFUSED && MQ_F_BAD_SUB == EMQX_MQ_F_BAD_SUB &&
                  MQ_F_OUTPUT_FULL == EMQX_MQ_F_OUTPUT_FULL && MQ_F_BAD_REF == EMQX_MQ_F_BAD_REF && MQ_F_BAD_RING == EMQX_MQ_F_BAD_RING &&
                  MQ_F_ROW_FULL == EMQX_MQ_F_ROW_FULL && MQ_F_LEN_MISMATCH == EMQX_MQ_F_LEN_MISMATCH &&
                  MQ_S_WORDS == EMQX_MQ_SUMMARY_WORDS,
              "flags");
static_assert(MQ_MIN_Q == EMQX_MQ_MIN_Q && MQ_MAX_Q == EMQX_MQ_MAX_Q && MQ_NO_REF == EMQX_MQ_NO_REF && MQ_EXPIRED == EMQX_MQ_EXPIRED &&
                  MQ_NO_EXPIRY == EMQX_RETRY_NO_EXPIRY && MQ_MAX_NOW == EMQX_RETRY_MAX_NOW,
              "constants");
static_assert(WN_SEND_QOS0 == EMQX_W_SEND_QOS0 && WN_SEND == EMQX_W_SEND && WN_QUEUED == EMQX_W_QUEUED &&
                  WN_QUEUED_DROPPED == EMQX_W_QUEUED_DROPPED && WN_EVICTS == EMQX_W_EVICTS && AK_W_MASK == EMQX_W_VERDICT_MASK &&
                  AK_O_QOS == EMQX_DELIVER_QOS_MASK && AK_OK == EMQX_A_OK && AK_NO_SESSION == EMQX_A_NO_SESSION && AK_PASS == EMQX_A_PASS &&
                  AK_PRESENT == EMQX_WINDOW_PRESENT && AK_PASSF == EMQX_WINDOW_PASS,
              "what the stage reads of the window and the ack stage");
static_assert(sizeof(emqx_mqueue_entry) == 8 && sizeof(emqx_mqueue_ring) == 8 && offsetof(emqx_mqueue_entry, opts) == 4 &&
                  sizeof(emqx_window_session) == 4 * AK_REC_WORDS && offsetof(emqx_window_session, inflight) == 4 * AK_REC_INFLIGHT &&
                  offsetof(emqx_window_session, inflight_max) == 4 * AK_REC_INFLIGHT_MAX &&
                  offsetof(emqx_window_session, mq_len) == 4 * MQ_REC_MQ_LEN &&
                  offsetof(emqx_window_session, next_pkt_id) == 4 * MQ_REC_NEXT_PKT && offsetof(emqx_window_session, flags) == 4 * AK_REC_FLAGS,
              "layout");

static_assert(EMQX_MQUEUE_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_mqueue : StageHandle {  // (stage_host.h)
  int64_t max_blocks = AK_MAX_BLOCKS, scan_chunk = AK_SCAN_BLOCK;
  uint64_t cap_in = 0, cap_boxes = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What every form requires of its argument block, whichever memory it points into.
bool batch_ok(const emqx_mqueue_put_args* b) {
  if (!b || !mq_q_ok(b->q)) return false;
  if (b->cap_in > AK_MAX_TOTAL || b->cap_boxes > AK_MAX_TOTAL || b->sub_limit > MAX_SUB_LIMIT) return false;
  if (!b->n_boxes && b->m > b->cap_boxes) return false;
  if (!b->inbox_offsets) return false;
  if (b->cap_boxes && (!b->inbox_subs || !b->out_unstored)) return false;
  if (b->cap_in && (!b->box_opts || !b->verdicts || !b->out_evicted)) return false;
  if (b->sub_limit && (!b->ring || !b->heads)) return false;
  return true;
}
bool batch_ok(const emqx_mqueue_take_args* b) {
  if (!b || !mq_q_ok(b->q) || b->now_ms >= MQ_MAX_NOW) return false;
  if (b->cap_boxes > AK_MAX_TOTAL || b->sub_limit > MAX_SUB_LIMIT || b->cap_out > AK_MAX_TOTAL * MQ_MAX_Q) return false;
  if (!b->n_boxes && b->m > b->cap_boxes) return false;
  if (b->sub_limit && (!b->sessions || !b->ring || !b->heads)) return false;
  if (!b->out_offsets) return false;
  if (b->cap_out && (!b->out_opts || !b->out_verdicts || !b->out_pkt_ids || !b->out_refs)) return false;
  if (b->cap_boxes && (!b->out_status || !b->out_counts)) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, MQ_S_WORDS * sizeof(uint64_t));
  if (sum[MQ_S_FLAGS] & MQ_F_INPUT_REFUSED) return EMQX_EINVAL;
  if (sum[MQ_S_FLAGS] & MQ_F_OUTPUT_FULL) return EMQX_EOVERFLOW;
  return (sum[MQ_S_FLAGS] & MQ_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.
bool refused(const emqx_mqueue_put_args* b, uint64_t m, uint64_t* total, uint64_t* sum) {
  *total = 0;
  sum[MQ_S_BOXES] = m;
  if (m <= b->cap_boxes && m <= AK_MAX_TOTAL) {
    *total = b->inbox_offsets[m];
    sum[MQ_S_TOTAL] = *total;
    if (*total <= b->cap_in && *total <= AK_MAX_TOTAL) return false;
  }
  sum[MQ_S_FLAGS] = MQ_F_INPUT_REFUSED;
  return true;
}
bool refused(const emqx_mqueue_take_args* b, uint64_t m, uint64_t* sum) {
  sum[MQ_S_BOXES] = m;
  if (m <= b->cap_boxes && m <= AK_MAX_TOTAL && (b->subs || m <= b->sub_limit)) return false;
  sum[MQ_S_FLAGS] = MQ_F_INPUT_REFUSED;
  return true;
}

// ---- the host evaluators -----------------------------------------------------------------------

const emqx_mqueue_entry NO_ENTRY = {MQ_NO_REF, 0, {0, 0, 0}};

int put_host(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t total;
  if (refused(b, m, &total, sum)) return status_of(sum, summary_out);
  const uint32_t Q = static_cast<uint32_t>(b->q), qm = Q - 1;
  for (uint64_t d = 0; d < total; ++d) b->out_evicted[d] = NO_ENTRY;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = b->inbox_subs[k];
    const bool ok = sub < b->sub_limit;
    const uint64_t lo = std::min(b->inbox_offsets[k], total), hi = std::min(b->inbox_offsets[k + 1], total);
    uint32_t s = 0, x = 0, qd = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      s += mq_is_queued(b->verdicts[d]);
      x += mq_evicts(b->verdicts[d]);
      qd += mq_is_qdropped(b->verdicts[d]);
    }
    uint32_t hd = 0, L = 0;
    bool bad = false;
    if (ok) mq_header(b->heads[sub].head, b->heads[sub].len, Q, &hd, &L, &bad);
    const MqPlan p = mq_put_plan(ok, hd, L, Q, s, x, qd);
    b->out_unstored[k] = p.unstored;
    sum[MQ_P_STORED] += p.stored;
    sum[MQ_P_EVICTED] += p.ev;
    sum[MQ_P_UNSTORED] += p.unstored;
    if (!ok) {
      sum[MQ_S_FLAGS] |= MQ_F_BAD_SUB;
      continue;
    }
    emqx_mqueue_entry* row = b->ring + sub * Q;
    // every read of an old entry stands in front of the stores: with L = Q they share positions
    uint32_t j = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      if (!mq_evicts(b->verdicts[d])) continue;
      if (j < L) b->out_evicted[d] = row[(hd + j) & qm];
      ++j;
    }
    uint32_t r = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      if (!mq_is_queued(b->verdicts[d])) continue;
      if (r < p.room) {
        emqx_mqueue_entry& e = row[(p.start + r) & qm];
        e.ref = b->refs ? b->refs[d] : static_cast<uint32_t>(d);
        e.opts = b->box_opts[d];
        e.rsv[0] = e.rsv[1] = e.rsv[2] = 0;
      }
      ++r;
    }
    b->heads[sub].head = p.head;
    b->heads[sub].len = p.len;
    if (p.unstored) {
      sum[MQ_P_FULL_ROWS] += 1;
      sum[MQ_S_FLAGS] |= MQ_F_ROW_FULL;
    }
    if (bad) sum[MQ_S_FLAGS] |= MQ_F_BAD_RING;
    if (b->sessions && b->sessions[sub].mq_len != p.len) {
      sum[MQ_P_MISMATCH] += 1;
      sum[MQ_S_FLAGS] |= MQ_F_LEN_MISMATCH;
    }
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

int take_host(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  const uint32_t Q = static_cast<uint32_t>(b->q), qm = Q - 1;
  struct Row {
    uint64_t sub;
    uint32_t h, L, n;
    uint8_t dead;
    bool bad;
  };
  auto row_of = [&](uint64_t k) {
    Row r{b->subs ? b->subs[k] : k, 0, 0, 0, 0, false};
    const bool ok = r.sub < b->sub_limit;
    r.dead = ak_session(ok, ok ? b->sessions[r.sub].flags : 0u);
    if (r.dead) return r;
    mq_header(b->heads[r.sub].head, b->heads[r.sub].len, Q, &r.h, &r.L, &r.bad);
    r.n = mq_budget(b->sessions[r.sub].inflight_max, b->sessions[r.sub].inflight);
    return r;
  };
  // One consumed entry after the other: f(i, entry, expired, before, bad_ref).
  auto fold = [&](const Row& r, auto&& f) {
    uint32_t before = 0;
    for (uint32_t i = 0; i < r.L && mq_consumed(before, r.n); ++i) {
      const emqx_mqueue_entry& e = b->ring[r.sub * Q + ((r.h + i) & qm)];
      bool bad_ref;
      const bool expired = mq_expired(e.ref, b->now_ms, b->deadlines, b->ref_limit, &bad_ref);
      f(i, e, expired, before, bad_ref);
      before += mq_counting(e.opts, expired) ? 1u : 0u;
    }
  };
  // the count pass and the scan of the device form
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; ++k) {
    b->out_offsets[k] = total;
    const Row r = row_of(k);
    if (r.dead) continue;
    fold(r, [&](uint32_t, const emqx_mqueue_entry&, bool, uint32_t, bool) { ++total; });
  }
  b->out_offsets[m] = total;
  const bool full = total > b->cap_out;
  sum[MQ_T_ITEMS] = total;
  if (full) sum[MQ_S_FLAGS] |= MQ_F_OUTPUT_FULL;
  // the emit pass
  for (uint64_t k = 0; k < m; ++k) {
    const Row r = row_of(k);
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    b->out_status[k] = r.dead ? r.dead : AK_OK;
    if (r.sub >= b->sub_limit) sum[MQ_S_FLAGS] |= MQ_F_BAD_SUB;
    if (r.dead) continue;
    sum[MQ_T_OKS] += 1;
    emqx_window_session& rec = b->sessions[r.sub];
    uint32_t items = 0;
    fold(r, [&](uint32_t i, const emqx_mqueue_entry& e, bool expired, uint32_t before, bool bad_ref) {
      uint16_t id;
      const uint8_t verdict = mq_item(e.opts, expired, rec.next_pkt_id, before, &id);
      counts[verdict == WN_SEND ? 0 : verdict == WN_SEND_QOS0 ? 1 : 2] += 1;
      if (bad_ref) sum[MQ_S_FLAGS] |= MQ_F_BAD_REF;
      ++items;
      if (full) return;
      const uint64_t pos = b->out_offsets[k] + i;
      b->out_opts[pos] = e.opts;
      b->out_verdicts[pos] = verdict;
      b->out_pkt_ids[pos] = id;
      b->out_refs[pos] = e.ref;
    });
    counts[3] = r.L - items;
    sum[MQ_T_SENDS] += counts[0];
    sum[MQ_T_SENDS0] += counts[1];
    sum[MQ_T_EXPIRED] += counts[2];
    if (rec.mq_len != r.L) {
      sum[MQ_T_MISMATCH] += 1;
      sum[MQ_S_FLAGS] |= MQ_F_LEN_MISMATCH;
    }
    if (r.bad) sum[MQ_S_FLAGS] |= MQ_F_BAD_RING;
    if (!b->update_table || full) continue;
    b->heads[r.sub].head = (r.h + items) & qm;
    b->heads[r.sub].len = r.L - items;
    rec.mq_len = r.L - items;
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

#ifndef EMQX_MQUEUE_NO_DEVICE

// What the scratch has to take for a call.
struct Need {
  uint64_t cap_in, cap_boxes;
};
Need need_of(const emqx_mqueue_put_args* b) { return {b->cap_in, b->cap_boxes}; }
Need need_of(const emqx_mqueue_take_args* b) { return {0, b->cap_boxes}; }

// The scratch: put's tile totals, head prefixes and plans; take's tile totals (sized for the
// fewest sessions a block takes, those of the largest Q); the counters with the take scan's total
// and decision and the synchronous forms' summary behind them.
struct Layout {
  uint64_t tile_sx, tile_qd, head_pre, plans, take_tot, ctr, bytes;
};

Layout layout_of(uint64_t cap_in, uint64_t cap_boxes) {
  Layout l{};
  const uint64_t tiles = std::max<uint64_t>(mq_tiles(cap_in), 1);
  uint64_t at = 0;
  auto place = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += align256(bytes);
    return o;
  };
  l.tile_sx = place(8 * tiles);
  l.tile_qd = place(4 * tiles);
  l.head_pre = place(8 * (cap_boxes + 1));
  l.plans = place(8 * std::max<uint64_t>(cap_boxes, 1));
  l.take_tot = place(8 * std::max<uint64_t>(mq_take_tiles(cap_boxes, MQ_MAX_Q), 1));
  l.ctr = place((MQ_C_WORDS + MQ_S_WORDS) * sizeof(uint64_t));
  l.bytes = at;
  return l;
}

// Holds h->mu.  Grows the scratch.
int reserve_locked(emqx_mqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  uint64_t in = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes);
  const int rc = grow_scratch(h, layout_of(in, boxes).bytes);
  if (rc != EMQX_OK) in = boxes = 0;  // there is no scratch any more
  h->cap_in = in;
  h->cap_boxes = boxes;
  return rc;
}

bool fits(emqx_mqueue* h, const Need& n) { return h->d_scratch && n.cap_in <= h->cap_in && n.cap_boxes <= h->cap_boxes; }

// The device forms move ring pairs and counts 16 bytes at a time.
bool aligned_ok(const emqx_mqueue_put_args* b) {
  return al(b->inbox_subs, 4) && al(b->inbox_offsets, 8) && al(b->n_boxes, 8) && al(b->refs, 4) && al(b->sessions, 16) &&
         al(b->ring, 16) && al(b->heads, 8) && al(b->out_evicted, 8) && al(b->out_unstored, 4);
}
bool aligned_ok(const emqx_mqueue_take_args* b) {
  return al(b->subs, 4) && al(b->n_boxes, 8) && al(b->sessions, 16) && al(b->ring, 16) && al(b->heads, 8) && al(b->deadlines, 8) &&
         al(b->out_offsets, 8) && al(b->out_pkt_ids, 2) && al(b->out_refs, 4) && al(b->out_counts, 16);
}

int reserve(emqx_mqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > AK_MAX_TOTAL || cap_boxes > AK_MAX_TOTAL) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  MqPutArgs a{};
  a.inbox_subs = b->inbox_subs;
  a.inbox_offsets = b->inbox_offsets;
  a.box_opts = b->box_opts;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.verdicts = b->verdicts;
  a.refs = b->refs;
  a.sessions = reinterpret_cast<const uint32_t*>(b->sessions);
  a.ring = reinterpret_cast<uint2*>(b->ring);
  a.heads = reinterpret_cast<uint2*>(b->heads);
  a.q = static_cast<uint32_t>(b->q);
  a.sub_limit = b->sub_limit;
  a.out_evicted = reinterpret_cast<uint2*>(b->out_evicted);
  a.out_unstored = b->out_unstored;
  a.tile_sx = reinterpret_cast<uint64_t*>(p + l.tile_sx);
  a.tile_qd = reinterpret_cast<uint32_t*>(p + l.tile_qd);
  a.head_pre = reinterpret_cast<uint64_t*>(p + l.head_pre);
  a.plans = reinterpret_cast<uint2*>(p + l.plans);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return mq_launch_put(a, s);
}

int launch(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  MqTakeArgs a{};
  a.subs = b->subs;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.ring = reinterpret_cast<const uint2*>(b->ring);
  a.heads = reinterpret_cast<uint2*>(b->heads);
  a.q = static_cast<uint32_t>(b->q);
  a.now_ms = b->now_ms;
  a.deadlines = b->deadlines;
  a.ref_limit = b->ref_limit;
  a.cap_out = b->cap_out;
  a.out_offsets = b->out_offsets;
  a.out_opts = b->out_opts;
  a.out_verdicts = b->out_verdicts;
  a.out_pkt_ids = b->out_pkt_ids;
  a.out_refs = b->out_refs;
  a.out_status = b->out_status;
  a.out_counts = b->out_counts;
  a.tile_tot = reinterpret_cast<uint64_t*>(p + l.take_tot);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return mq_launch_take(a, s);
}

struct Policy {
  static constexpr size_t WORDS = MQ_S_WORDS;
  template <class B>
  static bool batch_ok(const B* b) {
    return ::batch_ok(b);
  }
  template <class B>
  static bool aligned_ok(const B* b) {
    return ::aligned_ok(b);
  }
  template <class B>
  static bool fits(emqx_mqueue* h, const B* b) {
    return ::fits(h, need_of(b));
  }
  template <class B>
  static int reserve(emqx_mqueue* h, const B* b) {
    const Need n = need_of(b);
    return reserve_locked(h, n.cap_in, n.cap_boxes);
  }
  static Layout layout(const emqx_mqueue* h) { return layout_of(h->cap_in, h->cap_boxes); }
  static uint64_t* own_summary(const emqx_mqueue* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.ctr) + MQ_C_WORDS;
  }
  template <class B>
  static int launch(emqx_mqueue* h, const B* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

// The rows the call names as tables of their own: session k reads row k; a subscriber the table
// does not hold becomes id m, which that table does not hold either.
struct Gathered {
  std::vector<uint32_t> subs;
  std::vector<emqx_mqueue_entry> rows;
  std::vector<emqx_mqueue_ring> heads;
  std::vector<emqx_window_session> recs;
};
template <class SubOf>
void gather_rows(uint64_t m, uint64_t q, uint64_t sub_limit, SubOf sub_of, const emqx_mqueue_entry* ring, const emqx_mqueue_ring* heads,
                 const emqx_window_session* sessions, Gathered* g) {
  g->subs.resize(std::max<uint64_t>(m, 1));
  g->rows.assign(std::max<uint64_t>(m * q, 2), emqx_mqueue_entry{0, 0, {0, 0, 0}});
  g->heads.assign(std::max<uint64_t>(m, 1), emqx_mqueue_ring{0, 0});
  g->recs.resize(std::max<uint64_t>(m, 1));
  std::memset(g->recs.data(), 0, g->recs.size() * sizeof(g->recs[0]));
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = sub_of(k);
    const bool ok = sub < sub_limit;
    g->subs[k] = static_cast<uint32_t>(ok ? k : m);
    if (!ok) continue;
    std::memcpy(g->rows.data() + k * q, ring + sub * q, q * sizeof(emqx_mqueue_entry));
    g->heads[k] = heads[sub];
    if (sessions) g->recs[k] = sessions[sub];
  }
}

int run_batch(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m, q = b->q;
  uint64_t sum[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t total;
  if (refused(b, m, &total, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  auto sub_of = [&](uint64_t k) -> uint64_t { return b->inbox_subs[k]; };
  Gathered ga;
  gather_rows(m, q, b->sub_limit, sub_of, b->ring, b->heads, b->sessions, &ga);
  emqx_mqueue_put_args d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, need_of(&d))) {
    const int rc = reserve_locked(h, total, m);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_off = st.place((m + 1) * 8), o_opt = st.place(total), o_ver = st.place(total),
                 o_ref = st.place(b->refs ? total * 4 : 0), o_tab = st.place(ga.recs.size() * 32), o_row = st.place(ga.rows.size() * 8),
                 o_hd = st.place(ga.heads.size() * 8), o_evi = st.place(total * 8), o_uns = st.place(std::max<uint64_t>(m, 1) * 4);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.inbox_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.inbox_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.box_opts = D + o_opt;
  d.verdicts = D + o_ver;
  d.refs = b->refs ? reinterpret_cast<const uint32_t*>(D + o_ref) : nullptr;
  d.sessions = b->sessions ? reinterpret_cast<const emqx_window_session*>(D + o_tab) : nullptr;
  d.ring = reinterpret_cast<emqx_mqueue_entry*>(D + o_row);
  d.heads = reinterpret_cast<emqx_mqueue_ring*>(D + o_hd);
  d.out_evicted = reinterpret_cast<emqx_mqueue_entry*>(D + o_evi);
  d.out_unstored = reinterpret_cast<uint32_t*>(D + o_uns);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_off, b->inbox_offsets, (m + 1) * 8);
  cp.up(o_opt, b->box_opts, total);
  cp.up(o_ver, b->verdicts, total);
  if (b->refs) cp.up(o_ref, b->refs, total * 4);
  if (b->sessions) cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * q * 8);
  cp.up(o_hd, ga.heads.data(), m * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(b->out_evicted, o_evi, total * 8);
    cp.down(b->out_unstored, o_uns, m * 4);
    cp.down(ga.rows.data(), o_row, m * q * 8);
    cp.down(ga.heads.data(), o_hd, m * 8);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  if (!(sum[MQ_S_FLAGS] & MQ_F_INPUT_REFUSED)) {
    for (uint64_t k = 0; k < m; ++k) {
      const uint64_t sub = sub_of(k);
      if (sub >= b->sub_limit) continue;
      std::memcpy(b->ring + sub * q, ga.rows.data() + k * q, q * sizeof(emqx_mqueue_entry));
      b->heads[sub] = ga.heads[k];
    }
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m, q = b->q;
  uint64_t sum[MQ_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  auto sub_of = [&](uint64_t k) -> uint64_t { return b->subs ? b->subs[k] : k; };
  Gathered ga;
  gather_rows(m, q, b->sub_limit, sub_of, b->ring, b->heads, b->sessions, &ga);
  const uint64_t n_dead = b->deadlines ? b->ref_limit : 0;
  emqx_mqueue_take_args d = *b;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, need_of(&d))) {
    const int rc = reserve_locked(h, 0, m);
    if (rc != EMQX_OK) return rc;
  }
  const uint64_t cap = b->cap_out;
  Stage st{16};
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_tab = st.place(ga.recs.size() * 32), o_row = st.place(ga.rows.size() * 8),
                 o_hd = st.place(ga.heads.size() * 8), o_ddl = st.place(n_dead * 8), o_off = st.place((m + 1) * 8), o_opt = st.place(cap),
                 o_ver = st.place(cap), o_pkt = st.place(cap * 2), o_ref = st.place(cap * 4), o_sta = st.place(m), o_cnt = st.place(m * 16);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.ring = reinterpret_cast<const emqx_mqueue_entry*>(D + o_row);
  d.heads = reinterpret_cast<emqx_mqueue_ring*>(D + o_hd);
  d.deadlines = b->deadlines ? reinterpret_cast<const uint64_t*>(D + o_ddl) : nullptr;  // (ref_limit 0: never read)
  d.out_offsets = reinterpret_cast<uint64_t*>(D + o_off);
  d.out_opts = D + o_opt;
  d.out_verdicts = D + o_ver;
  d.out_pkt_ids = reinterpret_cast<uint16_t*>(D + o_pkt);
  d.out_refs = reinterpret_cast<uint32_t*>(D + o_ref);
  d.out_status = D + o_sta;
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * q * 8);
  cp.up(o_hd, ga.heads.data(), m * 8);
  cp.up(o_ddl, b->deadlines, n_dead * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;  // the summary says what to bring back
  const bool full = (sum[MQ_S_FLAGS] & MQ_F_OUTPUT_FULL) != 0;
  const bool none = (sum[MQ_S_FLAGS] & MQ_F_INPUT_REFUSED) != 0;
  if (rc == EMQX_OK && !none) {
    cp.down(b->out_offsets, o_off, (m + 1) * 8);
    cp.down(b->out_status, o_sta, m);
    cp.down(b->out_counts, o_cnt, m * 16);
    if (!full) {
      const uint64_t items = std::min<uint64_t>(sum[MQ_T_ITEMS], cap);
      cp.down(b->out_opts, o_opt, items);
      cp.down(b->out_verdicts, o_ver, items);
      cp.down(b->out_pkt_ids, o_pkt, items * 2);
      cp.down(b->out_refs, o_ref, items * 4);
      if (b->update_table) {
        cp.down(ga.heads.data(), o_hd, m * 8);
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

#endif  // EMQX_MQUEUE_NO_DEVICE

int mqueue_set_tuning(emqx_mqueue* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t hi;
  if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = AK_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = AK_SCAN_BLOCK;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < 1 || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int mqueue_stats_get(emqx_mqueue* h, emqx_mqueue_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_mqueue_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.cap_boxes = h->cap_boxes;
  s.scratch_bytes = h->scratch_bytes;
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_mqueue_create(int32_t device, emqx_mqueue** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_mqueue_destroy(emqx_mqueue* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_mqueue_reserve(emqx_mqueue* h, uint64_t cap_in, uint64_t cap_boxes) {
  return guarded([&] { return reserve(h, cap_in, cap_boxes); });
}
int emqx_mqueue_put_batch(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_mqueue_put_batch_device(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_mqueue_put_batch_device_async(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_mqueue_put_host(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out) {
  return guarded([&] { return put_host(h, b, summary_out); });
}
int emqx_mqueue_take_batch(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_mqueue_take_batch_device(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_mqueue_take_batch_device_async(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_mqueue_take_host(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out) {
  return guarded([&] { return take_host(h, b, summary_out); });
}
int emqx_mqueue_set_tuning(emqx_mqueue* h, const char* key, int64_t value) {
  return guarded([&] { return mqueue_set_tuning(h, key, value); });
}
int emqx_mqueue_stats_get(emqx_mqueue* h, emqx_mqueue_stats* out) {
  return guarded([&] { return mqueue_stats_get(h, out); });
}

}  // extern "C"
