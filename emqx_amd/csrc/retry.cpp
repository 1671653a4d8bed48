// C ABI of the retry stage (include/emqx_retry.h): the handle and its device scratch, the device
// entry points of both calls and the host evaluators.  The closed form of the fold lives in retry.h
// and is the same code on both sides.  With EMQX_RETRY_NO_DEVICE this file compiles with a plain
// C++ compiler into the host-only part (tests/c/test_retry_host.cpp): handles of device
// EMQX_RETRY_HOST_ONLY alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_RETRY_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/emqx_retry.h"
#include "retry.h"
#include "stage_host.h"

using namespace emqx;

static_assert(RT_F_INPUT_REFUSED == EMQX_RETRY_F_INPUT_REFUSED && RT_F_BAD_SUB == EMQX_RETRY_F_BAD_SUB &&
                  RT_F_OUTPUT_FULL == EMQX_RETRY_F_OUTPUT_FULL && RT_F_BAD_REF == EMQX_RETRY_F_BAD_REF &&
                  RT_F_UNSTAMPED == EMQX_RETRY_F_UNSTAMPED && RT_S_WORDS == EMQX_RETRY_SUMMARY_WORDS,
              "flags");
static_assert(RT_MODE_RETRY == EMQX_RETRY_MODE_RETRY && RT_MODE_REPLAY == EMQX_RETRY_MODE_REPLAY &&
                  RT_PUBLISH_DUP == EMQX_RETRY_PUBLISH_DUP && RT_PUBREL == EMQX_RETRY_PUBREL && RT_EXPIRED == EMQX_RETRY_EXPIRED,
              "modes and kinds");
static_assert(RT_NO_TIMER == EMQX_RETRY_NO_TIMER && RT_NO_EXPIRY == EMQX_RETRY_NO_EXPIRY && RT_MAX_INTERVAL == EMQX_RETRY_MAX_INTERVAL &&
                  RT_MAX_NOW == EMQX_RETRY_MAX_NOW && RT_TS_SHIFT == EMQX_RETRY_STAMP_TS_SHIFT && RT_DUP == EMQX_RETRY_STAMP_DUP &&
                  RT_PHASE_SHIFT == EMQX_RETRY_STAMP_PHASE_SHIFT,
              "constants");
static_assert(AK_EMPTY == EMQX_ACK_EMPTY && AK_MSG == EMQX_ACK_MSG && AK_AWAIT == EMQX_ACK_PUBREL_AWAIT && AK_OK == EMQX_A_OK &&
                  AK_NO_SESSION == EMQX_A_NO_SESSION && AK_PASS == EMQX_A_PASS && AK_PRESENT == EMQX_WINDOW_PRESENT &&
                  AK_PASSF == EMQX_WINDOW_PASS,
              "what the stage reads of the ack and the window stage");
static_assert(sizeof(emqx_ack_slot) == 8 && sizeof(emqx_retry_item) == 8 && sizeof(emqx_window_session) == 4 * AK_REC_WORDS &&
                  offsetof(emqx_window_session, inflight) == 4 * AK_REC_INFLIGHT && offsetof(emqx_window_session, flags) == 4 * AK_REC_FLAGS,
              "layout");

static_assert(EMQX_RETRY_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_retry : StageHandle {  // (stage_host.h)
  int64_t max_blocks = AK_MAX_BLOCKS, scan_chunk = AK_SCAN_BLOCK;
  uint64_t cap_boxes = 0, w = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What both calls share of their argument blocks.
struct Common {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes, sub_limit, w, now_ms;
};
Common common_of(const emqx_retry_stamp_args* b) { return {b->subs, b->n_boxes, b->m, b->cap_boxes, b->sub_limit, b->w, b->now_ms}; }
Common common_of(const emqx_retry_sweep_args* b) { return {b->subs, b->n_boxes, b->m, b->cap_boxes, b->sub_limit, b->w, b->now_ms}; }

// What every form requires of its argument block, whichever memory it points into.
bool common_ok(const Common& c) {
  if (!ak_w_ok(c.w) || c.now_ms >= RT_MAX_NOW) return false;
  if (c.cap_boxes > AK_MAX_TOTAL || c.sub_limit > MAX_SUB_LIMIT) return false;
  if (!c.n_boxes && c.m > c.cap_boxes) return false;
  return true;
}
bool batch_ok(const emqx_retry_stamp_args* b) {
  if (!b || !common_ok(common_of(b))) return false;
  if (b->sub_limit && (!b->slots || !b->stamps)) return false;
  return true;
}
bool batch_ok(const emqx_retry_sweep_args* b) {
  if (!b || !common_ok(common_of(b))) return false;
  if (b->mode != RT_MODE_RETRY && b->mode != RT_MODE_REPLAY) return false;
  if (b->interval_ms > RT_MAX_INTERVAL || b->cap_out > AK_MAX_TOTAL * 64) return false;
  if (b->sub_limit && (!b->slots || !b->sessions || (b->mode == RT_MODE_RETRY && !b->stamps))) return false;
  if (!b->out_offsets || (b->cap_out && !b->out_items)) return false;
  if (b->cap_boxes && (!b->out_status || !b->out_counts || !b->out_timers)) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, RT_S_WORDS * sizeof(uint64_t));
  if (sum[RT_S_FLAGS] & RT_F_INPUT_REFUSED) return EMQX_EINVAL;
  if (sum[RT_S_FLAGS] & RT_F_OUTPUT_FULL) return EMQX_EOVERFLOW;
  return (sum[RT_S_FLAGS] & RT_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.
bool refused(const Common& c, uint64_t m, uint64_t* sum) {
  if (m <= c.cap_boxes && m <= AK_MAX_TOTAL && (c.subs || m <= c.sub_limit)) return false;
  sum[RT_S_FLAGS] = RT_F_INPUT_REFUSED;
  sum[RT_S_BOXES] = m;
  return true;
}

// ---- the host evaluators -----------------------------------------------------------------------

int stamp_host(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  sum[RT_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = b->subs ? b->subs[k] : k;
    if (sub >= b->sub_limit) {
      sum[RT_S_FLAGS] |= RT_F_BAD_SUB;
      continue;
    }
    sum[RT_S_ROWS] += 1;
    const emqx_ack_slot* row = b->slots + sub * W;
    uint64_t* stamps = b->stamps + sub * W;
    for (uint32_t w = 0; w < W; ++w) {
      const uint64_t next = rt_stamp_next(ak_word0(row[w].pkt_id, row[w].phase, row[w].qos), stamps[w], b->now_ms);
      if (next == stamps[w]) continue;
      sum[next ? RT_T_STAMPED : RT_T_CLEARED] += 1;
      stamps[w] = next;
    }
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

int sweep_host(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  sum[RT_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w), mode = static_cast<uint32_t>(b->mode);
  // Session k: its row, or null when it is kept out of the sweep.
  auto session = [&](uint64_t k, uint64_t* sub, uint32_t* interval) -> uint8_t {
    *sub = b->subs ? b->subs[k] : k;
    *interval = 0;
    const bool ok = *sub < b->sub_limit;
    const uint8_t dead = ak_session(ok, ok ? b->sessions[*sub].flags : 0u);
    if (!dead && mode != RT_MODE_REPLAY) *interval = rt_interval(b->intervals, *sub, b->interval_ms);
    return dead;
  };
  auto stamp_at = [&](uint64_t sub, uint32_t w) -> uint64_t { return (mode == RT_MODE_REPLAY || !b->stamps) ? 0ull : b->stamps[sub * W + w]; };
  // the count pass and the scan of the device form
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; ++k) {
    uint64_t sub;
    uint32_t interval;
    b->out_offsets[k] = total;
    if (session(k, &sub, &interval)) continue;
    const emqx_ack_slot* row = b->slots + sub * W;
    for (uint32_t w = 0; w < W; ++w)
      total += rt_is_item(mode, ak_word0(row[w].pkt_id, row[w].phase, row[w].qos), stamp_at(sub, w), b->now_ms, interval) ? 1u : 0u;
  }
  b->out_offsets[m] = total;
  const bool full = total > b->cap_out;
  sum[RT_W_ITEMS] = total;
  if (full) sum[RT_S_FLAGS] |= RT_F_OUTPUT_FULL;
  // the emit pass
  std::vector<std::pair<uint64_t, uint32_t>> order;  // (key, slot index) of the row's items
  for (uint64_t k = 0; k < m; ++k) {
    uint64_t sub;
    uint32_t interval;
    const uint8_t dead = session(k, &sub, &interval);
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    b->out_status[k] = dead ? dead : AK_OK;
    b->out_timers[k] = RT_NO_TIMER;
    if (sub >= b->sub_limit) sum[RT_S_FLAGS] |= RT_F_BAD_SUB;
    if (dead) continue;
    sum[RT_S_ROWS] += 1;
    emqx_ack_slot* row = b->slots + sub * W;
    RtSlot e[64];
    uint32_t young_age = 0, entries = 0;
    order.clear();
    for (uint32_t w = 0; w < W; ++w) {
      e[w] = rt_eval(mode, ak_word0(row[w].pkt_id, row[w].phase, row[w].qos), row[w].ref, stamp_at(sub, w), b->now_ms, interval,
                     b->deadlines, b->ref_limit);
      young_age = std::max(young_age, e[w].young_age);
      entries += e[w].nonempty;
      if (e[w].kind) {
        counts[e[w].kind - 1] += 1;
        order.emplace_back(e[w].key, w);
      }
      if (e[w].unstamped) {
        sum[RT_W_UNSTAMPED] += 1;
        sum[RT_S_FLAGS] |= RT_F_UNSTAMPED;
      }
      if (e[w].bad_ref) sum[RT_S_FLAGS] |= RT_F_BAD_REF;
    }
    std::sort(order.begin(), order.end());
    emqx_window_session& rec = b->sessions[sub];
    counts[3] = ak_inflight_after(rec.inflight, counts[2]);
    b->out_timers[k] = rt_timer(mode, entries != 0, interval, young_age);
    sum[RT_W_PUBLISHES] += counts[0];
    sum[RT_W_PUBRELS] += counts[1];
    sum[RT_W_EXPIRED] += counts[2];
    if (full) continue;
    for (size_t r = 0; r < order.size(); ++r) {
      const uint32_t w = order[r].second;
      emqx_retry_item& it = b->out_items[b->out_offsets[k] + r];
      it.pkt_id = row[w].pkt_id;
      it.kind = static_cast<uint8_t>(e[w].kind);
      it.qos = row[w].qos;
      it.ref = row[w].ref;
    }
    if (mode == RT_MODE_REPLAY) continue;
    for (uint32_t w = 0; w < W; ++w) {
      if (e[w].kind == RT_EXPIRED) std::memset(&row[w], 0, sizeof(row[w]));
      b->stamps[sub * W + w] = e[w].stamp_after;
    }
    if (b->update_table) rec.inflight = counts[3];
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

#ifndef EMQX_RETRY_NO_DEVICE

// The scratch: the tile totals of a sweep; the counters with the scan's total and decision and the
// synchronous forms' summary behind them.
struct Layout {
  uint64_t tiles, ctr, bytes;
};

Layout layout_of(uint64_t cap_boxes, uint64_t w) {
  Layout l{};
  l.tiles = align256(8 * std::max<uint64_t>(rt_tiles(cap_boxes, static_cast<uint32_t>(w)), 1));
  l.ctr = align256((RT_C_WORDS + RT_S_WORDS) * sizeof(uint64_t));
  l.bytes = l.tiles + l.ctr;
  return l;
}

// Holds h->mu.  Grows the scratch.
int reserve_locked(emqx_retry* h, uint64_t cap_boxes, uint64_t w) {
  uint64_t boxes = std::max(cap_boxes, h->cap_boxes), ww = std::max(w, h->w);
  const int rc = grow_scratch(h, layout_of(boxes, ww).bytes);
  if (rc != EMQX_OK) boxes = ww = 0;  // there is no scratch any more
  h->cap_boxes = boxes;
  h->w = ww;
  return rc;
}

bool fits(emqx_retry* h, const Common& c) { return h->d_scratch && c.cap_boxes <= h->cap_boxes && c.w <= h->w; }

// The device forms move rows, stamp rows and counts 16 bytes at a time.
bool aligned_ok(const emqx_retry_stamp_args* b) { return al(b->subs, 4) && al(b->n_boxes, 8) && al(b->slots, 16) && al(b->stamps, 16); }
bool aligned_ok(const emqx_retry_sweep_args* b) {
  return al(b->subs, 4) && al(b->n_boxes, 8) && al(b->slots, 16) && al(b->stamps, 16) && al(b->sessions, 16) && al(b->intervals, 4) &&
         al(b->deadlines, 8) && al(b->out_offsets, 8) && al(b->out_items, 8) && al(b->out_counts, 16) && al(b->out_timers, 4);
}

int reserve(emqx_retry* h, uint64_t cap_boxes, uint64_t w) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_boxes > AK_MAX_TOTAL || !ak_w_ok(w)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_boxes, w);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_retry* h, const emqx_retry_stamp_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  RtStampArgs a{};
  a.subs = b->subs;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_boxes = b->cap_boxes;
  a.slots = reinterpret_cast<const uint2*>(b->slots);
  a.stamps = b->stamps;
  a.w = static_cast<uint32_t>(b->w);
  a.sub_limit = b->sub_limit;
  a.now_ms = b->now_ms;
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.tiles);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  return rt_launch_stamp(a, s);
}

int launch(emqx_retry* h, const emqx_retry_sweep_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  RtSweepArgs a{};
  a.subs = b->subs;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.slots = reinterpret_cast<uint2*>(b->slots);
  a.stamps = b->stamps;
  a.w = static_cast<uint32_t>(b->w);
  a.now_ms = b->now_ms;
  a.interval_ms = b->interval_ms;
  a.intervals = b->intervals;
  a.deadlines = b->deadlines;
  a.ref_limit = b->ref_limit;
  a.mode = static_cast<uint32_t>(b->mode);
  a.cap_out = b->cap_out;
  a.out_offsets = b->out_offsets;
  a.out_items = reinterpret_cast<uint2*>(b->out_items);
  a.out_status = b->out_status;
  a.out_counts = b->out_counts;
  a.out_timers = b->out_timers;
  a.tile_tot = reinterpret_cast<uint64_t*>(p);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.tiles);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return rt_launch_sweep(a, s);
}

struct Policy {
  static constexpr size_t WORDS = RT_S_WORDS;
  template <class B>
  static bool batch_ok(const B* b) {
    return ::batch_ok(b);
  }
  template <class B>
  static bool aligned_ok(const B* b) {
    return ::aligned_ok(b);
  }
  template <class B>
  static bool fits(emqx_retry* h, const B* b) {
    return ::fits(h, common_of(b));
  }
  template <class B>
  static int reserve(emqx_retry* h, const B* b) {
    return reserve_locked(h, b->cap_boxes, b->w);
  }
  static Layout layout(const emqx_retry* h) { return layout_of(h->cap_boxes, h->w); }
  static uint64_t* own_summary(const emqx_retry* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.tiles) + RT_C_WORDS;
  }
  template <class B>
  static int launch(emqx_retry* h, const B* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

// The rows the call names as tables of their own: session k reads row k; a subscriber the table
// does not hold becomes id m, which that table does not hold either.
struct Gathered {
  std::vector<uint32_t> subs;
  std::vector<emqx_ack_slot> rows;
  std::vector<uint64_t> stamps;
};
uint64_t sub_of(const Common& c, uint64_t k) { return c.subs ? c.subs[k] : k; }
void gather_rows(const Common& c, uint64_t m, const emqx_ack_slot* slots, const uint64_t* stamps, Gathered* g) {
  g->subs.resize(std::max<uint64_t>(m, 1));
  g->rows.assign(std::max<uint64_t>(m * c.w, 2), emqx_ack_slot{0, 0, 0, 0});
  g->stamps.assign(std::max<uint64_t>(m * c.w, 2), 0);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = sub_of(c, k);
    const bool ok = sub < c.sub_limit;
    g->subs[k] = static_cast<uint32_t>(ok ? k : m);
    if (!ok) continue;
    std::memcpy(g->rows.data() + k * c.w, slots + sub * c.w, c.w * sizeof(emqx_ack_slot));
    if (stamps) std::memcpy(g->stamps.data() + k * c.w, stamps + sub * c.w, c.w * sizeof(uint64_t));
  }
}
void scatter_rows(const Common& c, uint64_t m, emqx_ack_slot* slots, uint64_t* stamps, const Gathered& g) {
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = sub_of(c, k);
    if (sub >= c.sub_limit) continue;
    if (slots) std::memcpy(slots + sub * c.w, g.rows.data() + k * c.w, c.w * sizeof(emqx_ack_slot));
    if (stamps) std::memcpy(stamps + sub * c.w, g.stamps.data() + k * c.w, c.w * sizeof(uint64_t));
  }
}

int run_batch(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  Gathered ga;
  gather_rows(c, m, b->slots, b->stamps, &ga);
  emqx_retry_stamp_args d = *b;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_row = st.place(ga.rows.size() * 8), o_stp = st.place(ga.stamps.size() * 8);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.slots = reinterpret_cast<const emqx_ack_slot*>(D + o_row);
  d.stamps = reinterpret_cast<uint64_t*>(D + o_stp);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_row, ga.rows.data(), m * b->w * 8);
  cp.up(o_stp, ga.stamps.data(), m * b->w * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(ga.stamps.data(), o_stp, m * b->w * 8);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  scatter_rows(c, m, nullptr, b->stamps, ga);
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const bool replay = b->mode == RT_MODE_REPLAY;
  Gathered ga;
  gather_rows(c, m, b->slots, replay ? nullptr : b->stamps, &ga);
  std::vector<emqx_window_session> recs(std::max<uint64_t>(m, 1));
  std::memset(recs.data(), 0, recs.size() * sizeof(recs[0]));
  std::vector<uint32_t> ivals(std::max<uint64_t>(m, 1), 0);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = sub_of(c, k);
    if (sub >= b->sub_limit) continue;
    recs[k] = b->sessions[sub];
    if (b->intervals) ivals[k] = b->intervals[sub];
  }
  const bool expiry = b->deadlines && !replay;
  const uint64_t n_dead = expiry ? b->ref_limit : 0;
  emqx_retry_sweep_args d = *b;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(ga.subs.size() * 4), o_tab = st.place(recs.size() * 32), o_row = st.place(ga.rows.size() * 8),
                 o_stp = st.place(ga.stamps.size() * 8), o_ivl = st.place(ivals.size() * 4), o_ddl = st.place(n_dead * 8),
                 o_off = st.place((m + 1) * 8), o_itm = st.place(b->cap_out * 8), o_sta = st.place(m), o_cnt = st.place(m * 16),
                 o_tmr = st.place(m * 4);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.slots = reinterpret_cast<emqx_ack_slot*>(D + o_row);
  d.stamps = reinterpret_cast<uint64_t*>(D + o_stp);
  d.intervals = b->intervals ? reinterpret_cast<const uint32_t*>(D + o_ivl) : nullptr;
  d.deadlines = expiry ? reinterpret_cast<const uint64_t*>(D + o_ddl) : nullptr;  // (ref_limit 0: never read)
  d.out_offsets = reinterpret_cast<uint64_t*>(D + o_off);
  d.out_items = reinterpret_cast<emqx_retry_item*>(D + o_itm);
  d.out_status = D + o_sta;
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  d.out_timers = reinterpret_cast<uint32_t*>(D + o_tmr);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_tab, recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * b->w * 8);
  cp.up(o_stp, ga.stamps.data(), m * b->w * 8);
  if (b->intervals) cp.up(o_ivl, ivals.data(), m * 4);
  cp.up(o_ddl, b->deadlines, n_dead * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;  // the summary says what to bring back
  const bool full = (sum[RT_S_FLAGS] & RT_F_OUTPUT_FULL) != 0;
  const bool none = (sum[RT_S_FLAGS] & RT_F_INPUT_REFUSED) != 0;
  if (rc == EMQX_OK && !none) {
    cp.down(b->out_offsets, o_off, (m + 1) * 8);
    cp.down(b->out_status, o_sta, m);
    cp.down(b->out_counts, o_cnt, m * 16);
    cp.down(b->out_timers, o_tmr, m * 4);
    if (!full) {
      cp.down(b->out_items, o_itm, std::min<uint64_t>(sum[RT_W_ITEMS], b->cap_out) * 8);
      if (!replay) {
        cp.down(ga.rows.data(), o_row, m * b->w * 8);
        cp.down(ga.stamps.data(), o_stp, m * b->w * 8);
        cp.down(recs.data(), o_tab, m * 32);
      }
    }
    if (!cp.ok) rc = EMQX_EDEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  }
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  if (!none && !full && !replay) {
    scatter_rows(c, m, b->slots, b->stamps, ga);
    if (b->update_table) {
      for (uint64_t k = 0; k < m; ++k)
        if (sub_of(c, k) < b->sub_limit) b->sessions[sub_of(c, k)].inflight = recs[k].inflight;
    }
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

#endif  // EMQX_RETRY_NO_DEVICE

int retry_set_tuning(emqx_retry* h, const char* key, int64_t value) {
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

int retry_stats_get(emqx_retry* h, emqx_retry_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_retry_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_boxes = h->cap_boxes;
  s.w = h->w;
  s.scratch_bytes = h->scratch_bytes;
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_retry_create(int32_t device, emqx_retry** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_retry_destroy(emqx_retry* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_retry_reserve(emqx_retry* h, uint64_t cap_boxes, uint64_t w) {
  return guarded([&] { return reserve(h, cap_boxes, w); });
}
int emqx_retry_stamp_batch(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_retry_stamp_batch_device(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_retry_stamp_batch_device_async(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_retry_stamp_host(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out) {
  return guarded([&] { return stamp_host(h, b, summary_out); });
}
int emqx_retry_sweep_batch(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_retry_sweep_batch_device(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_retry_sweep_batch_device_async(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_retry_sweep_host(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out) {
  return guarded([&] { return sweep_host(h, b, summary_out); });
}
int emqx_retry_set_tuning(emqx_retry* h, const char* key, int64_t value) {
  return guarded([&] { return retry_set_tuning(h, key, value); });
}
int emqx_retry_stats_get(emqx_retry* h, emqx_retry_stats* out) {
  return guarded([&] { return retry_stats_get(h, out); });
}

}  // extern "C"
