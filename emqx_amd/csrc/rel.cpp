// C ABI of the rel stage (include/emqx_rel.h): the handle and its device scratch, the device entry
// points of both calls and the host evaluators.  The step of the fold, the session classification
// and the expiry predicate live in rel.h and are the same code on both sides.  With
// EMQX_REL_NO_DEVICE this file compiles with a plain C++ compiler into the host-only part
// (tests/c/test_rel_host.cpp): handles of device EMQX_REL_HOST_ONLY alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_REL_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/emqx_rel.h"
#include "rel.h"
#include "stage_host.h"

using namespace emqx;

static_assert(RL_F_INPUT_REFUSED == EMQX_REL_F_INPUT_REFUSED && RL_F_BAD_SUB == EMQX_REL_F_BAD_SUB &&
                  RL_F_ROW_SMALL == EMQX_REL_F_ROW_SMALL && RL_F_BAD_TS == EMQX_REL_F_BAD_TS && RL_S_WORDS == EMQX_REL_SUMMARY_WORDS,
              "flags");
static_assert(RL_PUBLISH == EMQX_REL_PUBLISH && RL_PUBREL == EMQX_REL_PUBREL && RL_DIRECT == EMQX_REL_DIRECT, "kinds");
static_assert(RL_OK == EMQX_REL_OK && RL_IN_USE == EMQX_REL_IN_USE && RL_NOT_FOUND == EMQX_REL_NOT_FOUND &&
                  RL_EXCEEDED == EMQX_REL_EXCEEDED && RL_NO_SESSION == EMQX_REL_NO_SESSION && RL_PASS == EMQX_REL_PASS &&
                  RL_ROW_SMALL == EMQX_REL_ROW_SMALL && RL_BAD_KIND == EMQX_REL_BAD_KIND && RL_IDLE == EMQX_REL_IDLE,
              "verdicts");
static_assert(RL_NO_TIMEOUT == EMQX_REL_NO_TIMEOUT && RL_TS_LIMIT == EMQX_REL_TS_LIMIT && RL_MAX_W == EMQX_REL_MAX_W &&
                  RL_MAX_EVENTS + 1 == EMQX_REL_MAX_EVENTS,
              "constants");
static_assert(RL_PRESENT == EMQX_WINDOW_PRESENT && RL_CONNECTED == EMQX_WINDOW_CONNECTED && RL_PASSF == EMQX_WINDOW_PASS,
              "what the stage reads of the window stage");
static_assert(sizeof(emqx_window_session) == 4 * RL_REC_WORDS && offsetof(emqx_window_session, flags) == 4 * RL_REC_FLAGS, "layout");
static_assert(rl_entry(5, 7) == EMQX_REL_ENTRY(5, 7), "entry");

static_assert(EMQX_REL_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_rel : StageHandle {  // (stage_host.h)
  int64_t lanes = 0;
  int64_t max_blocks = RL_MAX_BLOCKS, scan_chunk = RL_SCAN_BLOCK;
  uint64_t cap_in = 0, cap_boxes = 0, w = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What both calls share of their argument blocks; an expire call has no events (cap_in 0).
struct Common {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes, sub_limit, w;
};
Common common_of(const emqx_rel_run_args* b) { return {b->ev_subs, b->n_boxes, b->m, b->cap_in, b->cap_boxes, b->sub_limit, b->w}; }
Common common_of(const emqx_rel_expire_args* b) { return {b->subs, b->n_boxes, b->m, 0, b->cap_boxes, b->sub_limit, b->w}; }

// What every form requires of its argument block, whichever memory it points into.
bool common_ok(const Common& c) {
  if (!rl_w_ok(c.w)) return false;
  if (c.cap_in > RL_MAX_TOTAL || c.cap_boxes > RL_MAX_TOTAL || c.sub_limit > MAX_SUB_LIMIT) return false;
  if (!c.n_boxes && c.m > c.cap_boxes) return false;
  return true;
}
bool batch_ok(const emqx_rel_run_args* b) {
  if (!b || !common_ok(common_of(b)) || !b->ev_offsets) return false;
  if (b->cap_boxes && !b->ev_subs) return false;
  if (b->cap_in && (!b->events || !b->verdicts || !b->out_route)) return false;
  if (b->cap_boxes && (!b->out_counts || !b->out_arm)) return false;
  if (b->sub_limit && (!b->rel || !b->sessions)) return false;
  return true;
}
bool batch_ok(const emqx_rel_expire_args* b) {
  if (!b || !common_ok(common_of(b))) return false;
  if (b->cap_boxes && (!b->out_status || !b->out_counts)) return false;
  if (b->sub_limit && (!b->rel || !b->sessions)) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, RL_S_WORDS * sizeof(uint64_t));
  return (sum[RL_S_FLAGS] & (RL_F_INPUT_REFUSED | RL_F_BAD_SUB)) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.  offsets NULL: an expire call.
bool refused(const Common& c, const uint64_t* offsets, uint64_t m, uint64_t* sum) {
  const bool boxes_ok = m <= c.cap_boxes && m <= RL_MAX_TOTAL;
  if (boxes_ok && (!offsets || (offsets[m] <= c.cap_in && offsets[m] <= RL_MAX_EVENTS))) return false;
  sum[RL_S_FLAGS] = RL_F_INPUT_REFUSED;
  sum[RL_S_BOXES] = m;
  sum[RL_S_TOTAL] = boxes_ok && offsets ? offsets[m] : 0;
  return true;
}

// ---- the host evaluators -----------------------------------------------------------------------

int run_host(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, b->ev_offsets, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(b->ev_offsets, m)) return EMQX_EINVAL;
  sum[RL_S_TOTAL] = b->ev_offsets[m];
  sum[RL_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w);
  uint64_t n_route = 0;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t lo = b->ev_offsets[k], hi = b->ev_offsets[k + 1];
    const uint32_t sub = b->ev_subs[k];
    const bool ok = sub < b->sub_limit;
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    b->out_arm[k] = 0;
    if (!ok) sum[RL_S_FLAGS] |= RL_F_BAD_SUB;
    const uint32_t limit = ok ? (b->maxes ? b->maxes[sub] : b->max_awaiting) : 0u;
    const uint8_t dead = rl_session(ok, ok ? b->sessions[sub].flags : 0u, limit, W);
    if (dead) {
      if (dead == RL_ROW_SMALL) sum[RL_S_FLAGS] |= RL_F_ROW_SMALL;
      for (uint64_t d = lo; d < hi; ++d) b->verdicts[d] = dead;
      continue;
    }
    uint64_t* row = b->rel + static_cast<uint64_t>(sub) * W;
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < W; ++w) cnt += row[w] != 0;
    for (uint64_t d = lo; d < hi; ++d) {
      const uint32_t kind = b->events[d] >> 16, id = b->events[d] & 0xFFFFu;
      uint32_t at = W;  // the lowest slot that holds the id
      for (uint32_t w = 0; w < W && at == W; ++w)
        if (rl_hit(row[w], id)) at = w;
      const uint8_t v = rl_verdict(kind, cnt, limit, at < W);
      b->verdicts[d] = v;
      if (rl_routed(kind, v)) {
        b->out_route[n_route++] = b->src ? b->src[d] : static_cast<uint32_t>(d);
        ++counts[0];
      }
      if (v == RL_OK && kind == RL_PUBLISH) {
        uint32_t free_at = 0;
        while (row[free_at] != 0) ++free_at;  // (cnt < limit <= W: there is one)
        bool bad;
        row[free_at] = rl_entry(rl_stamp(b->ts ? b->ts[d] : b->now_ms, &bad), id);
        if (bad) sum[RL_S_FLAGS] |= RL_F_BAD_TS;
        ++cnt;
        b->out_arm[k] = 1;
      } else if (v == RL_OK && kind == RL_PUBREL) {
        row[at] = 0;
        --cnt;
        ++counts[1];
      } else if (v != RL_OK) {
        ++counts[2];
        if (v != RL_BAD_KIND) sum[v == RL_IN_USE ? RL_R_IN_USE : v == RL_NOT_FOUND ? RL_R_NOT_FOUND : RL_R_EXCEEDED] += 1;
      }
    }
    counts[3] = cnt;
    sum[RL_R_ROUTED] += counts[0];
    sum[RL_R_RELEASED] += counts[1];
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

int expire_host(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, nullptr, m, sum)) return status_of(sum, summary_out);
  sum[RL_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = b->subs ? b->subs[k] : k;
    const bool ok = sub < b->sub_limit;
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!ok) sum[RL_S_FLAGS] |= RL_F_BAD_SUB;
    const uint8_t st = rl_expire_session(ok, ok ? b->sessions[sub].flags : 0u, b->channel_rule != 0);
    b->out_status[k] = st;
    if (st != RL_OK) continue;
    const uint32_t timeout = b->timeouts ? b->timeouts[sub] : b->timeout_ms;
    uint64_t* row = b->rel + sub * W;
    for (uint32_t w = 0; w < W; ++w) {
      if (rl_expired(row[w], b->now_ms, timeout)) {
        row[w] = 0;
        ++counts[0];
      } else if (row[w] != 0) {
        ++counts[1];
      }
    }
    counts[2] = counts[1] > 0;
    sum[RL_X_OK] += 1;
    sum[RL_X_EXPIRED] += counts[0];
    sum[RL_X_REMAINING] += counts[1];
    sum[RL_X_ARMED] += counts[2];
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

#ifndef EMQX_REL_NO_DEVICE

// The scratch: the tile totals of the route list, and the counters with the synchronous forms'
// summary behind them.  The fold keeps a session's row in registers: no per-session scratch.
struct Layout {
  uint64_t tiles, ctr, bytes;
};

Layout layout_of(uint64_t cap_in) {
  Layout l{};
  l.tiles = align256(4 * std::max<uint64_t>(rl_tiles(cap_in), 1));
  l.ctr = align256(2 * RL_S_WORDS * sizeof(uint64_t));
  l.bytes = l.tiles + l.ctr;
  return l;
}

// Holds h->mu.  Grows the scratch.
int reserve_locked(emqx_rel* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  uint64_t cap = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes), ww = std::max(w, h->w);
  const int rc = grow_scratch(h, layout_of(cap).bytes);
  if (rc != EMQX_OK) cap = boxes = ww = 0;  // there is no scratch any more
  h->cap_in = cap;
  h->cap_boxes = boxes;
  h->w = ww;
  return rc;
}

bool fits(emqx_rel* h, const Common& c) { return h->d_scratch && c.cap_in <= h->cap_in && c.cap_boxes <= h->cap_boxes && c.w <= h->w; }

// The device forms move rows and counts 16 bytes at a time.
bool aligned_ok(const emqx_rel_run_args* b) {
  return al(b->ev_subs, 4) && al(b->ev_offsets, 8) && al(b->n_boxes, 8) && al(b->events, 4) && al(b->ts, 8) && al(b->src, 4) &&
         al(b->sessions, 16) && al(b->rel, 16) && al(b->maxes, 4) && al(b->out_route, 4) && al(b->out_counts, 16);
}
bool aligned_ok(const emqx_rel_expire_args* b) {
  return al(b->subs, 4) && al(b->n_boxes, 8) && al(b->sessions, 16) && al(b->rel, 16) && al(b->timeouts, 4) && al(b->out_counts, 16);
}

int reserve(emqx_rel* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > RL_MAX_TOTAL || cap_boxes > RL_MAX_TOTAL || !rl_w_ok(w)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes, w);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_rel* h, const emqx_rel_run_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  RlRunArgs a{};
  a.ev_subs = b->ev_subs;
  a.ev_offsets = b->ev_offsets;
  a.events = b->events;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.ts = b->ts;
  a.src = b->src;
  a.sessions = reinterpret_cast<const uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.rel = b->rel;
  a.w = static_cast<uint32_t>(b->w);
  a.now_ms = b->now_ms;
  a.max_awaiting = b->max_awaiting;
  a.maxes = b->maxes;
  a.verdicts = b->verdicts;
  a.out_route = b->out_route;
  a.out_counts = b->out_counts;
  a.out_arm = b->out_arm;
  a.tile_tot = reinterpret_cast<uint32_t*>(p);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.bytes - l.ctr);
  a.summary = summary;
  a.lanes = rl_lanes(a.w, static_cast<uint32_t>(h->lanes));
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return rl_launch_run(a, s);
}

int launch(emqx_rel* h, const emqx_rel_expire_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  RlExpArgs a{};
  a.subs = b->subs;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<const uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.rel = b->rel;
  a.w = static_cast<uint32_t>(b->w);
  a.now_ms = b->now_ms;
  a.timeout_ms = b->timeout_ms;
  a.timeouts = b->timeouts;
  a.channel_rule = b->channel_rule;
  a.out_status = b->out_status;
  a.out_counts = b->out_counts;
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.bytes - l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  return rl_launch_expire(a, s);
}

struct Policy {
  static constexpr size_t WORDS = RL_S_WORDS;
  template <class B>
  static bool batch_ok(const B* b) {
    return ::batch_ok(b);
  }
  template <class B>
  static bool aligned_ok(const B* b) {
    return ::aligned_ok(b);
  }
  template <class B>
  static bool fits(emqx_rel* h, const B* b) {
    return ::fits(h, common_of(b));
  }
  template <class B>
  static int reserve(emqx_rel* h, const B* b) {
    const Common c = common_of(b);
    return reserve_locked(h, c.cap_in, c.cap_boxes, c.w);
  }
  static Layout layout(const emqx_rel* h) { return layout_of(h->cap_in); }
  static uint64_t* own_summary(const emqx_rel* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.bytes - l.ctr) + RL_S_WORDS;
  }
  template <class B>
  static int launch(emqx_rel* h, const B* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

// The rows, records and per-session limits the call names as tables of their own: session k reads
// row k; a subscriber the table does not hold becomes id m, which that table does not hold either.
struct Gathered {
  std::vector<uint32_t> subs, lims;
  std::vector<uint64_t> rows;
  std::vector<emqx_window_session> recs;
};
void gather(const uint32_t* subs, uint64_t m, uint64_t sub_limit, uint64_t w, const uint64_t* rel, const emqx_window_session* sessions,
            const uint32_t* lims, Gathered* g) {
  g->subs.resize(std::max<uint64_t>(m, 1));
  g->lims.assign(std::max<uint64_t>(m, 1), 0);
  g->rows.assign(std::max<uint64_t>(m * w, 2), 0);
  g->recs.resize(std::max<uint64_t>(m, 1));
  std::memset(g->recs.data(), 0, g->recs.size() * sizeof(g->recs[0]));
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = subs ? subs[k] : k;
    const bool ok = sub < sub_limit;
    g->subs[k] = static_cast<uint32_t>(ok ? k : m);
    if (!ok) continue;
    std::memcpy(g->rows.data() + k * w, rel + sub * w, w * sizeof(uint64_t));
    g->recs[k] = sessions[sub];
    if (lims) g->lims[k] = lims[sub];
  }
}
void scatter_rows(const uint32_t* subs, uint64_t m, uint64_t sub_limit, uint64_t w, uint64_t* rel, const std::vector<uint64_t>& rows) {
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = subs ? subs[k] : k;
    if (sub < sub_limit) std::memcpy(rel + sub * w, rows.data() + k * w, w * sizeof(uint64_t));
  }
}

int run_batch(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, b->ev_offsets, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(b->ev_offsets, m)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t total = b->ev_offsets[m];
  Gathered ga;
  gather(b->ev_subs, m, b->sub_limit, b->w, b->rel, b->sessions, b->maxes, &ga);
  emqx_rel_run_args d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, total, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(m * 4), o_off = st.place((m + 1) * 8), o_ev = st.place(total * 4), o_ts = st.place(total * 8),
                 o_src = st.place(total * 4), o_tab = st.place(ga.recs.size() * 32), o_row = st.place(ga.rows.size() * 8),
                 o_lim = st.place(m * 4), o_ver = st.place(total), o_rt = st.place(total * 4), o_cnt = st.place(m * 16),
                 o_arm = st.place(m);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.ev_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.ev_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.events = reinterpret_cast<const uint32_t*>(D + o_ev);
  d.ts = b->ts ? reinterpret_cast<const uint64_t*>(D + o_ts) : nullptr;
  d.src = b->src ? reinterpret_cast<const uint32_t*>(D + o_src) : nullptr;
  d.sessions = reinterpret_cast<const emqx_window_session*>(D + o_tab);
  d.rel = reinterpret_cast<uint64_t*>(D + o_row);
  d.maxes = b->maxes ? reinterpret_cast<const uint32_t*>(D + o_lim) : nullptr;
  d.verdicts = D + o_ver;
  d.out_route = reinterpret_cast<uint32_t*>(D + o_rt);
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  d.out_arm = D + o_arm;
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_off, b->ev_offsets, (m + 1) * 8);
  cp.up(o_ev, b->events, total * 4);
  if (b->ts) cp.up(o_ts, b->ts, total * 8);
  if (b->src) cp.up(o_src, b->src, total * 4);
  cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * b->w * 8);
  if (b->maxes) cp.up(o_lim, ga.lims.data(), m * 4);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK && hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;  // the summary says how much was routed
  if (rc == EMQX_OK) {
    cp.down(ga.rows.data(), o_row, m * b->w * 8);
    cp.down(b->verdicts, o_ver, total);
    cp.down(b->out_route, o_rt, std::min(sum[RL_R_ROUTED], total) * 4);
    cp.down(b->out_counts, o_cnt, m * 16);
    cp.down(b->out_arm, o_arm, m);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  scatter_rows(b->ev_subs, m, b->sub_limit, b->w, b->rel, ga.rows);
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[RL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, nullptr, m, sum)) return status_of(sum, summary_out);
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  Gathered ga;
  gather(b->subs, m, b->sub_limit, b->w, b->rel, b->sessions, b->timeouts, &ga);
  emqx_rel_expire_args d = *b;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, 0, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(m * 4), o_tab = st.place(ga.recs.size() * 32), o_row = st.place(ga.rows.size() * 8),
                 o_lim = st.place(m * 4), o_st = st.place(m), o_cnt = st.place(m * 16);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.sessions = reinterpret_cast<const emqx_window_session*>(D + o_tab);
  d.rel = reinterpret_cast<uint64_t*>(D + o_row);
  d.timeouts = b->timeouts ? reinterpret_cast<const uint32_t*>(D + o_lim) : nullptr;
  d.out_status = D + o_st;
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, ga.subs.data(), m * 4);
  cp.up(o_tab, ga.recs.data(), m * 32);
  cp.up(o_row, ga.rows.data(), m * b->w * 8);
  if (b->timeouts) cp.up(o_lim, ga.lims.data(), m * 4);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(ga.rows.data(), o_row, m * b->w * 8);
    cp.down(b->out_status, o_st, m);
    cp.down(b->out_counts, o_cnt, m * 16);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  scatter_rows(b->subs, m, b->sub_limit, b->w, b->rel, ga.rows);
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

#endif  // EMQX_REL_NO_DEVICE

int rel_set_tuning(emqx_rel* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t lo = 1, hi;
  if (std::strcmp(key, "lanes") == 0) {
    if (!rl_lanes_ok(value)) return EMQX_EINVAL;
    field = &h->lanes;
    lo = 0;
    hi = RL_MAX_LANES;
  } else if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = RL_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = RL_SCAN_BLOCK;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < lo || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int rel_stats_get(emqx_rel* h, emqx_rel_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_rel_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.cap_boxes = h->cap_boxes;
  s.w = h->w;
  s.scratch_bytes = h->scratch_bytes;
  s.lanes = static_cast<uint64_t>(h->lanes);
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_rel_create(int32_t device, emqx_rel** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_rel_destroy(emqx_rel* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_rel_reserve(emqx_rel* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  return guarded([&] { return reserve(h, cap_in, cap_boxes, w); });
}
int emqx_rel_run_batch(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_rel_run_batch_device(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_rel_run_batch_device_async(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_rel_run_host(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_host(h, b, summary_out); });
}
int emqx_rel_expire_batch(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_rel_expire_batch_device(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_rel_expire_batch_device_async(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_rel_expire_host(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out) {
  return guarded([&] { return expire_host(h, b, summary_out); });
}
int emqx_rel_set_tuning(emqx_rel* h, const char* key, int64_t value) {
  return guarded([&] { return rel_set_tuning(h, key, value); });
}
int emqx_rel_stats_get(emqx_rel* h, emqx_rel_stats* out) {
  return guarded([&] { return rel_stats_get(h, out); });
}

}  // extern "C"
