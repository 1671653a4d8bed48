// C ABI of the window stage (include/emqx_window.h): the handle and its device scratch, the three
// device entry points and the host evaluator.  The closed form of the session fold lives in
// window.h and is the same code on both sides.  With EMQX_WINDOW_NO_DEVICE this file compiles with
// a plain C++ compiler into the host-only part (tests/c/test_window_host.cpp): handles of device
// EMQX_WINDOW_HOST_ONLY alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_WINDOW_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/emqx_window.h"
#include "window.h"
#include "stage_host.h"

using namespace emqx;

static_assert(WN_F_INPUT_REFUSED == EMQX_WINDOW_F_INPUT_REFUSED && WN_F_BAD_SUB == EMQX_WINDOW_F_BAD_SUB, "flags");
static_assert(WN_S_WORDS == EMQX_WINDOW_SUMMARY_WORDS && sizeof(WnRec) == sizeof(emqx_window_session), "layout");
static_assert(WN_SEND_QOS0 == EMQX_W_SEND_QOS0 && WN_SEND == EMQX_W_SEND && WN_QUEUED == EMQX_W_QUEUED &&
                  WN_QUEUED_DROPPED == EMQX_W_QUEUED_DROPPED && WN_DROP_QOS0 == EMQX_W_DROP_QOS0 &&
                  WN_SKIP_NO_LOCAL == EMQX_W_SKIP_NO_LOCAL && WN_BAD_MESSAGE == EMQX_W_BAD_MESSAGE &&
                  WN_NO_SESSION == EMQX_W_NO_SESSION && WN_PASS == EMQX_W_PASS && WN_EVICTS == EMQX_W_EVICTS,
              "verdicts");
static_assert(WN_O_QOS == EMQX_DELIVER_QOS_MASK && WN_O_NO_LOCAL == EMQX_DELIVER_DROP_NO_LOCAL &&
                  WN_O_BAD == EMQX_DELIVER_BAD_MESSAGE,
              "the opts byte");
static_assert(WN_PRESENT == EMQX_WINDOW_PRESENT && WN_CONNECTED == EMQX_WINDOW_CONNECTED &&
                  WN_STORE_QOS0 == EMQX_WINDOW_STORE_QOS0 && WN_PASSF == EMQX_WINDOW_PASS,
              "record flags");

static_assert(EMQX_WINDOW_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_window : StageHandle {  // (stage_host.h)
  int64_t path = 0;
  int64_t max_blocks = WN_MAX_BLOCKS, scan_chunk = WN_SCAN_BLOCK;
  uint64_t cap_in = 0, cap_boxes = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What every form requires of its argument block, whichever memory it points into.
bool batch_ok(const emqx_window_batch* b) {
  if (!b || !b->inbox_offsets) return false;
  if (b->cap_in > WN_MAX_TOTAL || b->cap_boxes > WN_MAX_TOTAL || b->sub_limit > MAX_SUB_LIMIT) return false;
  if (b->cap_in && (!b->box_opts || !b->verdicts || !b->pkt_ids)) return false;
  if (b->cap_boxes && (!b->inbox_subs || !b->out_sessions || !b->out_counts)) return false;
  if (b->sub_limit && !b->sessions) return false;
  if (!b->n_boxes && b->m > b->cap_boxes) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, WN_S_WORDS * sizeof(uint64_t));
  return (sum[WN_S_FLAGS] & (WN_F_INPUT_REFUSED | WN_F_BAD_SUB)) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.
bool refused(const emqx_window_batch* b, uint64_t m, uint64_t* sum) {
  const bool boxes_ok = m <= b->cap_boxes && m <= WN_MAX_TOTAL;
  if (boxes_ok && b->inbox_offsets[m] <= b->cap_in && b->inbox_offsets[m] <= WN_MAX_TOTAL) return false;
  sum[WN_S_FLAGS] = WN_F_INPUT_REFUSED;
  sum[WN_S_BOXES] = m;
  sum[WN_S_TOTAL] = boxes_ok ? b->inbox_offsets[m] : 0;
  return true;
}

int run_host(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(b->inbox_offsets, m)) return EMQX_EINVAL;
  const uint64_t total = b->inbox_offsets[m];
  sum[WN_S_TOTAL] = total;
  sum[WN_S_BOXES] = m;
  const WnRec* table = reinterpret_cast<const WnRec*>(b->sessions);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t lo = b->inbox_offsets[k], hi = b->inbox_offsets[k + 1];
    uint32_t A = 0, Z = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      const uint32_t l = wn_live(b->box_opts[d]);
      A += l == 2;
      Z += l == 1;
    }
    const uint32_t sub = b->inbox_subs[k];
    const bool ok = sub < b->sub_limit;
    WnRec rec{0, 0, 0, 0, 0, 0, 0};
    if (ok) rec = table[sub];
    WnTotals t;
    const WnPlan p = wn_plan(ok, &rec, A, Z, &t);
    uint32_t a = 0, z = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      const uint8_t o = b->box_opts[d];
      b->verdicts[d] = wn_verdict(p, o, a, z, &b->pkt_ids[d]);
      const uint32_t l = wn_live(o);
      a += l == 2;
      z += l == 1;
    }
    std::memcpy(&b->out_sessions[k], &rec, sizeof(rec));
    uint32_t* c = b->out_counts + 4 * k;
    c[0] = t.sends, c[1] = t.sends0, c[2] = t.queued, c[3] = t.evicted_old;
    sum[WN_S_SENDS] += t.sends;
    sum[WN_S_SENDS0] += t.sends0;
    sum[WN_S_QUEUED] += t.queued;
    sum[WN_S_DROPS] += t.drops;
    sum[WN_S_WRAPPED] += t.wrapped;
    if (!ok) sum[WN_S_FLAGS] |= WN_F_BAD_SUB;
  }
  if (b->update_table) {  // behind every read of the table: each inbox saw the record at entry
    for (uint64_t k = 0; k < m; ++k) {
      const emqx_window_session& r = b->out_sessions[k];
      if (b->inbox_subs[k] < b->sub_limit && (r.flags & WN_PRESENT) && !(r.flags & WN_PASSF)) b->sessions[b->inbox_subs[k]] = r;
    }
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

#ifndef EMQX_WINDOW_NO_DEVICE

// The scratch of a call: the tile totals, the prefix at every inbox head (and at the end), the
// counters with the synchronous forms' summary behind them.
struct Layout {
  uint64_t tiles, heads, ctr, bytes;
};

Layout layout_of(uint64_t cap_in, uint64_t cap_boxes) {
  Layout l{};
  l.tiles = align256(8 * std::max<uint64_t>(wn_tiles(cap_in), 1));
  l.heads = align256(8 * (cap_boxes + 1));
  l.ctr = align256(2 * WN_S_WORDS * sizeof(uint64_t));
  l.bytes = l.tiles + l.heads + l.ctr;
  return l;
}

// Holds h->mu.  Grows the scratch to take cap_in deliveries and cap_boxes inboxes.
int reserve_locked(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  uint64_t cap = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes);
  const int rc = grow_scratch(h, layout_of(cap, boxes).bytes);
  if (rc != EMQX_OK) cap = boxes = 0;  // there is no scratch any more
  h->cap_in = cap;
  h->cap_boxes = boxes;
  return rc;
}

bool fits(emqx_window* h, const emqx_window_batch* b) {
  return h->d_scratch && b->cap_in <= h->cap_in && b->cap_boxes <= h->cap_boxes;
}

// The device forms move records and counts 16 bytes at a time.
bool aligned_ok(const emqx_window_batch* b) {
  return al(b->sessions, 16) && al(b->out_sessions, 16) && al(b->out_counts, 16) && al(b->inbox_offsets, 8) && al(b->n_boxes, 8) &&
         al(b->inbox_subs, 4) && al(b->pkt_ids, 2);
}

int reserve(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > WN_MAX_TOTAL || cap_boxes > WN_MAX_TOTAL) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_window* h, const emqx_window_batch* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  WnArgs a{};
  a.inbox_subs = b->inbox_subs;
  a.inbox_offsets = b->inbox_offsets;
  a.box_opts = b->box_opts;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<WnRec*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.verdicts = b->verdicts;
  a.pkt_ids = b->pkt_ids;
  a.out_sessions = reinterpret_cast<WnRec*>(b->out_sessions);
  a.out_counts = b->out_counts;
  a.tile_tot = reinterpret_cast<uint64_t*>(p);
  a.head_pre = reinterpret_cast<uint64_t*>(p + l.tiles);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.tiles + l.heads);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return wn_launch(a, static_cast<int>(h->path), s);
}

struct Policy {
  static constexpr size_t WORDS = WN_S_WORDS;
  static bool batch_ok(const emqx_window_batch* b) { return ::batch_ok(b); }
  static bool aligned_ok(const emqx_window_batch* b) { return ::aligned_ok(b); }
  static bool fits(emqx_window* h, const emqx_window_batch* b) { return ::fits(h, b); }
  static int reserve(emqx_window* h, const emqx_window_batch* b) { return reserve_locked(h, b->cap_in, b->cap_boxes); }
  static Layout layout(const emqx_window* h) { return layout_of(h->cap_in, h->cap_boxes); }
  static uint64_t* own_summary(const emqx_window* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.tiles + l.heads) + WN_S_WORDS;
  }
  static int launch(emqx_window* h, const emqx_window_batch* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

int run_batch(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m;
  {
    uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (refused(b, m, sum)) return status_of(sum, summary_out);
  }
  if (!offsets_ok(b->inbox_offsets, m)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t total = b->inbox_offsets[m];
  // the m records the inboxes name travel as a table of their own: inbox k reads record k; a
  // subscriber the table does not hold becomes id m, which that table does not hold either
  std::vector<uint32_t> subs(m);
  std::vector<emqx_window_session> recs(std::max<uint64_t>(m, 1));
  for (uint64_t k = 0; k < m; ++k) {
    const bool ok = b->inbox_subs[k] < b->sub_limit;
    subs[k] = static_cast<uint32_t>(ok ? k : m);
    if (ok) recs[k] = b->sessions[b->inbox_subs[k]];
    else std::memset(&recs[k], 0, sizeof(recs[k]));
  }
  emqx_window_batch d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  d.update_table = 0;
  if (!fits(h, &d)) {
    const int rc = reserve_locked(h, total, m);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(m * 4), o_off = st.place((m + 1) * 8), o_opt = st.place(total), o_tab = st.place(recs.size() * 32),
                 o_ver = st.place(total), o_ids = st.place(total * 2), o_rec = st.place(m * 32), o_cnt = st.place(m * 16);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.inbox_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.inbox_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.box_opts = D + o_opt;
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.verdicts = D + o_ver;
  d.pkt_ids = reinterpret_cast<uint16_t*>(D + o_ids);
  d.out_sessions = reinterpret_cast<emqx_window_session*>(D + o_rec);
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, subs.data(), m * 4);
  cp.up(o_off, b->inbox_offsets, (m + 1) * 8);
  cp.up(o_opt, b->box_opts, total);
  cp.up(o_tab, recs.data(), m * 32);
  uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(b->verdicts, o_ver, total);
    cp.down(b->pkt_ids, o_ids, total * 2);
    cp.down(b->out_sessions, o_rec, m * 32);
    cp.down(b->out_counts, o_cnt, m * 16);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  if (b->update_table) {
    for (uint64_t k = 0; k < m; ++k) {
      const emqx_window_session& r = b->out_sessions[k];
      if (b->inbox_subs[k] < b->sub_limit && (r.flags & WN_PRESENT) && !(r.flags & WN_PASSF)) b->sessions[b->inbox_subs[k]] = r;
    }
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

#endif  // EMQX_WINDOW_NO_DEVICE

int window_set_tuning(emqx_window* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t lo = 1, hi;
  if (std::strcmp(key, "path") == 0) {
    field = &h->path;
    lo = 0;
    hi = 1;
  } else if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = WN_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = WN_SCAN_BLOCK;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < lo || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int window_stats_get(emqx_window* h, emqx_window_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_window_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.cap_boxes = h->cap_boxes;
  s.scratch_bytes = h->scratch_bytes;
  s.path = static_cast<uint64_t>(h->path);
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_window_create(int32_t device, emqx_window** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_window_destroy(emqx_window* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_window_reserve(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  return guarded([&] { return reserve(h, cap_in, cap_boxes); });
}
int emqx_window_run_batch(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_window_run_batch_device(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_window_run_batch_device_async(emqx_window* h, const emqx_window_batch* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_window_run_host(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  return guarded([&] { return run_host(h, b, summary_out); });
}
int emqx_window_set_tuning(emqx_window* h, const char* key, int64_t value) {
  return guarded([&] { return window_set_tuning(h, key, value); });
}
int emqx_window_stats_get(emqx_window* h, emqx_window_stats* out) {
  return guarded([&] { return window_stats_get(h, out); });
}

}  // extern "C"
