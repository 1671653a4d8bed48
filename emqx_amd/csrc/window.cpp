// C ABI of the window stage (include/emqx_window.h): the handle and its device scratch, the three
// device entry points and the host evaluator.  The closed form of the session fold lives in
// window.h and is the same code on both sides.  With EMQX_WINDOW_NO_DEVICE this file compiles with
// a plain C++ compiler into the host-only part (tests/c/test_window_host.cpp): handles of device
// EMQX_WINDOW_HOST_ONLY alone.
#ifndef EMQX_WINDOW_NO_DEVICE
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/emqx_window.h"
#include "window.h"
#ifndef EMQX_WINDOW_NO_DEVICE
#include "streams.h"
#endif

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

struct emqx_window {
  int device = EMQX_WINDOW_HOST_ONLY;
  std::mutex mu;  // the calls of a handle, its scratch and its stats
  int64_t path = 0;
  int64_t max_blocks = WN_MAX_BLOCKS, scan_chunk = WN_SCAN_BLOCK;
  uint64_t calls = 0;
  double last_call_ms = 0;
  uint64_t cap_in = 0, cap_boxes = 0, scratch_bytes = 0;  // what the scratch takes
#ifndef EMQX_WINDOW_NO_DEVICE
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // behind the last call enqueued
  bool inflight = false;
  uint8_t* d_scratch = nullptr;
  uint8_t* d_stage = nullptr;  // staging of the host entry point
  uint64_t stage_cap = 0;
#endif
};

namespace {

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

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

// Host buffers only: the inbox count, inbox_offsets[0] = 0, no decrease.
bool offsets_ok(const emqx_window_batch* b, uint64_t m) {
  if (b->inbox_offsets[0] != 0) return false;
  for (uint64_t k = 0; k < m; ++k)
    if (b->inbox_offsets[k + 1] < b->inbox_offsets[k]) return false;
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

void note_call(emqx_window* h, double ms) {
  ++h->calls;
  if (ms >= 0) h->last_call_ms = ms;
}

int window_create(int32_t device, emqx_window** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != EMQX_WINDOW_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_WINDOW_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_window> h(new (std::nothrow) emqx_window());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
#ifndef EMQX_WINDOW_NO_DEVICE
  if (device >= 0) {
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->done, hipEventDisableTiming) != hipSuccess) {
      if (h->stream) (void)hipStreamDestroy(h->stream);
      return EMQX_EDEVICE;
    }
  }
#endif
  *out = h.release();
  return EMQX_OK;
}

int window_destroy(emqx_window* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_WINDOW_NO_DEVICE
  if (h->device >= 0) {
    (void)hipSetDevice(h->device);
    if (h->inflight) (void)hipEventSynchronize(h->done);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
  }
#endif
  delete h;
  return EMQX_OK;
}

int run_host(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(b, m)) return EMQX_EINVAL;
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

#ifdef EMQX_WINDOW_NO_DEVICE

int window_reserve(emqx_window* h, uint64_t, uint64_t) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int run_batch(emqx_window* h, const emqx_window_batch*, uint64_t*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int run_batch_device(emqx_window* h, const emqx_window_batch*, uint64_t*, void*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int run_batch_device_async(emqx_window* h, const emqx_window_batch*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

#define WN_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

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

void drain(emqx_window* h) {
  if (h->inflight) (void)hipEventSynchronize(h->done);
  h->inflight = false;
}

// Holds h->mu.  Grows the scratch to take cap_in deliveries and cap_boxes inboxes.
int reserve_locked(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  const uint64_t cap = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes);
  if (h->d_scratch && cap == h->cap_in && boxes == h->cap_boxes) return EMQX_OK;
  drain(h);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  h->d_scratch = nullptr;
  h->cap_in = h->cap_boxes = h->scratch_bytes = 0;
  const Layout l = layout_of(cap, boxes);
  if (hipMalloc(reinterpret_cast<void**>(&h->d_scratch), l.bytes) != hipSuccess) return EMQX_ENOMEM;
  h->cap_in = cap;
  h->cap_boxes = boxes;
  h->scratch_bytes = l.bytes;
  return EMQX_OK;
}

bool fits(emqx_window* h, const emqx_window_batch* b) {
  return h->d_scratch && b->cap_in <= h->cap_in && b->cap_boxes <= h->cap_boxes;
}

// The device forms move records and counts 16 bytes at a time.
bool aligned_ok(const emqx_window_batch* b) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  return a16(b->sessions) && a16(b->out_sessions) && a16(b->out_counts) &&
         (reinterpret_cast<uintptr_t>(b->inbox_offsets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(b->n_boxes) & 7u) == 0 &&
         (reinterpret_cast<uintptr_t>(b->inbox_subs) & 3u) == 0 && (reinterpret_cast<uintptr_t>(b->pkt_ids) & 1u) == 0;
}

int window_reserve(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > WN_MAX_TOTAL || cap_boxes > WN_MAX_TOTAL) return EMQX_EINVAL;
  WN_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes);
}

// Holds h->mu.  Orders the call behind the handle's previous one and enqueues the passes;
// `summary` NULL: the handle's own summary words.
int enqueue(emqx_window* h, const emqx_window_batch* b, uint64_t* summary, hipStream_t s, uint64_t** d_sum_out) {
  const Layout l = layout_of(h->cap_in, h->cap_boxes);
  uint8_t* p = h->d_scratch;
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
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(p + l.tiles + l.heads) + WN_S_WORDS;
  a.summary = summary ? summary : d_sum;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  if (d_sum_out) *d_sum_out = d_sum;
  if (h->inflight) WN_TRY(hipStreamWaitEvent(s, h->done, 0));
  const int rc = wn_launch(a, static_cast<int>(h->path), s) == 0 ? EMQX_OK : EMQX_EDEVICE;
  if (hipEventRecord(h->done, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    h->inflight = false;
    return EMQX_EDEVICE;
  }
  h->inflight = true;
  return rc;
}

int run_batch_device_async(emqx_window* h, const emqx_window_batch* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !batch_ok(b) || !aligned_ok(b)) return EMQX_EINVAL;
  WN_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  if (!fits(h, b)) return EMQX_EOVERFLOW;  // nothing is enqueued
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) WN_TRY(after_null_stream(s));
  const int rc = enqueue(h, b, summary, s, nullptr);
  note_call(h, -1);
  return rc;
}

int run_batch_device(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || !aligned_ok(b)) return EMQX_EINVAL;
  WN_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  if (!fits(h, b)) {
    const int rc = reserve_locked(h, b->cap_in, b->cap_boxes);
    if (rc != EMQX_OK) return rc;
  }
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) WN_TRY(after_null_stream(s));
  uint64_t* d_sum = nullptr;
  uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = enqueue(h, b, nullptr, s, &d_sum);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const uint64_t m = b->m;
  {
    uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (refused(b, m, sum)) return status_of(sum, summary_out);
  }
  if (!offsets_ok(b, m)) return EMQX_EINVAL;
  WN_TRY(hipSetDevice(h->device));
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
  // staging, every section 16-byte aligned
  uint64_t at = 0;
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_sub = place(m * 4), o_off = place((m + 1) * 8), o_opt = place(total), o_tab = place(recs.size() * 32),
                 o_ver = place(total), o_ids = place(total * 2), o_rec = place(m * 32), o_cnt = place(m * 16);
  const uint64_t need = std::max<uint64_t>(at, 16);
  if (h->stage_cap < need) {
    drain(h);
    if (h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&h->d_stage), need + need / 2) != hipSuccess) return EMQX_ENOMEM;
    h->stage_cap = need + need / 2;
  }
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
  auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
    return bytes == 0 || hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  };
  auto down = [&](void* dst, uint64_t o, uint64_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  };
  int rc = EMQX_OK;
  if (h->inflight && hipStreamWaitEvent(s, h->done, 0) != hipSuccess) rc = EMQX_EDEVICE;  // it may read the staging
  bool ok = rc == EMQX_OK && up(o_sub, subs.data(), m * 4) && up(o_off, b->inbox_offsets, (m + 1) * 8) &&
            up(o_opt, b->box_opts, total) && up(o_tab, recs.data(), m * 32);
  if (!ok) rc = EMQX_EDEVICE;
  uint64_t* d_sum = nullptr;
  uint64_t sum[WN_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == EMQX_OK) rc = enqueue(h, &d, nullptr, s, &d_sum);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    ok = down(b->verdicts, o_ver, total) && down(b->pkt_ids, o_ids, total * 2) && down(b->out_sessions, o_rec, m * 32) &&
         down(b->out_counts, o_cnt, m * 16);
    if (!ok) rc = EMQX_EDEVICE;
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
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_window_create(int32_t device, emqx_window** out) {
  return guarded([&] { return window_create(device, out); });
}
int emqx_window_destroy(emqx_window* h) {
  return guarded([&] { return window_destroy(h); });
}
int emqx_window_reserve(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes) {
  return guarded([&] { return window_reserve(h, cap_in, cap_boxes); });
}
int emqx_window_run_batch(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_window_run_batch_device(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device(h, b, summary_out, stream); });
}
int emqx_window_run_batch_device_async(emqx_window* h, const emqx_window_batch* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async(h, b, summary, stream); });
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
