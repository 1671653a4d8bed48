// C ABI of the delivery-options table (include/emqx_deliver.h): the writer side (a map of
// (filter, subscriber) -> options), commit (one open-addressing table, built on the host, no
// tombstones: every commit builds a fresh snapshot), the host evaluator and the batch entry
// points.  The per-delivery predicate lives in deliver.h and is the same code on both sides.
// With EMQX_DELIVER_NO_DEVICE this file compiles with a plain C++ compiler into the host-only
// part (tests/c/test_deliver_host.cpp): handles of device EMQX_DELIVER_HOST_ONLY alone.
#ifndef EMQX_DELIVER_NO_DEVICE
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/emqx_deliver.h"
#include "deliver.h"
#ifndef EMQX_DELIVER_NO_DEVICE
#include "streams.h"
#endif

using namespace emqx;

static_assert(DV_KEY_MASK == static_cast<uint32_t>(~(EMQX_FANOUT_SHARED_BIT | EMQX_FANOUT_RETRY_BIT)), "key mask");
static_assert(DV_OUT_DROP == EMQX_DELIVER_DROP_NO_LOCAL && DV_OUT_BAD == EMQX_DELIVER_BAD_MESSAGE &&
                  DV_OUT_NO_SUBOPTS == EMQX_DELIVER_NO_SUBOPTS && DV_OUT_NL == EMQX_DELIVER_NL &&
                  DV_OUT_RETAIN == EMQX_DELIVER_RETAIN,
              "output byte");
static_assert(DV_SUB_NL == EMQX_SUBOPT_NL && DV_SUB_RAP == EMQX_SUBOPT_RAP && DV_SUB_UPGRADE == EMQX_SUBOPT_UPGRADE_QOS &&
                  DV_SUB_SUBID == EMQX_SUBOPT_HAS_SUBID,
              "options word");
static_assert(DV_S_WORDS == EMQX_DELIVER_SUMMARY_WORDS && sizeof(DvSlot) == 16, "layout");

namespace {

constexpr uint64_t MAX_ENTRIES = (1ull << 31) - 1;

struct Opt {
  uint32_t opts, subid;
};

struct Snapshot {
  std::vector<DvSlot> slots;
  DvView hv{};  // into slots
  DvView dv{};  // into d_slots
  DvSlot* d_slots = nullptr;
  int device = EMQX_DELIVER_HOST_ONLY;
  uint64_t n_entries = 0;
  ~Snapshot() {
#ifndef EMQX_DELIVER_NO_DEVICE
    if (d_slots) {
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(device);
      (void)hipFree(d_slots);  // the last reference is gone: every call that read it has finished
      (void)hipSetDevice(cur);
    }
#endif
  }
};

#ifndef EMQX_DELIVER_NO_DEVICE
#define DV_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

// Per-call device scratch, one per concurrent caller.
struct Work {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  unsigned long long* d_ctr = nullptr;  // [DV_S_WORDS] counters, then [DV_S_WORDS] summary of the sync forms
  uint32_t* d_tile_kept = nullptr;
  uint64_t* d_tile_base = nullptr;
  uint64_t tiles_cap = 0;
  std::shared_ptr<Snapshot> inflight;  // an asynchronous call's snapshot, until `done`
  uint8_t* d_stage = nullptr;          // staging of the host entry point
  uint64_t stage_cap = 0;
  ~Work() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (done) (void)hipEventSynchronize(done);
    if (d_ctr) (void)hipFree(d_ctr);
    if (d_tile_kept) (void)hipFree(d_tile_kept);
    if (d_tile_base) (void)hipFree(d_tile_base);
    if (d_stage) (void)hipFree(d_stage);
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
#endif

inline uint64_t key_of(uint32_t filter, uint32_t sub) { return (static_cast<uint64_t>(filter) << 32) | sub; }

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct emqx_subopts {
  int device = EMQX_DELIVER_HOST_ONLY;
  std::mutex wmu;  // writers
  std::unordered_map<uint64_t, Opt> table;
  std::mutex smu;  // current snapshot, stats
  std::shared_ptr<Snapshot> snap;
  uint64_t epoch = 0;
  double last_build_ms = 0, last_call_ms = 0;
  std::atomic<int64_t> max_load_pct{50};
  std::atomic<int64_t> max_blocks{DV_MAX_BLOCKS};
  std::atomic<int64_t> scan_chunk{DV_SCAN_BLOCK};
#ifndef EMQX_DELIVER_NO_DEVICE
  std::mutex pmu;  // work pool
  std::vector<std::unique_ptr<Work>> pool;
#endif
};

namespace {

std::shared_ptr<Snapshot> current(emqx_subopts* h) {
  std::lock_guard<std::mutex> g(h->smu);
  return h->snap;
}

void note_call(emqx_subopts* h, double ms) {
  std::lock_guard<std::mutex> g(h->smu);
  h->last_call_ms = ms;
}

// The open-addressing table of every pair: linear probing from dv_home, the longest run recorded
// so that a lookup is bounded.
int build_snapshot(emqx_subopts* h, std::shared_ptr<Snapshot>* out) {
  auto sn = std::make_shared<Snapshot>();
  sn->device = h->device;
  const uint64_t n = h->table.size();
  if (n > MAX_ENTRIES) return EMQX_EOVERFLOW;
  const uint64_t pct = static_cast<uint64_t>(h->max_load_pct.load(std::memory_order_relaxed));
  const uint64_t n_slots = std::max<uint64_t>((n * 100 + pct - 1) / pct, n + 1);  // at least one stays empty
  sn->slots.assign(n_slots, DvSlot{DV_EMPTY, 0, 0, 0});
  uint32_t max_probe = 0;
  for (const auto& kv : h->table) {
    const uint32_t f = static_cast<uint32_t>(kv.first >> 32), s = static_cast<uint32_t>(kv.first);
    uint32_t i = dv_home(f, s, static_cast<uint32_t>(n_slots)), run = 1;
    while (sn->slots[i].filter != DV_EMPTY) {
      if (++i >= n_slots) i = 0;
      ++run;
    }
    sn->slots[i] = DvSlot{f, s, kv.second.opts, kv.second.subid};
    max_probe = std::max(max_probe, run);
  }
  sn->n_entries = n;
  sn->hv = DvView{sn->slots.data(), static_cast<uint32_t>(n_slots), max_probe};
#ifndef EMQX_DELIVER_NO_DEVICE
  if (h->device >= 0) {
    DV_TRY(hipSetDevice(h->device));
    DV_TRY(hipMalloc(reinterpret_cast<void**>(&sn->d_slots), n_slots * sizeof(DvSlot)));
    DV_TRY(hipMemcpy(sn->d_slots, sn->slots.data(), n_slots * sizeof(DvSlot), hipMemcpyHostToDevice));
    sn->dv = DvView{sn->d_slots, static_cast<uint32_t>(n_slots), max_probe};
  }
#endif
  *out = std::move(sn);
  return EMQX_OK;
}

// What every enrich form requires of its argument block, whichever memory it points into.
bool batch_ok(const emqx_deliver_batch* b) {
  if (!b || !b->offsets) return false;
  if (b->n && (!b->msg_qos || !b->msg_flags)) return false;
  if (b->cap_in && (!b->subs || !b->filters || !b->out_opts)) return false;
  if (b->kept_offsets) {
    if (b->cap_kept && (!b->kept_subs || !b->kept_filters || !b->kept_opts)) return false;
    if (b->kept_subids && !b->out_subids) return false;  // the kept subids are copies of out_subids
  }
  return true;
}

// Host buffers only: offsets[0] = 0, no decrease, offsets[n] within cap_in.
bool offsets_ok(const emqx_deliver_batch* b) {
  if (b->offsets[0] != 0) return false;
  for (uint64_t i = 0; i < b->n; ++i)
    if (b->offsets[i + 1] < b->offsets[i]) return false;
  return b->offsets[b->n] <= b->cap_in;
}

int sub_create(int32_t device, emqx_subopts** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != EMQX_DELIVER_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_DELIVER_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_subopts> h(new (std::nothrow) emqx_subopts());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
  const int rc = build_snapshot(h.get(), &h->snap);  // the empty table: every key is absent
  if (rc != EMQX_OK) return rc;
  *out = h.release();
  return EMQX_OK;
}

int sub_destroy(emqx_subopts* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_DELIVER_NO_DEVICE
  if (h->device >= 0) (void)hipSetDevice(h->device);
  h->pool.clear();
#endif
  delete h;
  return EMQX_OK;
}

int sub_set(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, const uint8_t* opts,
            const uint32_t* subids, uint64_t n) {
  if (!h || (n && (!filter_ids || !sub_ids || !opts))) return EMQX_EINVAL;
  for (uint64_t i = 0; i < n; ++i) {  // all of it is checked before any of it is applied
    const uint32_t o = opts[i];
    if (filter_ids[i] >= EMQX_DELIVER_MAX_FILTER) return EMQX_EINVAL;
    if ((o & EMQX_SUBOPT_QOS_MASK) == 3u || (o & ~0x3Fu)) return EMQX_EINVAL;
    if ((o & EMQX_SUBOPT_HAS_SUBID) && (!subids || subids[i] < 1 || subids[i] > EMQX_DELIVER_MAX_SUBID))
      return EMQX_EINVAL;
  }
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i)
    h->table[key_of(filter_ids[i], sub_ids[i])] = Opt{opts[i], (opts[i] & EMQX_SUBOPT_HAS_SUBID) ? subids[i] : 0u};
  return EMQX_OK;
}

int sub_remove(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, uint64_t n) {
  if (!h || (n && (!filter_ids || !sub_ids))) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i) h->table.erase(key_of(filter_ids[i], sub_ids[i]));
  return EMQX_OK;
}

int sub_drop_subscribers(emqx_subopts* h, const uint32_t* sub_ids, uint64_t n) {
  if (!h || (n && !sub_ids)) return EMQX_EINVAL;
  if (n == 0) return EMQX_OK;
  const std::unordered_set<uint32_t> gone(sub_ids, sub_ids + n);
  std::lock_guard<std::mutex> g(h->wmu);
  for (auto it = h->table.begin(); it != h->table.end();)  // one pass for the whole list
    it = gone.count(static_cast<uint32_t>(it->first)) ? h->table.erase(it) : std::next(it);
  return EMQX_OK;
}

int sub_commit(emqx_subopts* h) {
  if (!h) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  const auto t0 = std::chrono::steady_clock::now();
  std::shared_ptr<Snapshot> sn;
  const int rc = build_snapshot(h, &sn);
  if (rc != EMQX_OK) return rc;
  std::shared_ptr<Snapshot> old;
  {
    std::lock_guard<std::mutex> g2(h->smu);
    old = std::move(h->snap);
    h->snap = std::move(sn);
    ++h->epoch;
    h->last_build_ms = ms_since(t0);
  }
  return EMQX_OK;  // `old` is freed here unless a call in flight still holds it
}

int enrich_host(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out) {
  if (!h || !batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  uint64_t sum[DV_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  sum[DV_S_TOTAL] = b->offsets[b->n];
  for (uint64_t i = 0; i < b->n; ++i) {
    const uint32_t from = b->msg_from ? b->msg_from[i] : DV_NO_SENDER;
    for (uint64_t d = b->offsets[i]; d < b->offsets[i + 1]; ++d) {
      uint32_t subid;
      const uint32_t o = dv_enrich(sn->hv, b->subs[d], b->filters[d], b->msg_qos[i], b->msg_flags[i], from, &subid);
      b->out_opts[d] = static_cast<uint8_t>(o);
      if (b->out_subids) b->out_subids[d] = subid;
      if (o & DV_OUT_NO_SUBOPTS) ++sum[DV_S_NO_SUBOPTS];
      if (o & DV_OUT_DROP) {
        ++sum[DV_S_DROPPED];
      } else {
        ++sum[DV_S_KEPT];
        if (!(o & DV_OUT_BAD)) ++sum[DV_S_QOS0 + (o & 3u)];
      }
    }
  }
  int rc = EMQX_OK;
  if (b->kept_offsets) {
    const bool write = sum[DV_S_KEPT] <= b->cap_kept;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < b->n; ++i) {
      b->kept_offsets[i] = pos;
      for (uint64_t d = b->offsets[i]; d < b->offsets[i + 1]; ++d) {
        if (b->out_opts[d] & DV_OUT_DROP) continue;
        if (write) {
          b->kept_subs[pos] = b->subs[d];
          b->kept_filters[pos] = b->filters[d];
          b->kept_opts[pos] = b->out_opts[d];
          if (b->kept_subids) b->kept_subids[pos] = b->out_subids[d];
        }
        ++pos;
      }
    }
    b->kept_offsets[b->n] = pos;
    if (!write) {
      sum[DV_S_FLAGS] |= DV_F_KEPT_OVERFLOW;
      rc = EMQX_EOVERFLOW;
    }
  }
  if (n_kept) *n_kept = sum[DV_S_KEPT];
  if (summary_out) std::memcpy(summary_out, sum, sizeof(sum));
  note_call(h, ms_since(t0));
  return rc;
}

#ifdef EMQX_DELIVER_NO_DEVICE

int enrich_batch(emqx_subopts* h, const emqx_deliver_batch*, uint64_t*, uint64_t*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int enrich_batch_device(emqx_subopts* h, const emqx_deliver_batch*, uint64_t*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
int enrich_batch_device_async(emqx_subopts* h, const emqx_deliver_batch*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

// A scratch nobody is using: one that is idle, or one whose asynchronous call has drained (its
// event is complete); otherwise a new one.  A call never waits for another call to drain.
Work* acquire(emqx_subopts* h) {
  std::unique_ptr<Work> w;
  {
    std::lock_guard<std::mutex> g(h->pmu);
    for (auto it = h->pool.begin(); it != h->pool.end(); ++it)
      if (!(*it)->inflight || hipEventQuery((*it)->done) == hipSuccess) {
        w = std::move(*it);
        h->pool.erase(it);
        break;
      }
  }
  if (w) {
    w->inflight.reset();  // that call has drained: its snapshot may go
    return w.release();
  }
  w.reset(new (std::nothrow) Work());
  if (!w) return nullptr;
  if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&w->d_ctr), 2 * DV_S_WORDS * sizeof(unsigned long long)) != hipSuccess)
    return nullptr;
  return w.release();
}

void release(emqx_subopts* h, Work* w) {
  std::unique_ptr<Work> p(w);
  std::lock_guard<std::mutex> g(h->pmu);
  h->pool.push_back(std::move(p));
}

// Zeroes the counters on the stream and enqueues the passes.  The scratch of a call that has
// drained is free to grow: nothing on the device still reads it.
int enqueue(emqx_subopts* h, const Snapshot& sn, Work* w, const emqx_deliver_batch* b, uint64_t* summary, hipStream_t s) {
  const uint64_t tiles = (b->cap_in + DV_TILE - 1) / DV_TILE;
  if (b->kept_offsets && w->tiles_cap < tiles) {
    if (w->d_tile_kept) (void)hipFree(w->d_tile_kept);
    if (w->d_tile_base) (void)hipFree(w->d_tile_base);
    w->d_tile_kept = nullptr;
    w->d_tile_base = nullptr;
    w->tiles_cap = 0;
    const uint64_t cap = tiles + tiles / 2;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_tile_kept), cap * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&w->d_tile_base), cap * sizeof(uint64_t)) != hipSuccess)
      return EMQX_ENOMEM;
    w->tiles_cap = cap;
  }
  DvArgs a{};
  a.v = sn.dv;
  a.offsets = b->offsets;
  a.subs = b->subs;
  a.filters = b->filters;
  a.n = b->n;
  a.cap_in = b->cap_in;
  a.msg_qos = b->msg_qos;
  a.msg_flags = b->msg_flags;
  a.msg_from = b->msg_from;
  a.out_opts = b->out_opts;
  a.out_subids = b->out_subids;
  a.kept_offsets = b->kept_offsets;
  a.kept_subs = b->kept_subs;
  a.kept_filters = b->kept_filters;
  a.kept_opts = b->kept_opts;
  a.kept_subids = b->kept_subids;
  a.cap_kept = b->cap_kept;
  a.ctr = w->d_ctr;
  a.tile_kept = w->d_tile_kept;
  a.tile_base = w->d_tile_base;
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks.load(std::memory_order_relaxed));
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk.load(std::memory_order_relaxed));
  DV_TRY(hipMemsetAsync(w->d_ctr, 0, DV_S_WORDS * sizeof(unsigned long long), s));
  return dv_launch(a, s) == 0 ? EMQX_OK : EMQX_EDEVICE;
}

int enrich_batch_device_async(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !batch_ok(b)) return EMQX_EINVAL;
  DV_TRY(hipSetDevice(h->device));
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  int rc = EMQX_OK;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK) rc = enqueue(h, *sn, w, b, summary, s);
  if (hipEventRecord(w->done, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    rc = EMQX_EDEVICE;
  } else {
    w->inflight = sn;  // released when this scratch is next used, after `done`
  }
  release(h, w);
  return rc;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* n_kept, uint64_t* summary_out) {
  if (n_kept) *n_kept = sum[DV_S_KEPT];
  if (summary_out) std::memcpy(summary_out, sum, DV_S_WORDS * sizeof(uint64_t));
  if (sum[DV_S_FLAGS] & DV_F_INPUT_REFUSED) return EMQX_EINVAL;
  return (sum[DV_S_FLAGS] & DV_F_KEPT_OVERFLOW) ? EMQX_EOVERFLOW : EMQX_OK;
}

int enrich_batch_device(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out,
                        void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b)) return EMQX_EINVAL;
  DV_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + DV_S_WORDS);
  uint64_t sum[DV_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = EMQX_OK;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK) rc = enqueue(h, *sn, w, b, d_sum, s);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_kept, summary_out);
}

int enrich_batch(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b)) return EMQX_EINVAL;
  if (!offsets_ok(b)) return EMQX_EINVAL;
  DV_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  const uint64_t n = b->n, total = b->offsets[n];
  const bool compact = b->kept_offsets != nullptr;
  const uint64_t cap_kept = compact ? std::min(b->cap_kept, total) : 0;  // no more than `total` can be kept
  // staging, every section 16-byte aligned
  uint64_t at = 0;
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_off = place((n + 1) * 8), o_subs = place(total * 4), o_fil = place(total * 4), o_qos = place(n),
                 o_flags = place(n), o_from = place(b->msg_from ? n * 4 : 0), o_out = place(total),
                 o_osid = place(b->out_subids ? total * 4 : 0), o_koff = place(compact ? (n + 1) * 8 : 0),
                 o_ksubs = place(cap_kept * 4), o_kfil = place(cap_kept * 4), o_kopts = place(cap_kept),
                 o_ksid = place(b->kept_subids ? cap_kept * 4 : 0);
  const uint64_t need = std::max<uint64_t>(at, 16);
  int rc = EMQX_OK;
  if (w->stage_cap < need) {
    if (w->d_stage) (void)hipFree(w->d_stage);
    w->d_stage = nullptr;
    w->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_stage), need + need / 2) == hipSuccess) w->stage_cap = need + need / 2;
    else rc = EMQX_ENOMEM;
  }
  uint64_t sum[DV_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == EMQX_OK) {
    hipStream_t s = w->stream;
    uint8_t* D = w->d_stage;
    emqx_deliver_batch d = *b;
    d.offsets = reinterpret_cast<const uint64_t*>(D + o_off);
    d.subs = reinterpret_cast<const uint32_t*>(D + o_subs);
    d.filters = reinterpret_cast<const uint32_t*>(D + o_fil);
    d.cap_in = total;
    d.msg_qos = D + o_qos;
    d.msg_flags = D + o_flags;
    d.msg_from = b->msg_from ? reinterpret_cast<const uint32_t*>(D + o_from) : nullptr;
    d.out_opts = D + o_out;
    d.out_subids = b->out_subids ? reinterpret_cast<uint32_t*>(D + o_osid) : nullptr;
    d.kept_offsets = compact ? reinterpret_cast<uint64_t*>(D + o_koff) : nullptr;
    d.kept_subs = reinterpret_cast<uint32_t*>(D + o_ksubs);
    d.kept_filters = reinterpret_cast<uint32_t*>(D + o_kfil);
    d.kept_opts = D + o_kopts;
    d.kept_subids = b->kept_subids ? reinterpret_cast<uint32_t*>(D + o_ksid) : nullptr;
    d.cap_kept = cap_kept;
    uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + DV_S_WORDS);
    auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    };
    auto down = [&](void* dst, uint64_t o, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    bool ok = up(o_off, b->offsets, (n + 1) * 8) && up(o_subs, b->subs, total * 4) && up(o_fil, b->filters, total * 4) &&
              up(o_qos, b->msg_qos, n) && up(o_flags, b->msg_flags, n) && up(o_from, b->msg_from, b->msg_from ? n * 4 : 0);
    if (!ok) rc = EMQX_EDEVICE;
    if (rc == EMQX_OK) rc = enqueue(h, *sn, w, &d, d_sum, s);
    if (rc == EMQX_OK) {
      ok = down(b->out_opts, o_out, total) && down(b->out_subids, o_osid, b->out_subids ? total * 4 : 0) &&
           down(b->kept_offsets, o_koff, compact ? (n + 1) * 8 : 0) &&
           hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) == hipSuccess;
      if (!ok) rc = EMQX_EDEVICE;
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    if (rc == EMQX_OK && compact) {
      // the staging holds min(cap_kept, total) kept deliveries: more were kept only if the
      // caller's capacity is smaller too
      const uint64_t kept = sum[DV_S_KEPT];
      if (kept <= b->cap_kept) {
        ok = down(b->kept_subs, o_ksubs, kept * 4) && down(b->kept_filters, o_kfil, kept * 4) &&
             down(b->kept_opts, o_kopts, kept) && down(b->kept_subids, o_ksid, b->kept_subids ? kept * 4 : 0);
        if (!ok) rc = EMQX_EDEVICE;
        if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
      }
    }
  }
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_kept, summary_out);
}

#endif  // EMQX_DELIVER_NO_DEVICE

int sub_set_tuning(emqx_subopts* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  if (std::strcmp(key, "max_load_pct") == 0) {
    if (value < 10 || value > 95) return EMQX_EINVAL;
    h->max_load_pct.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    if (value < 1 || value > DV_MAX_BLOCKS) return EMQX_EINVAL;
    h->max_blocks.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "scan_chunk") == 0) {
    if (value < 1 || value > DV_SCAN_BLOCK) return EMQX_EINVAL;
    h->scan_chunk.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  return EMQX_ENOTFOUND;
}

int sub_stats_get(emqx_subopts* h, emqx_subopts_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_subopts_stats s{};
  std::lock_guard<std::mutex> g(h->smu);
  s.n_entries = h->snap->n_entries;
  s.n_slots = h->snap->hv.n_slots;
  s.table_bytes = h->snap->slots.size() * sizeof(DvSlot);
  s.epoch = h->epoch;
  s.max_probe = h->snap->hv.max_probe;
  s.last_build_ms = h->last_build_ms;
  s.last_call_ms = h->last_call_ms;
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_subopts_create(int32_t device, emqx_subopts** out) {
  return guarded([&] { return sub_create(device, out); });
}
int emqx_subopts_destroy(emqx_subopts* h) {
  return guarded([&] { return sub_destroy(h); });
}
int emqx_subopts_set(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, const uint8_t* opts,
                     const uint32_t* subids, uint64_t n) {
  return guarded([&] { return sub_set(h, filter_ids, sub_ids, opts, subids, n); });
}
int emqx_subopts_remove(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, uint64_t n) {
  return guarded([&] { return sub_remove(h, filter_ids, sub_ids, n); });
}
int emqx_subopts_drop_subscribers(emqx_subopts* h, const uint32_t* sub_ids, uint64_t n) {
  return guarded([&] { return sub_drop_subscribers(h, sub_ids, n); });
}
int emqx_subopts_commit(emqx_subopts* h) {
  return guarded([&] { return sub_commit(h); });
}
int emqx_deliver_enrich_batch(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out) {
  return guarded([&] { return enrich_batch(h, b, n_kept, summary_out); });
}
int emqx_deliver_enrich_batch_device(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept,
                                     uint64_t* summary_out, void* stream) {
  return guarded([&] { return enrich_batch_device(h, b, n_kept, summary_out, stream); });
}
int emqx_deliver_enrich_batch_device_async(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* summary,
                                           void* stream) {
  return guarded([&] { return enrich_batch_device_async(h, b, summary, stream); });
}
int emqx_deliver_enrich_host(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out) {
  return guarded([&] { return enrich_host(h, b, n_kept, summary_out); });
}
int emqx_subopts_set_tuning(emqx_subopts* h, const char* key, int64_t value) {
  return guarded([&] { return sub_set_tuning(h, key, value); });
}
int emqx_subopts_stats_get(emqx_subopts* h, emqx_subopts_stats* out) {
  return guarded([&] { return sub_stats_get(h, out); });
}

}  // extern "C"
