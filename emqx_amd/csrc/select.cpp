// C ABI of the owner table (include/emqx_select.h): the writer side (a map owner -> class,
// flags, filter ids), commit (posting lists by filter id in one blob, built on the host: every
// commit builds a fresh snapshot), the host evaluator and the batch entry points.  The per-entry
// predicate lives in select.h and is the same code on both sides.  With EMQX_SELECT_NO_DEVICE
// this file compiles with a plain C++ compiler into the host-only part
// (tests/c/test_select_host.cpp): handles of device EMQX_SELECT_HOST_ONLY alone.
#ifndef EMQX_SELECT_NO_DEVICE
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
#include <vector>

#include "../../include/emqx_select.h"
#include "select.h"
#ifndef EMQX_SELECT_NO_DEVICE
#include "streams.h"
#endif

using namespace emqx;
using SelBatch = struct emqx_select_batch;  // the plain name is the entry point

static_assert(SL_S_WORDS == EMQX_SELECT_SUMMARY_WORDS && SL_F_OUT_OVERFLOW == EMQX_SELECT_F_OUT_OVERFLOW &&
                  SL_F_INPUT_REFUSED == EMQX_SELECT_F_INPUT_REFUSED,
              "summary");

namespace {

constexpr uint64_t MAX_POSTINGS = (1ull << 31) - 1;
constexpr uint64_t SECTION_ALIGN = 256;

struct Owner {
  uint32_t class_bit, flags;
  std::vector<uint32_t> filters;  // ascending, unique
};

struct Snapshot {
  std::vector<uint8_t> blob;  // post_offsets | postings | owner_word | match_all, 256-byte aligned sections
  SlView hv{};                // into blob
  SlView dv{};                // into d_blob
  uint8_t* d_blob = nullptr;
  int device = EMQX_SELECT_HOST_ONLY;
  uint64_t n_owners = 0, n_filters = 0, max_list = 0;
  ~Snapshot() {
#ifndef EMQX_SELECT_NO_DEVICE
    if (d_blob) {
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(device);
      (void)hipFree(d_blob);  // the last reference is gone: every call that read it has finished
      (void)hipSetDevice(cur);
    }
#endif
  }
};

#ifndef EMQX_SELECT_NO_DEVICE
#define SL_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

// Per-call device scratch, one per concurrent caller.
struct Work {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  unsigned long long* d_ctr = nullptr;  // [SL_C_WORDS] counters, then [SL_S_WORDS] summary of the sync forms
  uint8_t* d_scratch = nullptr;         // entry_kept | tile_base | mtile_base | ma_before
  uint64_t scratch_cap = 0;
  std::shared_ptr<Snapshot> inflight;  // an asynchronous call's snapshot, until `done`
  uint8_t* d_stage = nullptr;          // staging of the host entry point
  uint64_t stage_cap = 0;
  ~Work() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (done) (void)hipEventSynchronize(done);
    if (d_ctr) (void)hipFree(d_ctr);
    if (d_scratch) (void)hipFree(d_scratch);
    if (d_stage) (void)hipFree(d_stage);
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
#endif

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct emqx_owntab {
  int device = EMQX_SELECT_HOST_ONLY;
  std::mutex wmu;  // writers
  std::unordered_map<uint32_t, Owner> table;
  std::mutex smu;  // current snapshot, stats
  std::shared_ptr<Snapshot> snap;
  uint64_t epoch = 0;
  double last_build_ms = 0, last_call_ms = 0;
  std::atomic<int64_t> max_blocks{16384};
  std::atomic<int64_t> scan_chunk{SL_SCAN_BLOCK};
#ifndef EMQX_SELECT_NO_DEVICE
  std::mutex pmu;  // work pool
  std::vector<std::unique_ptr<Work>> pool;
#endif
};

namespace {

std::shared_ptr<Snapshot> current(emqx_owntab* h) {
  std::lock_guard<std::mutex> g(h->smu);
  return h->snap;
}

void note_call(emqx_owntab* h, double ms) {
  std::lock_guard<std::mutex> g(h->smu);
  h->last_call_ms = ms;
}

SlView view_of(const Snapshot& sn, const uint8_t* base, const uint64_t at[4]) {
  SlView v = sn.hv;
  v.post_offsets = reinterpret_cast<const uint32_t*>(base + at[0]);
  v.postings = reinterpret_cast<const uint32_t*>(base + at[1]);
  v.owner_word = reinterpret_cast<const uint32_t*>(base + at[2]);
  v.match_all = reinterpret_cast<const uint32_t*>(base + at[3]);
  return v;
}

// Posting lists by filter id.  The owners are walked in ascending order and each owner's filter
// list is unique, so every list comes out ascending and unique.  A match-all owner gets no
// postings: it is selected for every message anyway.
int build_snapshot(emqx_owntab* h, std::shared_ptr<Snapshot>* out) {
  auto sn = std::make_shared<Snapshot>();
  sn->device = h->device;
  std::vector<uint32_t> ids;
  ids.reserve(h->table.size());
  for (const auto& kv : h->table) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  uint64_t n_filters = 0, n_postings = 0, n_match_all = 0;
  for (uint32_t o : ids) {
    const Owner& w = h->table[o];
    if (w.flags & EMQX_OWNER_MATCH_ALL) {
      ++n_match_all;
    } else if (!w.filters.empty()) {
      n_filters = std::max<uint64_t>(n_filters, static_cast<uint64_t>(w.filters.back()) + 1);
      n_postings += w.filters.size();
    }
  }
  if (n_postings > MAX_POSTINGS) return EMQX_EOVERFLOW;
  const uint64_t n_owners = ids.empty() ? 0 : static_cast<uint64_t>(ids.back()) + 1;
  uint64_t at[4], end = 0;
  const uint64_t words[4] = {n_filters + 1, n_postings, n_owners, n_match_all};
  for (int k = 0; k < 4; ++k) {
    at[k] = end;
    end += (words[k] * 4 + SECTION_ALIGN - 1) / SECTION_ALIGN * SECTION_ALIGN;
  }
  sn->blob.assign(std::max<uint64_t>(end, SECTION_ALIGN), 0);
  uint32_t* po = reinterpret_cast<uint32_t*>(sn->blob.data() + at[0]);
  uint32_t* postings = reinterpret_cast<uint32_t*>(sn->blob.data() + at[1]);
  uint32_t* owner_word = reinterpret_cast<uint32_t*>(sn->blob.data() + at[2]);
  uint32_t* match_all = reinterpret_cast<uint32_t*>(sn->blob.data() + at[3]);
  SlView& v = sn->hv;
  v.n_filters = static_cast<uint32_t>(n_filters);
  v.n_postings = static_cast<uint32_t>(n_postings);
  v.n_owners = static_cast<uint32_t>(n_owners);
  v.n_match_all = static_cast<uint32_t>(n_match_all);
  uint32_t k_all = 0;
  for (uint32_t o : ids) {  // counts, one slot up: po[f + 1] = |list of f|
    const Owner& w = h->table[o];
    const bool on = w.flags & EMQX_OWNER_ENABLED;
    owner_word[o] = w.class_bit | (on ? SL_W_ENABLED : 0u);
    if (w.flags & EMQX_OWNER_MATCH_ALL) {
      match_all[k_all++] = o;
      if (on) ++v.ma_class[w.class_bit];
    } else {
      for (uint32_t f : w.filters) ++po[f + 1];
    }
  }
  uint64_t used = 0, max_list = 0;
  for (uint64_t f = 0; f < n_filters; ++f) {
    used += po[f + 1] != 0;
    max_list = std::max<uint64_t>(max_list, po[f + 1]);
    po[f + 1] += po[f];
  }
  std::vector<uint32_t> fill(po, po + n_filters);
  for (uint32_t o : ids) {
    const Owner& w = h->table[o];
    if (w.flags & EMQX_OWNER_MATCH_ALL) continue;
    for (uint32_t f : w.filters) postings[fill[f]++] = o;
  }
  sn->n_owners = ids.size();
  sn->n_filters = used;
  sn->max_list = max_list;
  v = view_of(*sn, sn->blob.data(), at);
#ifndef EMQX_SELECT_NO_DEVICE
  if (h->device >= 0) {
    SL_TRY(hipSetDevice(h->device));
    SL_TRY(hipMalloc(reinterpret_cast<void**>(&sn->d_blob), sn->blob.size()));
    SL_TRY(hipMemcpy(sn->d_blob, sn->blob.data(), sn->blob.size(), hipMemcpyHostToDevice));  // the one copy
    sn->dv = view_of(*sn, sn->d_blob, at);
  }
#endif
  *out = std::move(sn);
  return EMQX_OK;
}

// What every select form requires of its argument block, whichever memory it points into.
bool batch_ok(const SelBatch* b) {
  if (!b || !b->offsets || !b->out_offsets) return false;
  if (b->cap_in && !b->filters) return false;
  if (b->cap_out && !b->out_owners) return false;
  return true;
}

// Host buffers only: offsets[0] = 0, no decrease, offsets[n] within cap_in.
bool offsets_ok(const SelBatch* b) {
  if (b->offsets[0] != 0) return false;
  for (uint64_t i = 0; i < b->n; ++i)
    if (b->offsets[i + 1] < b->offsets[i]) return false;
  return b->offsets[b->n] <= b->cap_in;
}

int own_create(int32_t device, emqx_owntab** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != EMQX_SELECT_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_SELECT_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_owntab> h(new (std::nothrow) emqx_owntab());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
  const int rc = build_snapshot(h.get(), &h->snap);  // the empty table: nothing is selected
  if (rc != EMQX_OK) return rc;
  *out = h.release();
  return EMQX_OK;
}

int own_destroy(emqx_owntab* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_SELECT_NO_DEVICE
  if (h->device >= 0) (void)hipSetDevice(h->device);
  h->pool.clear();
#endif
  delete h;
  return EMQX_OK;
}

int own_set(emqx_owntab* h, uint32_t owner, uint32_t class_bit, uint32_t flags, const uint32_t* filter_ids, uint64_t n) {
  if (!h || (n && !filter_ids)) return EMQX_EINVAL;
  if (owner >= EMQX_SELECT_MAX_OWNER || class_bit >= SL_CLASSES || (flags & ~(EMQX_OWNER_ENABLED | EMQX_OWNER_MATCH_ALL)))
    return EMQX_EINVAL;
  for (uint64_t i = 0; i < n; ++i)  // all of it is checked before any of it is applied
    if (filter_ids[i] >= EMQX_SELECT_MAX_FILTER) return EMQX_EINVAL;
  Owner w{class_bit, flags, std::vector<uint32_t>(filter_ids, filter_ids + n)};
  std::sort(w.filters.begin(), w.filters.end());
  w.filters.erase(std::unique(w.filters.begin(), w.filters.end()), w.filters.end());
  std::lock_guard<std::mutex> g(h->wmu);
  h->table[owner] = std::move(w);
  return EMQX_OK;
}

int own_enable(emqx_owntab* h, const uint32_t* owners, uint64_t n, int32_t on) {
  if (!h || (n && !owners)) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i) {
    auto it = h->table.find(owners[i]);
    if (it == h->table.end()) continue;
    it->second.flags = on ? (it->second.flags | EMQX_OWNER_ENABLED) : (it->second.flags & ~EMQX_OWNER_ENABLED);
  }
  return EMQX_OK;
}

int own_remove(emqx_owntab* h, const uint32_t* owners, uint64_t n) {
  if (!h || (n && !owners)) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i) h->table.erase(owners[i]);
  return EMQX_OK;
}

int own_commit(emqx_owntab* h) {
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

int select_host(emqx_owntab* h, const SelBatch* b, uint64_t* n_out, uint64_t* summary_out) {
  if (!h || !batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  const SlView& v = sn->hv;
  uint64_t sum[SL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  sum[SL_S_ENTRIES] = b->offsets[b->n];
  std::vector<uint32_t> owners;  // copied out only when the whole of it fits
  std::vector<uint32_t> room;
  for (uint64_t i = 0; i < b->n; ++i) {
    const uint32_t mask = b->msg_classes ? b->msg_classes[i] : EMQX_SELECT_ALL_CLASSES;
    const uint64_t at = owners.size();
    b->out_offsets[i] = at;
    const uint32_t all = sl_match_all_count(v, mask);
    owners.resize(at + all);
    (void)sl_match_all(v, mask, owners.data() + at, all);
    const uint64_t s = b->offsets[i];
    for (uint64_t d = s; d < b->offsets[i + 1]; ++d) {
      const uint32_t f = b->filters[d];
      room.resize(f < v.n_filters ? v.post_offsets[f + 1] - v.post_offsets[f] : 0);
      const SlCount c = sl_entry(v, b->filters, s, d, mask, room.data(), room.size());
      owners.insert(owners.end(), room.begin(), room.begin() + c.kept);
      sum[SL_S_POSTINGS] += c.examined;
      sum[SL_S_DUPS] += c.dups;
      sum[SL_S_UNKNOWN] += c.unknown;
    }
    const uint64_t count = owners.size() - at;
    sum[SL_S_MESSAGES] += count != 0;
    sum[SL_S_MAX] = std::max(sum[SL_S_MAX], count);
  }
  b->out_offsets[b->n] = owners.size();
  sum[SL_S_SELECTED] = owners.size();
  int rc = EMQX_OK;
  if (owners.size() > b->cap_out) {
    sum[SL_S_FLAGS] |= SL_F_OUT_OVERFLOW;
    rc = EMQX_EOVERFLOW;
  } else if (!owners.empty()) {
    std::memcpy(b->out_owners, owners.data(), owners.size() * sizeof(uint32_t));
  }
  if (n_out) *n_out = owners.size();
  if (summary_out) std::memcpy(summary_out, sum, sizeof(sum));
  note_call(h, ms_since(t0));
  return rc;
}

#ifdef EMQX_SELECT_NO_DEVICE

int select_batch(emqx_owntab* h, const SelBatch*, uint64_t*, uint64_t*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int select_batch_device(emqx_owntab* h, const SelBatch*, uint64_t*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
int select_batch_device_async(emqx_owntab* h, const SelBatch*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

// A scratch nobody is using: one that is idle, or one whose asynchronous call has drained (its
// event is complete); otherwise a new one.  A call never waits for another call to drain.
Work* acquire(emqx_owntab* h) {
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
      hipMalloc(reinterpret_cast<void**>(&w->d_ctr), (SL_C_WORDS + SL_S_WORDS) * sizeof(unsigned long long)) != hipSuccess)
    return nullptr;
  return w.release();
}

void release(emqx_owntab* h, Work* w) {
  std::unique_ptr<Work> p(w);
  std::lock_guard<std::mutex> g(h->pmu);
  h->pool.push_back(std::move(p));
}

// Zeroes the counters on the stream and enqueues the passes.  The scratch of a call that has
// drained is free to grow: nothing on the device still reads it.
int enqueue(emqx_owntab* h, const Snapshot& sn, Work* w, const SelBatch* b, uint64_t* summary, hipStream_t s) {
  const uint64_t tiles = (b->cap_in + SL_TILE - 1) / SL_TILE, mtiles = (b->n + 1 + SL_TILE - 1) / SL_TILE;
  if (mtiles > 0x7FFFFFFFull || tiles > (1ull << 40)) return EMQX_EINVAL;
  uint64_t at = 0;
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_kept = place(b->cap_in * 4), o_tile = place(tiles * 8), o_mtile = place(mtiles * 8),
                 o_before = place(b->n * 8);
  const uint64_t need = std::max<uint64_t>(at, 16);
  if (w->scratch_cap < need) {
    if (w->d_scratch) (void)hipFree(w->d_scratch);
    w->d_scratch = nullptr;
    w->scratch_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_scratch), need + need / 2) != hipSuccess) return EMQX_ENOMEM;
    w->scratch_cap = need + need / 2;
  }
  SlArgs a{};
  a.v = sn.dv;
  a.offsets = b->offsets;
  a.filters = b->filters;
  a.n = b->n;
  a.cap_in = b->cap_in;
  a.msg_classes = b->msg_classes;
  a.out_offsets = b->out_offsets;
  a.out_owners = b->out_owners;
  a.cap_out = b->cap_out;
  a.ctr = w->d_ctr;
  a.entry_kept = reinterpret_cast<uint32_t*>(w->d_scratch + o_kept);
  a.tile_base = reinterpret_cast<uint64_t*>(w->d_scratch + o_tile);
  a.mtile_base = reinterpret_cast<uint64_t*>(w->d_scratch + o_mtile);
  a.ma_before = reinterpret_cast<uint64_t*>(w->d_scratch + o_before);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks.load(std::memory_order_relaxed));
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk.load(std::memory_order_relaxed));
  SL_TRY(hipMemsetAsync(w->d_ctr, 0, SL_C_WORDS * sizeof(unsigned long long), s));
  return sl_launch(a, s) == 0 ? EMQX_OK : EMQX_EDEVICE;
}

int select_batch_device_async(emqx_owntab* h, const SelBatch* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !batch_ok(b)) return EMQX_EINVAL;
  SL_TRY(hipSetDevice(h->device));
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
int status_of(const uint64_t* sum, uint64_t* n_out, uint64_t* summary_out) {
  if (n_out) *n_out = sum[SL_S_SELECTED];
  if (summary_out) std::memcpy(summary_out, sum, SL_S_WORDS * sizeof(uint64_t));
  if (sum[SL_S_FLAGS] & SL_F_INPUT_REFUSED) return EMQX_EINVAL;
  return (sum[SL_S_FLAGS] & SL_F_OUT_OVERFLOW) ? EMQX_EOVERFLOW : EMQX_OK;
}

int select_batch_device(emqx_owntab* h, const SelBatch* b, uint64_t* n_out, uint64_t* summary_out, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b)) return EMQX_EINVAL;
  SL_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + SL_C_WORDS);
  uint64_t sum[SL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = EMQX_OK;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK) rc = enqueue(h, *sn, w, b, d_sum, s);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_out, summary_out);
}

int select_batch(emqx_owntab* h, const SelBatch* b, uint64_t* n_out, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  SL_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  const uint64_t n = b->n, total = b->offsets[n];
  // no more can be selected than every match-all owner for every message and the longest list for every entry
  const long double bound = static_cast<long double>(n) * sn->hv.n_match_all + static_cast<long double>(total) * sn->max_list;
  const uint64_t cap_out = bound < static_cast<long double>(b->cap_out) ? static_cast<uint64_t>(bound) : b->cap_out;
  uint64_t at = 0;  // staging, every section 16-byte aligned
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_off = place((n + 1) * 8), o_fil = place(total * 4), o_cls = place(b->msg_classes ? n * 4 : 0),
                 o_ooff = place((n + 1) * 8), o_own = place(cap_out * 4);
  const uint64_t need = std::max<uint64_t>(at, 16);
  int rc = EMQX_OK;
  if (w->stage_cap < need) {
    if (w->d_stage) (void)hipFree(w->d_stage);
    w->d_stage = nullptr;
    w->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_stage), need + need / 2) == hipSuccess) w->stage_cap = need + need / 2;
    else rc = EMQX_ENOMEM;
  }
  uint64_t sum[SL_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == EMQX_OK) {
    hipStream_t s = w->stream;
    uint8_t* D = w->d_stage;
    SelBatch d = *b;
    d.offsets = reinterpret_cast<const uint64_t*>(D + o_off);
    d.filters = reinterpret_cast<const uint32_t*>(D + o_fil);
    d.cap_in = total;
    d.msg_classes = b->msg_classes ? reinterpret_cast<const uint32_t*>(D + o_cls) : nullptr;
    d.out_offsets = reinterpret_cast<uint64_t*>(D + o_ooff);
    d.out_owners = reinterpret_cast<uint32_t*>(D + o_own);
    d.cap_out = cap_out;
    uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + SL_C_WORDS);
    auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    };
    auto down = [&](void* dst, uint64_t o, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    bool ok = up(o_off, b->offsets, (n + 1) * 8) && up(o_fil, b->filters, total * 4) &&
              up(o_cls, b->msg_classes, b->msg_classes ? n * 4 : 0);
    if (!ok) rc = EMQX_EDEVICE;
    if (rc == EMQX_OK) rc = enqueue(h, *sn, w, &d, d_sum, s);
    if (rc == EMQX_OK) {
      ok = down(b->out_offsets, o_ooff, (n + 1) * 8) &&
           hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) == hipSuccess;
      if (!ok) rc = EMQX_EDEVICE;
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    // the staging holds min(cap_out, bound) owners: more were selected only if the caller's capacity is smaller too
    if (rc == EMQX_OK && sum[SL_S_SELECTED] <= b->cap_out && !(sum[SL_S_FLAGS] & SL_F_OUT_OVERFLOW)) {
      if (!down(b->out_owners, o_own, sum[SL_S_SELECTED] * 4)) rc = EMQX_EDEVICE;
      if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    }
  }
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_out, summary_out);
}

#endif  // EMQX_SELECT_NO_DEVICE

int own_set_tuning(emqx_owntab* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  if (std::strcmp(key, "max_blocks") == 0) {
    if (value < 1 || value > 16384) return EMQX_EINVAL;
    h->max_blocks.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "scan_chunk") == 0) {
    if (value < 1 || value > SL_SCAN_BLOCK) return EMQX_EINVAL;
    h->scan_chunk.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  return EMQX_ENOTFOUND;
}

int own_stats_get(emqx_owntab* h, emqx_owntab_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_owntab_stats s{};
  std::lock_guard<std::mutex> g(h->smu);
  s.n_owners = h->snap->n_owners;
  s.n_filters = h->snap->n_filters;
  s.n_postings = h->snap->hv.n_postings;
  s.n_match_all = h->snap->hv.n_match_all;
  s.max_list = h->snap->max_list;
  s.epoch = h->epoch;
  s.last_build_ms = h->last_build_ms;
  s.last_call_ms = h->last_call_ms;
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_owntab_create(int32_t device, emqx_owntab** out) {
  return guarded([&] { return own_create(device, out); });
}
int emqx_owntab_destroy(emqx_owntab* h) {
  return guarded([&] { return own_destroy(h); });
}
int emqx_owntab_set(emqx_owntab* h, uint32_t owner, uint32_t class_bit, uint32_t flags, const uint32_t* filter_ids,
                    uint64_t n) {
  return guarded([&] { return own_set(h, owner, class_bit, flags, filter_ids, n); });
}
int emqx_owntab_enable(emqx_owntab* h, const uint32_t* owners, uint64_t n, int32_t on) {
  return guarded([&] { return own_enable(h, owners, n, on); });
}
int emqx_owntab_remove(emqx_owntab* h, const uint32_t* owners, uint64_t n) {
  return guarded([&] { return own_remove(h, owners, n); });
}
int emqx_owntab_commit(emqx_owntab* h) {
  return guarded([&] { return own_commit(h); });
}
int emqx_select_batch(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out, uint64_t* summary_out) {
  return guarded([&] { return select_batch(h, b, n_out, summary_out); });
}
int emqx_select_batch_device(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out, uint64_t* summary_out,
                             void* stream) {
  return guarded([&] { return select_batch_device(h, b, n_out, summary_out, stream); });
}
int emqx_select_batch_device_async(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* summary, void* stream) {
  return guarded([&] { return select_batch_device_async(h, b, summary, stream); });
}
int emqx_select_host(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out, uint64_t* summary_out) {
  return guarded([&] { return select_host(h, b, n_out, summary_out); });
}
int emqx_owntab_set_tuning(emqx_owntab* h, const char* key, int64_t value) {
  return guarded([&] { return own_set_tuning(h, key, value); });
}
int emqx_owntab_stats_get(emqx_owntab* h, emqx_owntab_stats* out) {
  return guarded([&] { return own_stats_get(h, out); });
}

}  // extern "C"
