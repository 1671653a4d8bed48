// C ABI of the route table (include/emqx_route.h): the writer side (the bag of dests per filter
// id, insertion order kept), commit (one 16-byte record per filter id, dense, built on the host:
// every commit builds and uploads a fresh snapshot), the host evaluator and the batch entry
// points.  The per-record functions live in route.h and are the same code on both sides.  With
// EMQX_ROUTE_NO_DEVICE this file compiles with a plain C++ compiler into the host-only part
// (tests/c/test_route_host.cpp): handles of device EMQX_ROUTE_HOST_ONLY alone.
#ifndef EMQX_ROUTE_NO_DEVICE
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

#include "../../include/emqx_route.h"
#include "route.h"
#ifndef EMQX_ROUTE_NO_DEVICE
#include "streams.h"
#endif

using namespace emqx;
using RouteBatch = struct emqx_route_batch;  // the plain name is the entry point

static_assert(RT_S_WORDS == EMQX_ROUTE_SUMMARY_WORDS && RT_F_FWD_OVERFLOW == EMQX_ROUTE_F_FWD_OVERFLOW &&
                  RT_F_INPUT_REFUSED == EMQX_ROUTE_F_INPUT_REFUSED && RT_NODES == EMQX_ROUTE_MAX_NODES &&
                  RT_LOCAL == EMQX_ROUTE_LOCAL && RT_SHARE == EMQX_ROUTE_SHARE && RT_REMOTE == EMQX_ROUTE_REMOTE,
              "route.h restates emqx_route.h");

namespace {

constexpr uint64_t MAX_MSGS = 0xFFFFFFFFull;  // fwd_msgs holds message indices in 32 bits

struct Dest {
  uint32_t node, group;
  bool operator==(const Dest& o) const { return node == o.node && group == o.group; }
};

struct Snapshot {
  std::vector<RtRec> recs;  // dense by filter id: [largest id with a dest + 1]
  RtRec* d_recs = nullptr;
  int device = EMQX_ROUTE_HOST_ONLY;
  uint64_t n_filters = 0, n_plain = 0, n_grouped = 0, n_nodes = 0;
  uint32_t max_fwd = 0;    // the most nodes one filter forwards to
  uint64_t fwd_nodes = 0;  // the union of the forward masks
  ~Snapshot() {
#ifndef EMQX_ROUTE_NO_DEVICE
    if (d_recs) {
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(device);
      (void)hipFree(d_recs);  // the last reference is gone: every call that read it has finished
      (void)hipSetDevice(cur);
    }
#endif
  }
};

#ifndef EMQX_ROUTE_NO_DEVICE
#define RT_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

// Per-call device scratch, one per concurrent caller.
struct Work {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  unsigned long long* d_ctr = nullptr;  // [RT_C_WORDS] counters, then [RT_S_WORDS] summary of the sync forms
  uint8_t* d_scratch = nullptr;
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

struct emqx_routetab {
  int device = EMQX_ROUTE_HOST_ONLY;
  uint32_t local = 0;
  std::mutex wmu;  // writers and lookup
  std::unordered_map<uint32_t, std::vector<Dest>> bag;  // no empty vectors
  std::mutex smu;  // current snapshot, stats
  std::shared_ptr<Snapshot> snap;
  uint64_t epoch = 0;
  double last_build_ms = 0, last_call_ms = 0;
  std::atomic<int64_t> max_blocks{16384};
  std::atomic<int64_t> scan_chunk{RT_SCAN_BLOCK};
  std::atomic<int64_t> path{0};
  std::atomic<int64_t> stored_mask{1};  // measured: level with the re-gather at 1 M slots, 8 % ahead at 10 M
#ifndef EMQX_ROUTE_NO_DEVICE
  std::mutex pmu;  // work pool
  std::vector<std::unique_ptr<Work>> pool;
#endif
};

namespace {

std::shared_ptr<Snapshot> current(emqx_routetab* h) {
  std::lock_guard<std::mutex> g(h->smu);
  return h->snap;
}

void note_call(emqx_routetab* h, double ms) {
  std::lock_guard<std::mutex> g(h->smu);
  h->last_call_ms = ms;
}

// One record per filter id up to the largest with a dest: the plain nodes as a mask, the grouped
// dests as the number of distinct groups (what aggre/1's usort leaves of them).
int build_snapshot(emqx_routetab* h, std::shared_ptr<Snapshot>* out) {
  auto sn = std::make_shared<Snapshot>();
  sn->device = h->device;
  uint64_t slots = 0;
  for (const auto& kv : h->bag) slots = std::max<uint64_t>(slots, static_cast<uint64_t>(kv.first) + 1);
  sn->recs.assign(slots, RtRec{0, 0, 0});
  uint64_t nodes_used = 0;
  std::vector<uint32_t> groups;
  for (const auto& kv : h->bag) {
    RtRec& r = sn->recs[kv.first];
    groups.clear();
    for (const Dest& d : kv.second) {
      nodes_used |= 1ull << d.node;
      if (d.group == EMQX_NO_GROUP) {
        r.node_mask |= 1ull << d.node;
        ++sn->n_plain;
      } else {
        groups.push_back(d.group);
        ++sn->n_grouped;
      }
    }
    std::sort(groups.begin(), groups.end());
    r.n_groups = static_cast<uint32_t>(std::unique(groups.begin(), groups.end()) - groups.begin());
    sn->max_fwd = std::max(sn->max_fwd, rt_popc(rt_fwd_mask(r, h->local)));
    sn->fwd_nodes |= rt_fwd_mask(r, h->local);
  }
  sn->n_filters = h->bag.size();
  sn->n_nodes = rt_popc(nodes_used);
#ifndef EMQX_ROUTE_NO_DEVICE
  if (h->device >= 0 && slots) {
    RT_TRY(hipSetDevice(h->device));
    if (hipMalloc(reinterpret_cast<void**>(&sn->d_recs), slots * sizeof(RtRec)) != hipSuccess) return EMQX_ENOMEM;
    RT_TRY(hipMemcpy(sn->d_recs, sn->recs.data(), slots * sizeof(RtRec), hipMemcpyHostToDevice));  // the one copy
  }
#endif
  *out = std::move(sn);
  return EMQX_OK;
}

// What every route form requires of its argument block, whichever memory it points into.
bool batch_ok(const RouteBatch* b) {
  if (!b || !b->offsets || !b->node_offsets) return false;
  if (b->n > MAX_MSGS || (b->n && !b->msg_routes)) return false;
  if (b->cap_in && !b->filters) return false;
  if (b->cap_fwd && (!b->fwd_msgs || !b->fwd_filters)) return false;
  if (b->local_filters && !b->local_offsets) return false;  // the pair, or neither
  if (b->local_offsets && !b->local_filters && b->cap_in) return false;
  return true;
}

// Host buffers only: offsets[0] = 0, no decrease, offsets[n] within cap_in.
bool offsets_ok(const RouteBatch* b) {
  if (b->offsets[0] != 0) return false;
  for (uint64_t i = 0; i < b->n; ++i)
    if (b->offsets[i + 1] < b->offsets[i]) return false;
  return b->offsets[b->n] <= b->cap_in;
}

bool dests_ok(const uint32_t* filter_ids, const uint32_t* nodes, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (filter_ids[i] >= EMQX_ROUTE_MAX_FILTER || nodes[i] >= EMQX_ROUTE_MAX_NODES) return false;
  return true;
}

int tab_create(int32_t device, uint32_t local_node, emqx_routetab** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if ((device < -1 && device != EMQX_ROUTE_HOST_ONLY) || local_node >= EMQX_ROUTE_MAX_NODES) return EMQX_EINVAL;
#ifdef EMQX_ROUTE_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_routetab> h(new (std::nothrow) emqx_routetab());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
  h->local = local_node;
  const int rc = build_snapshot(h.get(), &h->snap);  // the empty table: every entry has flags 0
  if (rc != EMQX_OK) return rc;
  *out = h.release();
  return EMQX_OK;
}

int tab_destroy(emqx_routetab* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_ROUTE_NO_DEVICE
  if (h->device >= 0) (void)hipSetDevice(h->device);
  h->pool.clear();
#endif
  delete h;
  return EMQX_OK;
}

int tab_add(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups, uint64_t n) {
  if (!h || (n && (!filter_ids || !nodes))) return EMQX_EINVAL;
  if (!dests_ok(filter_ids, nodes, n)) return EMQX_EINVAL;  // all of it is checked before any of it is applied
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i) {
    const Dest d{nodes[i], groups ? groups[i] : EMQX_NO_GROUP};
    std::vector<Dest>& v = h->bag[filter_ids[i]];
    if (std::find(v.begin(), v.end(), d) == v.end()) v.push_back(d);  // lists:member(Route, lookup_routes(Topic))
  }
  return EMQX_OK;
}

int tab_remove(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups, uint64_t n) {
  if (!h || (n && (!filter_ids || !nodes))) return EMQX_EINVAL;
  if (!dests_ok(filter_ids, nodes, n)) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  for (uint64_t i = 0; i < n; ++i) {
    auto it = h->bag.find(filter_ids[i]);
    if (it == h->bag.end()) continue;
    const Dest d{nodes[i], groups ? groups[i] : EMQX_NO_GROUP};
    auto at = std::find(it->second.begin(), it->second.end(), d);
    if (at == it->second.end()) continue;
    it->second.erase(at);
    if (it->second.empty()) h->bag.erase(it);
  }
  return EMQX_OK;
}

int tab_purge_node(emqx_routetab* h, uint32_t node, uint32_t* emptied, uint64_t cap, uint64_t* n_emptied) {
  if (!h || node >= EMQX_ROUTE_MAX_NODES || (cap && !emptied)) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  std::vector<uint32_t> gone;
  for (const auto& kv : h->bag) {
    bool all = true;
    for (const Dest& d : kv.second) all = all && d.node == node;
    if (all) gone.push_back(kv.first);
  }
  if (n_emptied) *n_emptied = gone.size();
  if (gone.size() > cap) return EMQX_EOVERFLOW;  // nothing is removed
  std::sort(gone.begin(), gone.end());
  for (uint64_t k = 0; k < gone.size(); ++k) {
    emptied[k] = gone[k];
    h->bag.erase(gone[k]);
  }
  for (auto& kv : h->bag) {
    std::vector<Dest>& v = kv.second;
    v.erase(std::remove_if(v.begin(), v.end(), [node](const Dest& d) { return d.node == node; }), v.end());
  }
  return EMQX_OK;
}

int tab_lookup(emqx_routetab* h, uint32_t filter_id, uint32_t* nodes_out, uint32_t* groups_out, uint64_t cap, uint64_t* n) {
  if (!h || (cap && (!nodes_out || !groups_out))) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->wmu);
  const auto it = h->bag.find(filter_id);
  const uint64_t count = it == h->bag.end() ? 0 : it->second.size();
  if (n) *n = count;
  for (uint64_t k = 0; k < std::min(count, cap); ++k) {
    nodes_out[k] = it->second[k].node;
    groups_out[k] = it->second[k].group;
  }
  return count > cap ? EMQX_EOVERFLOW : EMQX_OK;
}

int tab_commit(emqx_routetab* h) {
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

int route_host(emqx_routetab* h, const RouteBatch* b, uint64_t* n_fwd, uint64_t* summary_out) {
  if (!h || !batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  const RtRec* recs = sn->recs.data();
  const uint64_t slots = sn->recs.size(), n = b->n, total = b->offsets[n];
  const uint32_t local = h->local;
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  sum[RT_S_ENTRIES] = total;
  uint64_t count[RT_NODES + 1];
  std::fill(count, count + RT_NODES + 1, 0);
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) {  // pass 1: everything but the forward lists
    uint64_t routes = 0;
    bool fwd = false;
    if (b->local_offsets) b->local_offsets[i] = kept;
    for (uint64_t d = b->offsets[i]; d < b->offsets[i + 1]; ++d) {
      const RtRec r = rt_record(recs, slots, b->filters[d]);
      const uint32_t fl = rt_flags(r, local);
      if (b->entry_flags) b->entry_flags[d] = static_cast<uint8_t>(fl);
      routes += rt_routes(r);
      sum[RT_S_UNKNOWN] += fl == 0;
      if (fl & (RT_LOCAL | RT_SHARE)) {
        if (b->local_filters) b->local_filters[kept] = b->filters[d];
        ++kept;
      }
      uint64_t m = rt_fwd_mask(r, local);
      fwd = fwd || m != 0;
      for (; m; m &= m - 1) ++count[__builtin_ctzll(m)];
    }
    b->msg_routes[i] = static_cast<uint32_t>(routes);
    sum[RT_S_DROPPED] += routes == 0;
    sum[RT_S_FWD_MSGS] += fwd;
  }
  if (b->local_offsets) b->local_offsets[n] = kept;
  sum[RT_S_KEPT] = kept;
  uint64_t at = 0;
  for (uint32_t v = 0; v <= RT_NODES; ++v) {  // exclusive scan: the extents
    const uint64_t c = v < RT_NODES ? count[v] : 0;
    sum[RT_S_FWD_NODES] += c != 0;
    b->node_offsets[v] = at;
    count[v] = at;
    at += c;
  }
  sum[RT_S_FWD] = at;
  int rc = EMQX_OK;
  if (at > b->cap_fwd) {
    sum[RT_S_FLAGS] |= RT_F_FWD_OVERFLOW;
    rc = EMQX_EOVERFLOW;
  } else {
    for (uint64_t i = 0; i < n; ++i)  // pass 2: ascending entry position within every node
      for (uint64_t d = b->offsets[i]; d < b->offsets[i + 1]; ++d) {
        const uint32_t f = b->filters[d];
        for (uint64_t m = rt_fwd_mask(rt_record(recs, slots, f), local); m; m &= m - 1) {
          const uint64_t p = count[__builtin_ctzll(m)]++;
          b->fwd_msgs[p] = static_cast<uint32_t>(i);
          b->fwd_filters[p] = f;
        }
      }
  }
  if (n_fwd) *n_fwd = at;
  if (summary_out) std::memcpy(summary_out, sum, sizeof(sum));
  note_call(h, ms_since(t0));
  return rc;
}

#ifdef EMQX_ROUTE_NO_DEVICE

int route_batch(emqx_routetab* h, const RouteBatch*, uint64_t*, uint64_t*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int route_batch_device(emqx_routetab* h, const RouteBatch*, uint64_t*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
int route_batch_device_async(emqx_routetab* h, const RouteBatch*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

// A scratch nobody is using: one that is idle, or one whose asynchronous call has drained (its
// event is complete); otherwise a new one.  A call never waits for another call to drain.
Work* acquire(emqx_routetab* h) {
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
      hipMalloc(reinterpret_cast<void**>(&w->d_ctr), (RT_C_WORDS + RT_S_WORDS) * sizeof(unsigned long long)) != hipSuccess)
    return nullptr;
  return w.release();
}

void release(emqx_routetab* h, Work* w) {
  std::unique_ptr<Work> p(w);
  std::lock_guard<std::mutex> g(h->pmu);
  h->pool.push_back(std::move(p));
}

// Zeroes the counters on the stream and enqueues the passes.  The scratch of a call that has
// drained is free to grow: nothing on the device still reads it.
int enqueue(emqx_routetab* h, const Snapshot& sn, Work* w, const RouteBatch* b, uint64_t* summary, hipStream_t s) {
  const int path = static_cast<int>(h->path.load(std::memory_order_relaxed));
  const uint64_t tiles = rt_tiles(b->cap_in);
  if (tiles > (1ull << 40) / RT_NODES || b->cap_fwd > (1ull << 40)) return EMQX_EINVAL;
  uint64_t at = 0;
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 255) & ~255ull;
    return o;
  };
  const uint64_t o_hist = place(RT_NODES * tiles * 8), o_routes = place(tiles * 8), o_kept = place(tiles * 8),
                 o_hasfwd = place(tiles * 8), o_fwd = place(tiles * 8), o_hr = place((b->n + 1) * 8),
                 o_hk = place((b->n + 1) * 4);
  const bool stored = h->stored_mask.load(std::memory_order_relaxed) != 0;
  const uint64_t o_mask = place(stored ? b->cap_in * 8 : 0);
  const uint64_t sort_n = path == 1 ? b->cap_fwd : 0;
  const uint64_t temp_bytes = sort_n ? rt_sort_temp_bytes(sort_n) : 0;
  const uint64_t o_k0 = place(sort_n * 4), o_k1 = place(sort_n * 4), o_v0 = place(sort_n * 8), o_v1 = place(sort_n * 8),
                 o_temp = place(temp_bytes);
  const uint64_t need = std::max<uint64_t>(at, 256);
  if (w->scratch_cap < need) {
    if (w->d_scratch) (void)hipFree(w->d_scratch);
    w->d_scratch = nullptr;
    w->scratch_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_scratch), need + need / 2) != hipSuccess) return EMQX_ENOMEM;
    w->scratch_cap = need + need / 2;
  }
  uint8_t* S = w->d_scratch;
  RtArgs a{};
  a.recs = sn.d_recs;
  a.n_slots = sn.d_recs ? sn.recs.size() : 0;
  a.local = h->local;
  a.fwd_nodes = sn.fwd_nodes;
  a.offsets = b->offsets;
  a.filters = b->filters;
  a.n = b->n;
  a.cap_in = b->cap_in;
  a.entry_flags = b->entry_flags;
  a.msg_routes = b->msg_routes;
  a.node_offsets = b->node_offsets;
  a.fwd_msgs = b->fwd_msgs;
  a.fwd_filters = b->fwd_filters;
  a.cap_fwd = b->cap_fwd;
  a.local_offsets = b->local_offsets;
  a.local_filters = b->local_filters;
  a.ctr = w->d_ctr;
  a.tile_hist = reinterpret_cast<uint64_t*>(S + o_hist);
  a.tile_routes = reinterpret_cast<uint64_t*>(S + o_routes);
  a.tile_kept = reinterpret_cast<uint64_t*>(S + o_kept);
  a.tile_hasfwd = reinterpret_cast<uint64_t*>(S + o_hasfwd);
  a.tile_fwd = reinterpret_cast<uint64_t*>(S + o_fwd);
  a.head_routes = reinterpret_cast<uint64_t*>(S + o_hr);
  a.head_kf = reinterpret_cast<uint32_t*>(S + o_hk);
  a.entry_mask = stored ? reinterpret_cast<uint64_t*>(S + o_mask) : nullptr;
  a.sort_key[0] = reinterpret_cast<uint32_t*>(S + o_k0);
  a.sort_key[1] = reinterpret_cast<uint32_t*>(S + o_k1);
  a.sort_val[0] = reinterpret_cast<uint64_t*>(S + o_v0);
  a.sort_val[1] = reinterpret_cast<uint64_t*>(S + o_v1);
  a.sort_temp = S + o_temp;
  a.sort_temp_bytes = temp_bytes;
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks.load(std::memory_order_relaxed));
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk.load(std::memory_order_relaxed));
  RT_TRY(hipMemsetAsync(w->d_ctr, 0, RT_C_WORDS * sizeof(unsigned long long), s));
  return rt_launch(a, path, s) == 0 ? EMQX_OK : EMQX_EDEVICE;
}

int route_batch_device_async(emqx_routetab* h, const RouteBatch* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !batch_ok(b)) return EMQX_EINVAL;
  RT_TRY(hipSetDevice(h->device));
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
int status_of(const uint64_t* sum, uint64_t* n_fwd, uint64_t* summary_out) {
  if (n_fwd) *n_fwd = sum[RT_S_FWD];
  if (summary_out) std::memcpy(summary_out, sum, RT_S_WORDS * sizeof(uint64_t));
  if (sum[RT_S_FLAGS] & RT_F_INPUT_REFUSED) return EMQX_EINVAL;
  return (sum[RT_S_FLAGS] & RT_F_FWD_OVERFLOW) ? EMQX_EOVERFLOW : EMQX_OK;
}

int route_batch_device(emqx_routetab* h, const RouteBatch* b, uint64_t* n_fwd, uint64_t* summary_out, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b)) return EMQX_EINVAL;
  RT_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + RT_C_WORDS);
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = EMQX_OK;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK) rc = enqueue(h, *sn, w, b, d_sum, s);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_fwd, summary_out);
}

int route_batch(emqx_routetab* h, const RouteBatch* b, uint64_t* n_fwd, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  RT_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(h);
  Work* w = acquire(h);
  if (!w) return EMQX_EDEVICE;
  const uint64_t n = b->n, total = b->offsets[n];
  // no entry forwards to more nodes than the widest filter of the snapshot
  const long double bound = static_cast<long double>(total) * sn->max_fwd;
  const uint64_t cap_fwd = bound < static_cast<long double>(b->cap_fwd) ? static_cast<uint64_t>(bound) : b->cap_fwd;
  const bool want_local = b->local_offsets != nullptr;
  uint64_t at = 0;  // staging, every section 16-byte aligned
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_off = place((n + 1) * 8), o_fil = place(total * 4), o_flags = place(b->entry_flags ? total : 0),
                 o_routes = place(n * 4), o_node = place((RT_NODES + 1) * 8), o_fm = place(cap_fwd * 4),
                 o_ff = place(cap_fwd * 4), o_loff = place(want_local ? (n + 1) * 8 : 0),
                 o_lfil = place(want_local ? total * 4 : 0);
  const uint64_t need = std::max<uint64_t>(at, 16);
  int rc = EMQX_OK;
  if (w->stage_cap < need) {
    if (w->d_stage) (void)hipFree(w->d_stage);
    w->d_stage = nullptr;
    w->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_stage), need + need / 2) == hipSuccess) w->stage_cap = need + need / 2;
    else rc = EMQX_ENOMEM;
  }
  uint64_t sum[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == EMQX_OK) {
    hipStream_t s = w->stream;
    uint8_t* D = w->d_stage;
    RouteBatch d = *b;
    d.offsets = reinterpret_cast<const uint64_t*>(D + o_off);
    d.filters = reinterpret_cast<const uint32_t*>(D + o_fil);
    d.cap_in = total;
    d.entry_flags = b->entry_flags ? D + o_flags : nullptr;
    d.msg_routes = reinterpret_cast<uint32_t*>(D + o_routes);
    d.node_offsets = reinterpret_cast<uint64_t*>(D + o_node);
    d.fwd_msgs = reinterpret_cast<uint32_t*>(D + o_fm);
    d.fwd_filters = reinterpret_cast<uint32_t*>(D + o_ff);
    d.cap_fwd = cap_fwd;
    d.local_offsets = want_local ? reinterpret_cast<uint64_t*>(D + o_loff) : nullptr;
    d.local_filters = want_local ? reinterpret_cast<uint32_t*>(D + o_lfil) : nullptr;
    uint64_t* d_sum = reinterpret_cast<uint64_t*>(w->d_ctr + RT_C_WORDS);
    auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    };
    auto down = [&](void* dst, uint64_t o, uint64_t bytes) {
      return bytes == 0 || hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    if (!(up(o_off, b->offsets, (n + 1) * 8) && up(o_fil, b->filters, total * 4))) rc = EMQX_EDEVICE;
    if (rc == EMQX_OK) rc = enqueue(h, *sn, w, &d, d_sum, s);
    if (rc == EMQX_OK) {
      const bool ok = down(b->entry_flags, o_flags, b->entry_flags ? total : 0) && down(b->msg_routes, o_routes, n * 4) &&
                      down(b->node_offsets, o_node, (RT_NODES + 1) * 8) &&
                      down(b->local_offsets, o_loff, want_local ? (n + 1) * 8 : 0) &&
                      hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) == hipSuccess;
      if (!ok) rc = EMQX_EDEVICE;
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    // the staging holds min(cap_fwd, bound) forwards: there are more only if the caller's capacity is smaller too
    if (rc == EMQX_OK && !(sum[RT_S_FLAGS] & (RT_F_FWD_OVERFLOW | RT_F_INPUT_REFUSED))) {
      const bool ok = down(b->fwd_msgs, o_fm, sum[RT_S_FWD] * 4) && down(b->fwd_filters, o_ff, sum[RT_S_FWD] * 4) &&
                      down(b->local_filters, o_lfil, want_local ? sum[RT_S_KEPT] * 4 : 0);
      if (!ok) rc = EMQX_EDEVICE;
      if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    } else if (rc == EMQX_OK && !(sum[RT_S_FLAGS] & RT_F_INPUT_REFUSED)) {
      if (!down(b->local_filters, o_lfil, want_local ? sum[RT_S_KEPT] * 4 : 0)) rc = EMQX_EDEVICE;
      if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
    }
  }
  release(h, w);
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return status_of(sum, n_fwd, summary_out);
}

#endif  // EMQX_ROUTE_NO_DEVICE

int tab_set_tuning(emqx_routetab* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  if (std::strcmp(key, "max_blocks") == 0) {
    if (value < 1 || value > 16384) return EMQX_EINVAL;
    h->max_blocks.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "scan_chunk") == 0) {
    if (value < 1 || value > RT_SCAN_BLOCK) return EMQX_EINVAL;
    h->scan_chunk.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "stored_mask") == 0) {
    if (value < 0 || value > 1) return EMQX_EINVAL;
    h->stored_mask.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  if (std::strcmp(key, "path") == 0) {
    if (value < 0 || value > 1) return EMQX_EINVAL;
    h->path.store(value, std::memory_order_relaxed);
    return EMQX_OK;
  }
  return EMQX_ENOTFOUND;
}

int tab_stats_get(emqx_routetab* h, emqx_routetab_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_routetab_stats s{};
  std::lock_guard<std::mutex> g(h->smu);
  s.n_filters = h->snap->n_filters;
  s.n_plain = h->snap->n_plain;
  s.n_grouped = h->snap->n_grouped;
  s.n_nodes = h->snap->n_nodes;
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

int emqx_routetab_create(int32_t device, uint32_t local_node, emqx_routetab** out) {
  return guarded([&] { return tab_create(device, local_node, out); });
}
int emqx_routetab_destroy(emqx_routetab* h) {
  return guarded([&] { return tab_destroy(h); });
}
int emqx_routetab_add(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups,
                      uint64_t n) {
  return guarded([&] { return tab_add(h, filter_ids, nodes, groups, n); });
}
int emqx_routetab_remove(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups,
                         uint64_t n) {
  return guarded([&] { return tab_remove(h, filter_ids, nodes, groups, n); });
}
int emqx_routetab_purge_node(emqx_routetab* h, uint32_t node, uint32_t* emptied, uint64_t cap, uint64_t* n_emptied) {
  return guarded([&] { return tab_purge_node(h, node, emptied, cap, n_emptied); });
}
int emqx_routetab_lookup(emqx_routetab* h, uint32_t filter_id, uint32_t* nodes_out, uint32_t* groups_out, uint64_t cap,
                         uint64_t* n) {
  return guarded([&] { return tab_lookup(h, filter_id, nodes_out, groups_out, cap, n); });
}
int emqx_routetab_commit(emqx_routetab* h) {
  return guarded([&] { return tab_commit(h); });
}
int emqx_route_batch(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out) {
  return guarded([&] { return route_batch(h, b, n_fwd, summary_out); });
}
int emqx_route_batch_device(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out,
                            void* stream) {
  return guarded([&] { return route_batch_device(h, b, n_fwd, summary_out, stream); });
}
int emqx_route_batch_device_async(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* summary, void* stream) {
  return guarded([&] { return route_batch_device_async(h, b, summary, stream); });
}
int emqx_route_host(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out) {
  return guarded([&] { return route_host(h, b, n_fwd, summary_out); });
}
int emqx_routetab_set_tuning(emqx_routetab* h, const char* key, int64_t value) {
  return guarded([&] { return tab_set_tuning(h, key, value); });
}
int emqx_routetab_stats_get(emqx_routetab* h, emqx_routetab_stats* out) {
  return guarded([&] { return tab_stats_get(h, out); });
}

}  // extern "C"
