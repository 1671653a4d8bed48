// C ABI of the authorization table (include/emqx_authz.h): rule compilation
// (emqx_authz_rule:compile/1), the client table, commit (one flat snapshot, segments resolved
// per client), the host evaluator and the batch entry points.  The per-pair predicate lives in
// authz.h and is the same code on both sides.
// With EMQX_AUTHZ_NO_DEVICE this file compiles with a plain C++ compiler into the host-only
// part (tests/c/test_authz_host.cpp): handles of device EMQX_AUTHZ_HOST_ONLY alone.
#ifndef EMQX_AUTHZ_NO_DEVICE
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/emqx_authz.h"
#include "authz.h"
#include "stage_common.h"
#ifndef EMQX_AUTHZ_NO_DEVICE
#include "streams.h"
#endif

using namespace emqx;

namespace emqx {
int az_launch_check(const AzView& v, const uint32_t* clients, const uint8_t* actions, const uint8_t* tbytes,
                    const uint64_t* toffs, uint64_t n, uint8_t* verdict_out, uint32_t* tag_out,
                    unsigned long long* evals_out, uint32_t group, uint64_t offset_base, void* stream);
int az_launch_summary(const uint8_t* verdict, uint64_t n, const unsigned long long* evals, uint64_t* summary,
                      void* stream);
}  // namespace emqx

namespace {

constexpr uint32_t MAX_STR = 65535;
constexpr uint32_t MAX_CLIENT_ID = 1u << 24;  // the client tables are indexed by id
constexpr uint64_t MAX_ENTRIES = (1ull << 31) - 1;

// One compiled rule list: the snapshot's arrays with offsets relative to the list.
struct RuleList {
  std::vector<AzRule> rules;
  std::vector<AzLeaf> leaves;
  std::vector<AzRange> cidrs;
  std::vector<AzEntry> entries;
  std::vector<uint8_t> arena;
};

struct ClientRec {
  uint32_t present = 0;  // AZ_HAS_* | AZ_REGISTERED
  uint32_t ipv4 = 0;
  uint64_t flags = 0;
  std::string clientid, username;
};

using ListKey = std::tuple<uint32_t, uint32_t, std::string>;  // source, scope, key

struct Snapshot {
  std::vector<uint8_t> blob;  // every array, 256-B aligned sections
  AzView hv{};                // into blob
  AzView dv{};                // into d_blob
  uint8_t* d_blob = nullptr;
  int device = EMQX_AUTHZ_HOST_ONLY;
  uint64_t n_sources = 0, n_lists = 0, n_rules = 0, n_entries = 0, n_clients = 0;
  uint32_t max_entries = 0;  // entries of the longest request (sum of a client's segments)
  ~Snapshot() {
#ifndef EMQX_AUTHZ_NO_DEVICE
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

#ifndef EMQX_AUTHZ_NO_DEVICE
#define AZ_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

// Per-call device scratch, one per concurrent caller.
struct Work {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  unsigned long long* d_evals = nullptr;
  std::shared_ptr<Snapshot> inflight;  // an asynchronous call's snapshot, until `done`
  // staging of the host entry point
  uint8_t* d_bytes = nullptr;
  uint64_t bytes_cap = 0;
  uint8_t* d_req = nullptr;  // offsets, clients, tags, actions, verdicts of n requests
  uint64_t req_cap = 0;
  ~Work() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (done) (void)hipEventSynchronize(done);
    if (d_evals) (void)hipFree(d_evals);
    if (d_bytes) (void)hipFree(d_bytes);
    if (d_req) (void)hipFree(d_req);
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
#endif

void set_err(char* err, uint64_t cap, const char* fmt, uint64_t a = 0, uint64_t b = 0) {
  if (err && cap) std::snprintf(err, cap, fmt, static_cast<unsigned long long>(a), static_cast<unsigned long long>(b));
}

// esockd_cidr:parse(S, true) for IPv4: "a.b.c.d" is a /32; the start is masked down to the
// network, the end is the last address (emqx_authz_rule_SUITE.erl:64-72).
bool parse_cidr(const uint8_t* p, uint64_t n, AzRange* out, const char** why) {
  for (uint64_t i = 0; i < n; ++i)
    if (p[i] == ':') {
      *why = "rule %llu: an IPv6 CIDR is not supported";
      return false;
    }
  *why = "rule %llu: malformed IPv4 CIDR";
  uint64_t i = 0;
  uint32_t ip = 0;
  for (int k = 0; k < 4; ++k) {
    uint32_t x = 0, digits = 0;
    while (i < n && p[i] >= '0' && p[i] <= '9' && digits < 4) x = x * 10 + (p[i++] - '0'), ++digits;
    if (digits == 0 || digits > 3 || x > 255) return false;
    ip = (ip << 8) | x;
    if (k < 3) {
      if (i >= n || p[i] != '.') return false;
      ++i;
    }
  }
  uint32_t len = 32;
  if (i < n) {
    if (p[i] != '/') return false;
    ++i;
    uint32_t digits = 0;
    len = 0;
    while (i < n && p[i] >= '0' && p[i] <= '9' && digits < 3) len = len * 10 + (p[i++] - '0'), ++digits;
    if (digits == 0 || i != n || len > 32) return false;
  }
  const uint32_t mask = len == 0 ? 0u : 0xFFFFFFFFu << (32 - len);
  out->lo = ip & mask;
  out->hi = (ip & mask) | ~mask;
  return true;
}

// pattern/1 (emqx_authz_rule.erl:93-94): some whole level is a placeholder.
bool has_placeholder(const uint8_t* p, uint32_t n) {
  uint32_t s = 0;
  for (;;) {
    const uint32_t e = az_level_end(p, s, n);
    if (az_placeholder(p, s, e)) return true;
    if (e == n) return false;
    s = e + 1;
  }
}

}  // namespace

struct emqx_authz {
  int device = EMQX_AUTHZ_HOST_ONLY;
  std::mutex wmu;  // writers
  std::map<ListKey, RuleList> lists;
  std::vector<ClientRec> clients;
  std::mutex smu;  // current snapshot, stats
  std::shared_ptr<Snapshot> snap;
  uint64_t epoch = 0, last_evals = 0, last_group = 0;
  double last_build_ms = 0, last_check_ms = 0;
  std::atomic<int64_t> tune_group{0};  // set while checks run
#ifndef EMQX_AUTHZ_NO_DEVICE
  std::mutex pmu;  // work pool
  std::vector<std::unique_ptr<Work>> pool;
#endif
};

namespace {

std::shared_ptr<Snapshot> current(emqx_authz* a) {
  std::lock_guard<std::mutex> g(a->smu);
  return a->snap;
}

template <class T>
uint64_t place(uint64_t& at, uint64_t count) {
  const uint64_t o = at;
  at += (count * sizeof(T) + 255) & ~255ull;
  return o;
}

int build_snapshot(emqx_authz* a, std::shared_ptr<Snapshot>* out) {
  auto sn = std::make_shared<Snapshot>();
  sn->device = a->device;
  uint64_t n_rules = 0, n_leaves = 0, n_cidrs = 0, n_entries = 0, n_arena = 0;
  for (auto& kv : a->lists) {
    n_rules += kv.second.rules.size();
    n_leaves += kv.second.leaves.size();
    n_cidrs += kv.second.cidrs.size();
    n_entries += kv.second.entries.size();
    n_arena += kv.second.arena.size();
  }
  if (n_entries > MAX_ENTRIES || n_rules > MAX_ENTRIES || n_leaves > 0xFFFFFFFFull || n_cidrs > 0xFFFFFFFFull ||
      n_arena > 0xFFFFFFFFull)
    return EMQX_EOVERFLOW;
  const uint64_t n_clients = a->clients.size();
  uint64_t n_carena = 0;
  for (auto& c : a->clients) n_carena += c.clientid.size() + c.username.size();
  if (n_carena > 0xFFFFFFFFull) return EMQX_EOVERFLOW;

  uint64_t at = 0;
  const uint64_t o_entries = place<AzEntry>(at, n_entries), o_rules = place<AzRule>(at, n_rules),
                 o_leaves = place<AzLeaf>(at, n_leaves), o_cidrs = place<AzRange>(at, n_cidrs),
                 o_arena = place<uint8_t>(at, n_arena), o_clients = place<AzClient>(at, n_clients),
                 o_carena = place<uint8_t>(at, n_carena), o_segs = place<AzRange>(at, n_clients * AZ_SEG_STRIDE);
  sn->blob.assign(at + 256, 0);
  uint8_t* B = sn->blob.data();
  auto* entries = reinterpret_cast<AzEntry*>(B + o_entries);
  auto* rules = reinterpret_cast<AzRule*>(B + o_rules);
  auto* leaves = reinterpret_cast<AzLeaf*>(B + o_leaves);
  auto* cidrs = reinterpret_cast<AzRange*>(B + o_cidrs);
  uint8_t* arena = B + o_arena;
  auto* clients = reinterpret_cast<AzClient*>(B + o_clients);
  uint8_t* carena = B + o_carena;
  auto* segs = reinterpret_cast<AzRange*>(B + o_segs);

  // lists, each contiguous; where each list's entries landed
  struct Where {
    AzRange all{0, 0};
    std::unordered_map<std::string, AzRange> by_clientid, by_username;
  } where[AZ_MAX_SOURCES];
  bool used[AZ_MAX_SOURCES] = {};
  uint32_t e0 = 0, r0 = 0, l0 = 0, c0 = 0, b0 = 0;
  for (auto& kv : a->lists) {
    const RuleList& L = kv.second;
    const uint32_t src = std::get<0>(kv.first), scope = std::get<1>(kv.first);
    for (size_t i = 0; i < L.entries.size(); ++i) {
      AzEntry e = L.entries[i];
      e.off += b0;
      e.rule += r0;
      entries[e0 + i] = e;
    }
    for (size_t i = 0; i < L.rules.size(); ++i) {
      AzRule r = L.rules[i];
      r.who_begin += l0;
      rules[r0 + i] = r;
    }
    for (size_t i = 0; i < L.leaves.size(); ++i) {
      AzLeaf l = L.leaves[i];
      if (l.kind == AZ_LEAF_CIDR) l.a += c0; else if (l.kind != AZ_LEAF_FLAG) l.a += b0;
      leaves[l0 + i] = l;
    }
    if (!L.cidrs.empty()) std::memcpy(cidrs + c0, L.cidrs.data(), L.cidrs.size() * sizeof(AzRange));
    if (!L.arena.empty()) std::memcpy(arena + b0, L.arena.data(), L.arena.size());
    const AzRange range{e0, e0 + static_cast<uint32_t>(L.entries.size())};
    if (scope == EMQX_AUTHZ_SCOPE_ALL) where[src].all = range;
    else if (scope == EMQX_AUTHZ_SCOPE_CLIENTID) where[src].by_clientid[std::get<2>(kv.first)] = range;
    else where[src].by_username[std::get<2>(kv.first)] = range;
    used[src] = true;
    e0 += static_cast<uint32_t>(L.entries.size());
    r0 += static_cast<uint32_t>(L.rules.size());
    l0 += static_cast<uint32_t>(L.leaves.size());
    c0 += static_cast<uint32_t>(L.cidrs.size());
    b0 += static_cast<uint32_t>(L.arena.size());
  }
  for (uint32_t s = 0; s < AZ_MAX_SOURCES; ++s) sn->n_sources += used[s];

  // clients: records, bytes and the entry ranges each one's requests walk — per source the
  // clientid list, the username list, the all list (emqx_authz_mnesia.erl:95-111)
  uint32_t cb = 0;
  uint64_t max_entries = 0;
  for (uint64_t id = 0; id < n_clients; ++id) {
    const ClientRec& c = a->clients[id];
    AzClient& d = clients[id];
    if (!(c.present & AZ_REGISTERED)) continue;
    ++sn->n_clients;
    d.present = c.present;
    d.ipv4 = c.ipv4;
    d.flags = c.flags;
    d.cid_off = cb;
    d.cid_len = static_cast<uint16_t>(c.clientid.size());
    std::memcpy(carena + cb, c.clientid.data(), c.clientid.size());
    cb += static_cast<uint32_t>(c.clientid.size());
    d.user_off = cb;
    d.user_len = static_cast<uint16_t>(c.username.size());
    std::memcpy(carena + cb, c.username.data(), c.username.size());
    cb += static_cast<uint32_t>(c.username.size());
    AzRange* sg = segs + id * AZ_SEG_STRIDE;
    uint32_t ns = 0;
    uint64_t total = 0;
    auto add = [&](AzRange r) {
      if (r.lo < r.hi) sg[ns++] = r, total += r.hi - r.lo;
    };
    for (uint32_t s = 0; s < AZ_MAX_SOURCES; ++s) {
      if (!used[s]) continue;
      if (c.present & AZ_HAS_CLIENTID) {
        auto it = where[s].by_clientid.find(c.clientid);
        if (it != where[s].by_clientid.end()) add(it->second);
      }
      if (c.present & AZ_HAS_USERNAME) {
        auto it = where[s].by_username.find(c.username);
        if (it != where[s].by_username.end()) add(it->second);
      }
      add(where[s].all);
    }
    d.n_seg = ns;
    max_entries = std::max(max_entries, total);
  }
  sn->max_entries = static_cast<uint32_t>(std::min<uint64_t>(max_entries, 0xFFFFFFFFull));
  sn->n_lists = a->lists.size();
  sn->n_rules = n_rules;
  sn->n_entries = n_entries;

  auto view = [&](const uint8_t* base) {
    AzView v{};
    v.entries = reinterpret_cast<const AzEntry*>(base + o_entries);
    v.rules = reinterpret_cast<const AzRule*>(base + o_rules);
    v.leaves = reinterpret_cast<const AzLeaf*>(base + o_leaves);
    v.cidrs = reinterpret_cast<const AzRange*>(base + o_cidrs);
    v.arena = base + o_arena;
    v.clients = reinterpret_cast<const AzClient*>(base + o_clients);
    v.carena = base + o_carena;
    v.segs = reinterpret_cast<const AzRange*>(base + o_segs);
    v.n_clients = static_cast<uint32_t>(n_clients);
    v.n_entries = static_cast<uint32_t>(n_entries);
    return v;
  };
  sn->hv = view(B);
#ifndef EMQX_AUTHZ_NO_DEVICE
  if (a->device >= 0) {
    AZ_TRY(hipSetDevice(a->device));
    AZ_TRY(hipMalloc(reinterpret_cast<void**>(&sn->d_blob), sn->blob.size()));
    AZ_TRY(hipMemcpy(sn->d_blob, B, sn->blob.size(), hipMemcpyHostToDevice));
    sn->dv = view(sn->d_blob);
  }
#endif
  *out = std::move(sn);
  return EMQX_OK;
}

bool offsets_ok(const uint64_t* off, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

#ifndef EMQX_AUTHZ_NO_DEVICE
// Lanes per request.  A batch that fills the device is fastest with the fewest
// lanes per request that still keep a long list from being walked serially: a lane each up to
// tens of entries, a wave each from about a thousand (the thresholds lie between the measured
// points of tools/authz_bench.py where the shapes cross: 33|65, 513|1025, 513|1025 entries).  A
// batch too small to fill the device takes more lanes per request, up to the group that covers
// the longest request in one step.
constexpr uint32_t AZ_ENTRIES_G4 = 48;     // longest request over this many entries: 4 lanes
constexpr uint32_t AZ_ENTRIES_G16 = 640;   // ... 16 lanes
constexpr uint32_t AZ_ENTRIES_G64 = 1024;  // ... a wave
constexpr uint64_t AZ_FILL_LANES = 1u << 18;  // lanes that occupy the device (256 CUs x 16 waves)
uint32_t pick_group(const emqx_authz* a, const Snapshot& s, uint64_t n) {
  const int64_t forced = a->tune_group.load(std::memory_order_relaxed);
  if (forced) return static_cast<uint32_t>(forced);
  const uint32_t e = s.max_entries;
  const uint32_t work = e > AZ_ENTRIES_G64 ? 64u : e > AZ_ENTRIES_G16 ? 16u : e > AZ_ENTRIES_G4 ? 4u : 1u;
  const uint32_t cover = e <= 1 ? 1u : e <= 4 ? 4u : e <= 16 ? 16u : 64u;  // more lanes than this only idle
  uint32_t fill = 1;
  while (fill < 64 && n * fill < AZ_FILL_LANES) fill *= 4;
  return std::max(work, std::min(fill, cover));
}

// A scratch nobody is using: one that is idle, or one whose asynchronous call has drained (its
// event is complete); otherwise a new one.  A call never waits for another call to drain.
Work* acquire(emqx_authz* a) {
  std::unique_ptr<Work> w;
  {
    std::lock_guard<std::mutex> g(a->pmu);
    for (auto it = a->pool.begin(); it != a->pool.end(); ++it)
      if (!(*it)->inflight || hipEventQuery((*it)->done) == hipSuccess) {
        w = std::move(*it);
        a->pool.erase(it);
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
      hipMalloc(reinterpret_cast<void**>(&w->d_evals), sizeof(unsigned long long)) != hipSuccess)
    return nullptr;
  return w.release();
}

void release(emqx_authz* a, Work* w) {
  std::unique_ptr<Work> p(w);
  std::lock_guard<std::mutex> g(a->pmu);
  a->pool.push_back(std::move(p));
}

int enqueue(emqx_authz* a, const Snapshot& sn, Work* w, const uint32_t* d_clients, const uint8_t* d_actions,
            const uint8_t* d_tb, const uint64_t* d_to, uint64_t offset_base, uint64_t n, uint8_t* d_verdict,
            uint32_t* d_tag, hipStream_t s, uint32_t* group_out) {
  const uint32_t group = pick_group(a, sn, n);
  *group_out = group;
  AZ_TRY(hipMemsetAsync(w->d_evals, 0, sizeof(unsigned long long), s));
  if (az_launch_check(sn.dv, d_clients, d_actions, d_tb, d_to, n, d_verdict, d_tag, w->d_evals, group, offset_base, s) != 0)
    return EMQX_EDEVICE;
  return EMQX_OK;
}

void note_call(emqx_authz* a, uint64_t evals, uint32_t group, double ms) {
  std::lock_guard<std::mutex> g(a->smu);
  a->last_evals = evals;
  a->last_group = group;
  a->last_check_ms = ms;
}
#endif

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

namespace {

// The entry points proper; the extern "C" functions at the end of the file call them and keep
// exceptions (std::bad_alloc of the containers) from crossing the C ABI.

int az_create(int32_t device, emqx_authz** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != EMQX_AUTHZ_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_AUTHZ_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_authz> a(new (std::nothrow) emqx_authz());
  if (!a) return EMQX_ENOMEM;
  a->device = device;
  const int rc = build_snapshot(a.get(), &a->snap);  // the empty table: every client is unknown
  if (rc != EMQX_OK) return rc;
  *out = a.release();
  return EMQX_OK;
}

int az_destroy(emqx_authz* a) {
  if (!a) return EMQX_EINVAL;
#ifndef EMQX_AUTHZ_NO_DEVICE
  if (a->device >= 0) (void)hipSetDevice(a->device);
  a->pool.clear();
#endif
  delete a;
  return EMQX_OK;
}

int az_list_set(emqx_authz* a, uint32_t source, uint32_t scope, const uint8_t* key, uint64_t key_len,
                        const emqx_authz_rule* rules, uint64_t n_rules, const emqx_authz_who* who, uint64_t n_who,
                        const uint8_t* bytes, const uint64_t* offsets, uint64_t n_strings, char* err,
                        uint64_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!a) return EMQX_EINVAL;
#define AZ_REJECT(...)                 \
  do {                                 \
    set_err(err, err_cap, __VA_ARGS__); \
    return EMQX_EINVAL;                \
  } while (0)
  if (source >= AZ_MAX_SOURCES) AZ_REJECT("source %llu: at most 8 sources", source);
  if (scope > EMQX_AUTHZ_SCOPE_USERNAME) AZ_REJECT("scope %llu is not all, clientid or username", scope);
  if (scope != EMQX_AUTHZ_SCOPE_ALL && key_len > MAX_STR) AZ_REJECT("list key of %llu bytes: at most 65535", key_len);
  if (scope != EMQX_AUTHZ_SCOPE_ALL && key_len && !key) AZ_REJECT("list key missing");
  if (n_rules && !rules) AZ_REJECT("rules missing");
  if (n_who && !who) AZ_REJECT("who leaves missing");
  if (n_strings && (!offsets || (!bytes && offsets[n_strings] != offsets[0]))) AZ_REJECT("strings missing");
  if (n_strings && !offsets_ok(offsets, n_strings)) AZ_REJECT("string offsets decrease");
  auto slen = [&](uint64_t i) { return offsets[i + 1] - offsets[i]; };
  auto sptr = [&](uint64_t i) { return bytes + offsets[i]; };

  RuleList L;
  uint64_t cursor = 0;
  for (uint64_t i = 0; i < n_rules; ++i) {
    const emqx_authz_rule& r = rules[i];
    if (r.permission != EMQX_AUTHZ_ALLOW && r.permission != EMQX_AUTHZ_DENY)
      AZ_REJECT("rule %llu: permission %llu is not allow (1) or deny (2)", i, r.permission);
    if (r.action < EMQX_AUTHZ_PUBLISH || r.action > EMQX_AUTHZ_ALL)
      AZ_REJECT("rule %llu: action %llu is not publish (1), subscribe (2) or all (3)", i, r.action);
    if (r.who_op > EMQX_AUTHZ_WHO_OR) AZ_REJECT("rule %llu: who_op %llu unknown", i, r.who_op);
    if (r.who_op == EMQX_AUTHZ_WHO_ALL && r.n_who != 0) AZ_REJECT("rule %llu: who all takes no leaves", i);
    if (r.who_op == EMQX_AUTHZ_WHO_ONE && r.n_who != 1) AZ_REJECT("rule %llu: a single who takes one leaf", i);
    if (r.n_who > n_who - cursor) AZ_REJECT("rule %llu: who leaves run past the array", i);
    if (r.first_topic > n_strings || r.n_topics > n_strings - r.first_topic)
      AZ_REJECT("rule %llu: topic filters run past the string array", i);
    AzRule cr{};
    cr.permission = r.permission;
    cr.action_mask = r.action;
    cr.who_op = r.who_op;
    cr.who_begin = static_cast<uint32_t>(L.leaves.size());
    cr.n_who = r.n_who;
    cr.tag = r.tag;
    for (uint32_t k = 0; k < r.n_who; ++k) {
      const emqx_authz_who& w = who[cursor + k];
      AzLeaf l{};
      l.kind = w.kind;
      switch (w.kind) {
        case EMQX_AUTHZ_WHO_USERNAME:
        case EMQX_AUTHZ_WHO_CLIENTID:
          if (w.operand >= n_strings) AZ_REJECT("rule %llu: who string %llu outside the array", i, w.operand);
          if (slen(w.operand) > MAX_STR) AZ_REJECT("rule %llu: principal of %llu bytes: at most 65535", i, slen(w.operand));
          l.a = static_cast<uint32_t>(L.arena.size());
          l.b = static_cast<uint32_t>(slen(w.operand));
          L.arena.insert(L.arena.end(), sptr(w.operand), sptr(w.operand) + l.b);
          break;
        case EMQX_AUTHZ_WHO_CIDR:
          if (w.operand > n_strings || w.count > n_strings - w.operand)
            AZ_REJECT("rule %llu: CIDR strings run past the array", i);
          l.a = static_cast<uint32_t>(L.cidrs.size());
          l.b = w.count;
          for (uint32_t c = 0; c < w.count; ++c) {
            AzRange range{};
            const char* why = "";
            if (!parse_cidr(sptr(w.operand + c), slen(w.operand + c), &range, &why)) AZ_REJECT(why, i);
            L.cidrs.push_back(range);
          }
          break;
        case EMQX_AUTHZ_WHO_FLAG:
          if (w.operand > 63) AZ_REJECT("rule %llu: flag bit %llu: at most 63", i, w.operand);
          l.a = w.operand;
          break;
        default:
          AZ_REJECT("rule %llu: who leaf kind %llu unknown (and/or do not nest)", i, w.kind);
      }
      L.leaves.push_back(l);
    }
    cursor += r.n_who;
    for (uint32_t k = 0; k < r.n_topics; ++k) {
      const uint8_t* p = sptr(r.first_topic + k);
      uint64_t n = slen(r.first_topic + k);
      AzEntry e{};
      // compile_topic/1 (emqx_authz_rule.erl:82-91)
      if (r.eq_topics) {
        e.kind = AZ_EQ;
      } else if (n >= 3 && p[0] == 'e' && p[1] == 'q' && p[2] == ' ') {
        e.kind = AZ_EQ;
        p += 3;
        n -= 3;
      }
      if (n > MAX_STR) AZ_REJECT("rule %llu: topic filter of %llu bytes: at most 65535", i, n);
      if (e.kind != AZ_EQ) e.kind = has_placeholder(p, static_cast<uint32_t>(n)) ? AZ_PATTERN : AZ_PLAIN;
      e.off = static_cast<uint32_t>(L.arena.size());
      e.len = static_cast<uint16_t>(n);
      e.rule = static_cast<uint32_t>(i);
      L.arena.insert(L.arena.end(), p, p + n);
      L.entries.push_back(e);
    }
    L.rules.push_back(cr);
  }
#undef AZ_REJECT
  std::lock_guard<std::mutex> g(a->wmu);
  ListKey k(source, scope, scope == EMQX_AUTHZ_SCOPE_ALL ? std::string() : std::string(reinterpret_cast<const char*>(key), key_len));
  if (n_rules == 0) a->lists.erase(k);
  else a->lists[k] = std::move(L);
  return EMQX_OK;
}

int az_source_clear(emqx_authz* a, uint32_t source) {
  if (!a || source >= AZ_MAX_SOURCES) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(a->wmu);
  for (auto it = a->lists.begin(); it != a->lists.end();)
    it = std::get<0>(it->first) == source ? a->lists.erase(it) : std::next(it);
  return EMQX_OK;
}

int az_clients_set(emqx_authz* a, const uint32_t* ids, uint64_t n, const uint8_t* clientid_bytes,
                           const uint64_t* clientid_offsets, const uint8_t* username_bytes,
                           const uint64_t* username_offsets, const uint32_t* ipv4, const uint8_t* present,
                           const uint64_t* flags) {
  if (!a || (n && (!ids || !present))) return EMQX_EINVAL;
  uint32_t max_id = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (ids[i] >= MAX_CLIENT_ID) return EMQX_EINVAL;
    max_id = std::max(max_id, ids[i]);
    if (present[i] & AZ_HAS_CLIENTID) {
      if (!clientid_offsets || clientid_offsets[i + 1] < clientid_offsets[i] ||
          clientid_offsets[i + 1] - clientid_offsets[i] > MAX_STR)
        return EMQX_EINVAL;
      if (clientid_offsets[i + 1] != clientid_offsets[i] && !clientid_bytes) return EMQX_EINVAL;
    }
    if (present[i] & AZ_HAS_USERNAME) {
      if (!username_offsets || username_offsets[i + 1] < username_offsets[i] ||
          username_offsets[i + 1] - username_offsets[i] > MAX_STR)
        return EMQX_EINVAL;
      if (username_offsets[i + 1] != username_offsets[i] && !username_bytes) return EMQX_EINVAL;
    }
    if ((present[i] & AZ_HAS_IPV4) && !ipv4) return EMQX_EINVAL;
  }
  std::lock_guard<std::mutex> g(a->wmu);
  if (n && a->clients.size() <= max_id) a->clients.resize(static_cast<size_t>(max_id) + 1);
  for (uint64_t i = 0; i < n; ++i) {
    ClientRec c;
    c.present = (present[i] & 7u) | AZ_REGISTERED;
    if ((c.present & AZ_HAS_CLIENTID) && clientid_offsets[i + 1] != clientid_offsets[i])
      c.clientid.assign(reinterpret_cast<const char*>(clientid_bytes) + clientid_offsets[i],
                        clientid_offsets[i + 1] - clientid_offsets[i]);
    if ((c.present & AZ_HAS_USERNAME) && username_offsets[i + 1] != username_offsets[i])
      c.username.assign(reinterpret_cast<const char*>(username_bytes) + username_offsets[i],
                        username_offsets[i + 1] - username_offsets[i]);
    if (c.present & AZ_HAS_IPV4) c.ipv4 = ipv4[i];
    c.flags = flags ? flags[i] : 0;
    a->clients[ids[i]] = std::move(c);
  }
  return EMQX_OK;
}

int az_clients_drop(emqx_authz* a, const uint32_t* ids, uint64_t n) {
  if (!a || (n && !ids)) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(a->wmu);
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] < a->clients.size()) a->clients[ids[i]] = ClientRec();
  while (!a->clients.empty() && !(a->clients.back().present & AZ_REGISTERED)) a->clients.pop_back();
  return EMQX_OK;
}

int az_commit(emqx_authz* a) {
  if (!a) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(a->wmu);
  const auto t0 = std::chrono::steady_clock::now();
  std::shared_ptr<Snapshot> sn;
  const int rc = build_snapshot(a, &sn);
  if (rc != EMQX_OK) return rc;
  std::shared_ptr<Snapshot> old;
  {
    std::lock_guard<std::mutex> g2(a->smu);
    old = std::move(a->snap);
    a->snap = std::move(sn);
    ++a->epoch;
    a->last_build_ms = ms_since(t0);
  }
  return EMQX_OK;  // `old` is freed here unless a call in flight still holds it
}

int az_check_host(emqx_authz* a, const uint32_t* clients, const uint8_t* actions,
                          const uint8_t* topic_bytes, const uint64_t* topic_offsets, uint64_t n,
                          uint8_t* verdict_out, uint32_t* tag_out) {
  if (!a || (n && (!clients || !actions || !topic_offsets || !verdict_out))) return EMQX_EINVAL;
  if (n && !offsets_ok(topic_offsets, n)) return EMQX_EINVAL;
  if (n && !topic_bytes && topic_offsets[n] != topic_offsets[0]) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(a);
  uint64_t evals = 0;
  static const uint8_t none = 0;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t tag;
    const uint8_t* t = topic_bytes ? topic_bytes + topic_offsets[i] : &none;
    verdict_out[i] = static_cast<uint8_t>(
        az_check(sn->hv, clients[i], actions[i], t, topic_offsets[i + 1] - topic_offsets[i], &tag, &evals));
    if (tag_out) tag_out[i] = tag;
  }
  std::lock_guard<std::mutex> g(a->smu);
  a->last_evals = evals;
  a->last_check_ms = ms_since(t0);
  return EMQX_OK;
}

#ifdef EMQX_AUTHZ_NO_DEVICE

int az_check_batch(emqx_authz* a, const uint32_t*, const uint8_t*, const uint8_t*, const uint64_t*, uint64_t,
                           uint8_t*, uint32_t*) {
  return a ? EMQX_EDEVICE : EMQX_EINVAL;
}
int az_check_batch_device(emqx_authz* a, const uint32_t*, const uint8_t*, const uint8_t*, const uint64_t*,
                                  uint64_t, uint8_t*, uint32_t*, void*) {
  return a ? EMQX_EDEVICE : EMQX_EINVAL;
}
int az_check_batch_device_async(emqx_authz* a, const uint32_t*, const uint8_t*, const uint8_t*,
                                        const uint64_t*, uint64_t, uint8_t*, uint32_t*, uint64_t*, void*) {
  return a ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

int az_check_batch_device(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                  const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets, uint64_t n,
                                  uint8_t* d_verdict_out, uint32_t* d_tag_out, void* stream) {
  if (!a) return EMQX_EINVAL;
  if (a->device < 0) return EMQX_EDEVICE;
  if (n && (!d_clients || !d_actions || !d_topic_offsets || !d_verdict_out)) return EMQX_EINVAL;
  AZ_TRY(hipSetDevice(a->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(a);
  Work* w = acquire(a);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  int rc = EMQX_OK;
  uint32_t group = 0;
  unsigned long long evals = 0;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK)
    rc = enqueue(a, *sn, w, d_clients, d_actions, d_topic_bytes, d_topic_offsets, 0, n, d_verdict_out, d_tag_out, s, &group);
  if (rc == EMQX_OK && hipMemcpyAsync(&evals, w->d_evals, sizeof(evals), hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  release(a, w);
  if (rc == EMQX_OK) note_call(a, evals, group, ms_since(t0));
  return rc;
}

int az_check_batch_device_async(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                        const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets,
                                        uint64_t n, uint8_t* d_verdict_out, uint32_t* d_tag_out,
                                        uint64_t* summary, void* stream) {
  if (!a || !summary) return EMQX_EINVAL;
  if (a->device < 0) return EMQX_EDEVICE;
  if (n && (!d_clients || !d_actions || !d_topic_offsets || !d_verdict_out)) return EMQX_EINVAL;
  AZ_TRY(hipSetDevice(a->device));
  auto sn = current(a);
  Work* w = acquire(a);
  if (!w) return EMQX_EDEVICE;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : w->stream;
  int rc = EMQX_OK;
  uint32_t group = 0;
  if (!stream && after_null_stream(s) != hipSuccess) rc = EMQX_EDEVICE;
  if (rc == EMQX_OK)
    rc = enqueue(a, *sn, w, d_clients, d_actions, d_topic_bytes, d_topic_offsets, 0, n, d_verdict_out, d_tag_out, s, &group);
  if (rc == EMQX_OK && az_launch_summary(d_verdict_out, n, w->d_evals, summary, s) != 0) rc = EMQX_EDEVICE;
  if (hipEventRecord(w->done, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    rc = EMQX_EDEVICE;
  } else {
    w->inflight = sn;  // released when this scratch is next used, after `done`
  }
  release(a, w);
  return rc;
}

int az_check_batch(emqx_authz* a, const uint32_t* clients, const uint8_t* actions,
                           const uint8_t* topic_bytes, const uint64_t* topic_offsets, uint64_t n,
                           uint8_t* verdict_out, uint32_t* tag_out) {
  if (!a) return EMQX_EINVAL;
  if (a->device < 0) return EMQX_EDEVICE;
  if (n && (!clients || !actions || !topic_offsets || !verdict_out)) return EMQX_EINVAL;
  if (n && !offsets_ok(topic_offsets, n)) return EMQX_EINVAL;
  if (n == 0) return EMQX_OK;
  const uint64_t base = topic_offsets[0], nbytes = topic_offsets[n] - base;
  if (nbytes && !topic_bytes) return EMQX_EINVAL;
  AZ_TRY(hipSetDevice(a->device));
  const auto t0 = std::chrono::steady_clock::now();
  auto sn = current(a);
  Work* w = acquire(a);
  if (!w) return EMQX_EDEVICE;
  int rc = EMQX_OK;
  // request staging: [offsets (n + 1) u64][clients n u32][tags n u32][actions n][verdicts n]
  const uint64_t o_cl = (n + 1) * 8, o_tag = o_cl + n * 4, o_act = o_tag + n * 4, o_ver = o_act + n, need = o_ver + n;
  if (w->req_cap < need) {
    if (w->d_req) (void)hipFree(w->d_req);
    w->d_req = nullptr;
    w->req_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&w->d_req), need + need / 2) == hipSuccess) w->req_cap = need + need / 2;
    else rc = EMQX_ENOMEM;
  }
  if (rc == EMQX_OK && w->bytes_cap < std::max<uint64_t>(nbytes, 1)) {
    if (w->d_bytes) (void)hipFree(w->d_bytes);
    w->d_bytes = nullptr;
    w->bytes_cap = 0;
    const uint64_t cap = std::max<uint64_t>(nbytes + nbytes / 2, 256);
    if (hipMalloc(reinterpret_cast<void**>(&w->d_bytes), cap) == hipSuccess) w->bytes_cap = cap;
    else rc = EMQX_ENOMEM;
  }
  uint32_t group = 0;
  unsigned long long evals = 0;
  if (rc == EMQX_OK) {
    hipStream_t s = w->stream;
    auto* d_off = reinterpret_cast<uint64_t*>(w->d_req);
    auto* d_cl = reinterpret_cast<uint32_t*>(w->d_req + o_cl);
    auto* d_tag = reinterpret_cast<uint32_t*>(w->d_req + o_tag);
    uint8_t* d_act = w->d_req + o_act;
    uint8_t* d_ver = w->d_req + o_ver;
    // the bytes from offsets[0] on are uploaded; the kernel takes that base off every offset
    bool ok = hipMemcpyAsync(d_off, topic_offsets, (n + 1) * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_cl, clients, n * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_act, actions, n, hipMemcpyHostToDevice, s) == hipSuccess &&
              (nbytes == 0 ||
               hipMemcpyAsync(w->d_bytes, topic_bytes + base, nbytes, hipMemcpyHostToDevice, s) == hipSuccess);
    if (!ok) rc = EMQX_EDEVICE;
    if (rc == EMQX_OK)
      rc = enqueue(a, *sn, w, d_cl, d_act, w->d_bytes, d_off, base, n, d_ver, d_tag, s, &group);
    if (rc == EMQX_OK) {
      ok = hipMemcpyAsync(verdict_out, d_ver, n, hipMemcpyDeviceToHost, s) == hipSuccess &&
           (!tag_out || hipMemcpyAsync(tag_out, d_tag, n * 4, hipMemcpyDeviceToHost, s) == hipSuccess) &&
           hipMemcpyAsync(&evals, w->d_evals, sizeof(evals), hipMemcpyDeviceToHost, s) == hipSuccess;
      if (!ok) rc = EMQX_EDEVICE;
    }
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  }
  release(a, w);
  if (rc == EMQX_OK) note_call(a, evals, group, ms_since(t0));
  return rc;
}

#endif  // EMQX_AUTHZ_NO_DEVICE

int az_set_tuning(emqx_authz* a, const char* key, int64_t value) {
  if (!a || !key) return EMQX_EINVAL;
  if (std::strcmp(key, "group") != 0) return EMQX_ENOTFOUND;
  if (value != 0 && value != 1 && value != 4 && value != 16 && value != 64) return EMQX_EINVAL;
  a->tune_group.store(value, std::memory_order_relaxed);
  return EMQX_OK;
}

int az_stats_get(emqx_authz* a, emqx_authz_stats* out) {
  if (!a || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_authz_stats s{};
  std::lock_guard<std::mutex> g(a->smu);
  s.n_sources = a->snap->n_sources;
  s.n_lists = a->snap->n_lists;
  s.n_rules = a->snap->n_rules;
  s.n_entries = a->snap->n_entries;
  s.n_clients = a->snap->n_clients;
  s.table_bytes = a->snap->blob.size();
  s.epoch = a->epoch;
  s.last_evals = a->last_evals;
  s.last_group = a->last_group;
  s.last_build_ms = a->last_build_ms;
  s.last_check_ms = a->last_check_ms;
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_authz_create(int32_t device, emqx_authz** out) {
  return guarded([&] { return az_create(device, out); });
}
int emqx_authz_destroy(emqx_authz* a) {
  return guarded([&] { return az_destroy(a); });
}
int emqx_authz_list_set(emqx_authz* a, uint32_t source, uint32_t scope, const uint8_t* key, uint64_t key_len,
                        const emqx_authz_rule* rules, uint64_t n_rules, const emqx_authz_who* who, uint64_t n_who,
                        const uint8_t* bytes, const uint64_t* offsets, uint64_t n_strings, char* err,
                        uint64_t err_cap) {
  return guarded([&] {
    return az_list_set(a, source, scope, key, key_len, rules, n_rules, who, n_who, bytes, offsets, n_strings, err, err_cap);
  });
}
int emqx_authz_source_clear(emqx_authz* a, uint32_t source) {
  return guarded([&] { return az_source_clear(a, source); });
}
int emqx_authz_clients_set(emqx_authz* a, const uint32_t* ids, uint64_t n, const uint8_t* clientid_bytes,
                           const uint64_t* clientid_offsets, const uint8_t* username_bytes,
                           const uint64_t* username_offsets, const uint32_t* ipv4, const uint8_t* present,
                           const uint64_t* flags) {
  return guarded([&] {
    return az_clients_set(a, ids, n, clientid_bytes, clientid_offsets, username_bytes, username_offsets, ipv4, present,
                          flags);
  });
}
int emqx_authz_clients_drop(emqx_authz* a, const uint32_t* ids, uint64_t n) {
  return guarded([&] { return az_clients_drop(a, ids, n); });
}
int emqx_authz_commit(emqx_authz* a) {
  return guarded([&] { return az_commit(a); });
}
int emqx_authz_check_host(emqx_authz* a, const uint32_t* clients, const uint8_t* actions, const uint8_t* topic_bytes,
                          const uint64_t* topic_offsets, uint64_t n, uint8_t* verdict_out, uint32_t* tag_out) {
  return guarded([&] { return az_check_host(a, clients, actions, topic_bytes, topic_offsets, n, verdict_out, tag_out); });
}
int emqx_authz_check_batch(emqx_authz* a, const uint32_t* clients, const uint8_t* actions, const uint8_t* topic_bytes,
                           const uint64_t* topic_offsets, uint64_t n, uint8_t* verdict_out, uint32_t* tag_out) {
  return guarded([&] { return az_check_batch(a, clients, actions, topic_bytes, topic_offsets, n, verdict_out, tag_out); });
}
int emqx_authz_check_batch_device(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                  const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets, uint64_t n,
                                  uint8_t* d_verdict_out, uint32_t* d_tag_out, void* stream) {
  return guarded([&] {
    return az_check_batch_device(a, d_clients, d_actions, d_topic_bytes, d_topic_offsets, n, d_verdict_out, d_tag_out,
                                 stream);
  });
}
int emqx_authz_check_batch_device_async(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                        const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets, uint64_t n,
                                        uint8_t* d_verdict_out, uint32_t* d_tag_out, uint64_t* summary, void* stream) {
  return guarded([&] {
    return az_check_batch_device_async(a, d_clients, d_actions, d_topic_bytes, d_topic_offsets, n, d_verdict_out,
                                       d_tag_out, summary, stream);
  });
}
int emqx_authz_set_tuning(emqx_authz* a, const char* key, int64_t value) {
  return guarded([&] { return az_set_tuning(a, key, value); });
}
int emqx_authz_stats_get(emqx_authz* a, emqx_authz_stats* out) {
  return guarded([&] { return az_stats_get(a, out); });
}

}  // extern "C"
