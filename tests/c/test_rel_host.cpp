// Stand-alone program over the host-only build of the rel stage (emqx_amd/csrc/rel.cpp with
// EMQX_REL_NO_DEVICE): generated batches of inbound events over random rows and session records,
// checked against the session's fold written here one event at a time over a std::map as the
// awaiting_rel map (packet id -> the slots that hold it); generated expire calls checked against the
// predicate per entry; sessions without events, subscriber ids at and above sub_limit, every W,
// the refusals and the argument errors.  Every buffer has exactly the size the contract gives it, so
// an access past it is the sanitizer's to find.  Run plainly and under ASan + UBSan
// (tests/test_rel_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../include/emqx_rel.h"

namespace {

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

static_assert(sizeof(emqx_rel_run_args) == 20 * 8 && sizeof(emqx_rel_expire_args) == 14 * 8 && sizeof(emqx_rel_stats) == 64, "ABI");

// memcmp without its demand for non-null pointers to nothing
bool same(const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 32);
  }
  uint32_t below(uint64_t n) { return static_cast<uint32_t>((static_cast<uint64_t>(next()) * n) >> 32); }
};

constexpr uint64_t NOW = 1600000000000ull;

struct Tables {
  uint32_t w = 0;
  std::vector<emqx_window_session> table;
  std::vector<uint64_t> rel;  // exactly sub_limit * w
  std::vector<uint32_t> lims;
};

Tables tables(Rng& r, uint32_t sub_limit, uint32_t w) {
  static const uint32_t flags[] = {3, 3, 3, 1, 3, 0, 11, 3};
  Tables t;
  t.w = w;
  for (uint32_t i = 0; i < sub_limit; ++i) {
    emqx_window_session s{};
    s.inflight = r.below(9);
    s.flags = flags[r.below(8)];
    s.dropped = r.next();
    t.table.push_back(s);
    const uint32_t pick = r.below(10);
    t.lims.push_back(pick == 0 ? 0 : pick == 1 ? w + 1 + r.below(5) : 1 + r.below(std::min<uint32_t>(w, 5)));
    for (uint32_t j = 0; j < w; ++j)  // few ids: some rows hold one twice; rows above their limit too
      t.rel.push_back(r.below(4) == 0 ? EMQX_REL_ENTRY(NOW - r.below(2000), 1 + r.below(8)) : 0);
  }
  return t;
}

// One run call against the fold written over a std::map.
void run_case(emqx_rel* h, Rng& r, uint32_t sub_limit, uint32_t w, uint32_t m, bool use_maxes, bool use_ts, bool use_src) {
  Tables t = tables(r, sub_limit, w);
  const uint32_t scalar = 1 + r.below(4);
  std::vector<uint32_t> subs, pool;
  for (uint32_t i = 0; i < sub_limit + 2; ++i) pool.push_back(i);  // two ids at and above sub_limit
  for (uint32_t i = 0; i < m && !pool.empty(); ++i) {
    const uint32_t at = r.below(pool.size());
    subs.push_back(pool[at]);
    pool.erase(pool.begin() + at);
  }
  m = static_cast<uint32_t>(subs.size());
  std::vector<uint64_t> off(m + 1, 0);
  std::vector<uint32_t> ev;
  for (uint32_t k = 0; k < m; ++k) {
    const uint32_t n = r.below(4) == 0 ? 0 : r.below(12);
    for (uint32_t i = 0; i < n; ++i) {
      static const uint32_t kinds[] = {1, 1, 1, 2, 2, 3, 0, 9};
      ev.push_back(kinds[r.below(8)] << 16 | (1 + r.below(8)));
    }
    off[k + 1] = ev.size();
  }
  const uint64_t total = ev.size();
  std::vector<uint64_t> ts(total);
  std::vector<uint32_t> src(total);
  for (uint64_t d = 0; d < total; ++d) {
    ts[d] = r.below(50) == 0 ? EMQX_REL_TS_LIMIT + r.below(9) : NOW + r.below(100);
    src[d] = r.next();
  }
  // the expectation
  std::vector<uint64_t> want_rel = t.rel;
  std::vector<uint8_t> want_ver(total);
  std::vector<uint32_t> want_route, want_cnt(4 * m, 0);
  std::vector<uint8_t> want_arm(m, 0);
  uint64_t want[8] = {0, total, m, 0, 0, 0, 0, 0};
  for (uint32_t k = 0; k < m; ++k) {
    const uint32_t sub = subs[k];
    const bool ok = sub < sub_limit;
    if (!ok) want[0] |= EMQX_REL_F_BAD_SUB;
    const uint32_t limit = ok ? (use_maxes ? t.lims[sub] : scalar) : 0;
    uint8_t dead = 0;
    if (!ok || !(t.table[sub].flags & EMQX_WINDOW_PRESENT)) dead = EMQX_REL_NO_SESSION;
    else if (t.table[sub].flags & EMQX_WINDOW_PASS) dead = EMQX_REL_PASS;
    else if (limit == 0 || limit > w) dead = EMQX_REL_ROW_SMALL, want[0] |= EMQX_REL_F_ROW_SMALL;
    if (dead) {
      for (uint64_t d = off[k]; d < off[k + 1]; ++d) want_ver[d] = dead;
      continue;
    }
    uint64_t* row = want_rel.data() + static_cast<uint64_t>(sub) * w;
    std::map<uint32_t, std::set<uint32_t>> awaiting;  // packet id -> its slots
    std::set<uint32_t> empty;
    size_t size = 0;
    for (uint32_t j = 0; j < w; ++j) {
      if (row[j]) awaiting[EMQX_REL_ENTRY_ID(row[j])].insert(j), ++size;
      else empty.insert(j);
    }
    for (uint64_t d = off[k]; d < off[k + 1]; ++d) {
      const uint32_t kind = ev[d] >> 16, id = ev[d] & 0xFFFFu;
      uint8_t v;
      if (kind == EMQX_REL_DIRECT) {
        v = EMQX_REL_OK;
      } else if (kind == EMQX_REL_PUBLISH) {
        if (size >= limit) v = EMQX_REL_EXCEEDED;
        else if (awaiting.count(id)) v = EMQX_REL_IN_USE;
        else {
          v = EMQX_REL_OK;
          const uint32_t j = *empty.begin();
          empty.erase(empty.begin());
          uint64_t stamp = use_ts ? ts[d] : NOW;
          if (stamp >= EMQX_REL_TS_LIMIT) stamp = EMQX_REL_TS_LIMIT - 1, want[0] |= EMQX_REL_F_BAD_TS;
          row[j] = EMQX_REL_ENTRY(stamp, id);
          awaiting[id].insert(j);
          ++size;
          want_arm[k] = 1;
        }
      } else if (kind == EMQX_REL_PUBREL) {
        auto it = awaiting.find(id);
        if (it == awaiting.end()) v = EMQX_REL_NOT_FOUND;
        else {
          v = EMQX_REL_OK;
          const uint32_t j = *it->second.begin();
          it->second.erase(it->second.begin());
          if (it->second.empty()) awaiting.erase(it);
          row[j] = 0;
          empty.insert(j);
          --size;
          ++want_cnt[4 * k + 1];
          ++want[4];
        }
      } else {
        v = EMQX_REL_BAD_KIND;
      }
      want_ver[d] = v;
      if (v == EMQX_REL_OK && kind != EMQX_REL_PUBREL) {
        want_route.push_back(use_src ? src[d] : static_cast<uint32_t>(d));
        ++want_cnt[4 * k];
        ++want[3];
      }
      if (v != EMQX_REL_OK) ++want_cnt[4 * k + 2];
      if (v == EMQX_REL_IN_USE) ++want[5];
      if (v == EMQX_REL_NOT_FOUND) ++want[6];
      if (v == EMQX_REL_EXCEEDED) ++want[7];
    }
    want_cnt[4 * k + 3] = static_cast<uint32_t>(size);
  }
  // the call, on buffers of exactly their size
  const std::vector<emqx_window_session> table0 = t.table;
  std::vector<uint8_t> ver(total, 0x5A), arm(m, 0x5A);
  std::vector<uint32_t> route(total, 0x5A5A5A5Au), cnt(4 * m, 0x5A5A5A5Au);
  emqx_rel_run_args b{};
  b.ev_subs = subs.data();
  b.ev_offsets = off.data();
  b.events = ev.data();
  b.m = m;
  b.cap_in = total;
  b.cap_boxes = m;
  b.ts = use_ts ? ts.data() : nullptr;
  b.src = use_src ? src.data() : nullptr;
  b.sessions = t.table.data();
  b.sub_limit = sub_limit;
  b.rel = t.rel.data();
  b.w = w;
  b.now_ms = NOW;
  b.max_awaiting = scalar;
  b.maxes = use_maxes ? t.lims.data() : nullptr;
  b.verdicts = ver.data();
  b.out_route = route.data();
  b.out_counts = cnt.data();
  b.out_arm = arm.data();
  uint64_t sum[8];
  const int rc = emqx_rel_run_host(h, &b, sum);
  CHECK(rc == ((want[0] & EMQX_REL_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  CHECK(same(sum, want, sizeof(want)));
  CHECK(same(ver.data(), want_ver.data(), total));
  CHECK(same(route.data(), want_route.data(), 4 * want_route.size()));
  for (uint64_t i = want_route.size(); i < total; ++i) CHECK(route[i] == 0x5A5A5A5Au);
  CHECK(same(cnt.data(), want_cnt.data(), 16 * m) && same(arm.data(), want_arm.data(), m));
  CHECK(same(t.rel.data(), want_rel.data(), 8 * want_rel.size()));
  CHECK(same(t.table.data(), table0.data(), sizeof(table0[0]) * table0.size()));
}

void expire_case(emqx_rel* h, Rng& r, uint32_t sub_limit, uint32_t w, bool listed, bool use_timeouts, bool channel_rule) {
  Tables t = tables(r, sub_limit, w);
  std::vector<uint32_t> subs, timeouts;
  for (uint32_t i = 0; i < sub_limit; ++i) {
    static const uint32_t some[] = {0, 1, 500, 1000, 1999, 2000, EMQX_REL_NO_TIMEOUT};
    timeouts.push_back(some[r.below(7)]);
  }
  if (listed) {
    for (uint32_t i = 0; i < sub_limit + 1; i += 1 + r.below(2)) subs.push_back(sub_limit - i);  // sub_limit itself first
  }
  const uint32_t m = listed ? static_cast<uint32_t>(subs.size()) : r.below(sub_limit + 1);
  const uint32_t scalar = 700;
  std::vector<uint64_t> want_rel = t.rel;
  std::vector<uint8_t> want_st(m);
  std::vector<uint32_t> want_cnt(4 * m, 0);
  uint64_t want[8] = {0, 0, m, 0, 0, 0, 0, 0};
  for (uint32_t k = 0; k < m; ++k) {
    const uint32_t sub = listed ? subs[k] : k;
    const bool ok = sub < sub_limit;
    if (!ok) want[0] |= EMQX_REL_F_BAD_SUB;
    const uint32_t fl = ok ? t.table[sub].flags : 0;
    want_st[k] = !(fl & EMQX_WINDOW_PRESENT) ? EMQX_REL_NO_SESSION
                 : (fl & EMQX_WINDOW_PASS)   ? EMQX_REL_PASS
                 : (channel_rule && !(fl & EMQX_WINDOW_CONNECTED)) ? EMQX_REL_IDLE : EMQX_REL_OK;
    if (want_st[k] != EMQX_REL_OK) continue;
    const uint32_t timeout = use_timeouts ? timeouts[sub] : scalar;
    for (uint32_t j = 0; j < w; ++j) {
      uint64_t& e = want_rel[static_cast<uint64_t>(sub) * w + j];
      if (!e) continue;
      const int64_t age = static_cast<int64_t>(NOW - 1000) - static_cast<int64_t>(EMQX_REL_ENTRY_TS(e));
      if (timeout != EMQX_REL_NO_TIMEOUT && age >= static_cast<int64_t>(timeout)) e = 0, ++want_cnt[4 * k];
      else ++want_cnt[4 * k + 1];
    }
    want_cnt[4 * k + 2] = want_cnt[4 * k + 1] > 0;
    want[1] += 1;
    want[3] += want_cnt[4 * k];
    want[4] += want_cnt[4 * k + 1];
    want[5] += want_cnt[4 * k + 2];
  }
  std::vector<uint8_t> st(m, 0x5A);
  std::vector<uint32_t> cnt(4 * m, 0x5A5A5A5Au);
  emqx_rel_expire_args b{};
  b.subs = listed ? subs.data() : nullptr;
  b.m = m;
  b.cap_boxes = m;
  b.sessions = t.table.data();
  b.sub_limit = sub_limit;
  b.rel = t.rel.data();
  b.w = w;
  b.now_ms = NOW - 1000;  // half of the stamps lie in the future
  b.timeout_ms = scalar;
  b.timeouts = use_timeouts ? timeouts.data() : nullptr;
  b.channel_rule = channel_rule;
  b.out_status = st.data();
  b.out_counts = cnt.data();
  uint64_t sum[8];
  const int rc = emqx_rel_expire_host(h, &b, sum);
  CHECK(rc == ((want[0] & EMQX_REL_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  CHECK(same(sum, want, sizeof(want)));
  CHECK(same(st.data(), want_st.data(), m) && same(cnt.data(), want_cnt.data(), 16 * m));
  CHECK(same(t.rel.data(), want_rel.data(), 8 * want_rel.size()));
}

void abi(emqx_rel* h) {
  emqx_rel* none = nullptr;
  CHECK(emqx_rel_create(0, &none) == EMQX_EDEVICE && none == nullptr);  // this build has no device
  CHECK(emqx_rel_create(-7, &none) == EMQX_EINVAL && emqx_rel_create(EMQX_REL_HOST_ONLY, nullptr) == EMQX_EINVAL);
  CHECK(emqx_rel_reserve(h, 10, 10, 8) == EMQX_EDEVICE && emqx_rel_reserve(nullptr, 10, 10, 8) == EMQX_EINVAL);
  emqx_rel_run_args b{};
  emqx_rel_expire_args x{};
  uint64_t sum[8];
  CHECK(emqx_rel_run_batch(h, &b, sum) == EMQX_EDEVICE && emqx_rel_run_batch_device(h, &b, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_rel_run_batch_device_async(h, &b, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_rel_expire_batch(h, &x, sum) == EMQX_EDEVICE && emqx_rel_expire_batch_device(h, &x, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_rel_expire_batch_device_async(h, &x, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_rel_run_host(h, &b, sum) == EMQX_EINVAL);  // w 0
  const uint64_t off[2] = {0, 0};
  b.ev_offsets = off;
  for (uint64_t w : {8, 16, 32, 64, 128}) {
    b.w = x.w = w;
    CHECK(emqx_rel_run_host(h, &b, sum) == EMQX_OK && sum[1] == 0 && sum[2] == 0);  // a call of nothing
    CHECK(emqx_rel_expire_host(h, &x, sum) == EMQX_OK && sum[2] == 0);
  }
  for (uint64_t w : {0, 7, 9, 48, 129, 256}) {
    b.w = x.w = w;
    CHECK(emqx_rel_run_host(h, &b, sum) == EMQX_EINVAL && emqx_rel_expire_host(h, &x, sum) == EMQX_EINVAL);
  }
  CHECK(emqx_rel_set_tuning(h, "lanes", 8) == EMQX_OK && emqx_rel_set_tuning(h, "lanes", 5) == EMQX_EINVAL);
  CHECK(emqx_rel_set_tuning(h, "max_blocks", 0) == EMQX_EINVAL && emqx_rel_set_tuning(h, "scan_chunk", 1) == EMQX_OK);
  CHECK(emqx_rel_set_tuning(h, "rematch", 0) == EMQX_ENOTFOUND && emqx_rel_set_tuning(h, nullptr, 0) == EMQX_EINVAL);
  emqx_rel_stats s{};
  s.size = sizeof(s);
  CHECK(emqx_rel_stats_get(h, &s) == EMQX_OK && s.size == sizeof(s) && s.lanes == 8 && s.calls > 0 && s.scratch_bytes == 0);
  s.size = 7;
  CHECK(emqx_rel_stats_get(h, &s) == EMQX_EINVAL);
}

}  // namespace

int main() {
  emqx_rel* h = nullptr;
  CHECK(emqx_rel_create(EMQX_REL_HOST_ONLY, &h) == EMQX_OK && h);
  Rng r{20240607};
  uint32_t cases = 0;
  for (uint32_t w : {8u, 16u, 32u, 64u, 128u}) {
    for (uint32_t round = 0; round < 40; ++round) {
      const uint32_t sub_limit = 1 + r.below(24);
      run_case(h, r, sub_limit, w, r.below(sub_limit + 3), round & 1, round & 2, round & 4);
      expire_case(h, r, sub_limit, w, round & 1, round & 2, round & 4);
      cases += 2;
    }
  }
  run_case(h, r, 3, 8, 0, false, false, false);  // no session at all
  abi(h);
  CHECK(emqx_rel_destroy(h) == EMQX_OK && emqx_rel_destroy(nullptr) == EMQX_EINVAL);
  std::printf("rel host ok: %u cases\n", cases);
  return 0;
}
