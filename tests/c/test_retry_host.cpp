// Stand-alone program over the host-only build of the retry stage (emqx_amd/csrc/retry.cpp with
// EMQX_RETRY_NO_DEVICE): generated tables of rows, stamps and session records, swept and checked
// against the session's fold written here over a std::map as the inflight window (sort by
// timestamp, walk until the first young entry), replayed, stamped and checked against a loop over
// the slots; the overflow and its repeat, subscriber ids at and above sub_limit, the whole-table
// sweep, the refusals and the argument errors.  Every buffer has exactly the size the contract gives
// it, so an access past it is the sanitizer's to find.  Run plainly and under ASan + UBSan
// (tests/test_retry_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/emqx_retry.h"

namespace {

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

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

constexpr uint64_t NOW = 1700000000000ull;

uint64_t mk(uint64_t ts, uint32_t dup, uint32_t phase, uint32_t id) { return (ts << 19) | (uint64_t(dup) << 18) | (uint64_t(phase & 3) << 16) | id; }
bool owns(uint64_t stamp, const emqx_ack_slot& s) {
  return s.phase != 0 && ((stamp >> 16) & 3) == s.phase && (stamp & 0xFFFF) == s.pkt_id;
}

struct Tables {
  uint32_t w = 0, sub_limit = 0;
  std::vector<emqx_window_session> table;
  std::vector<emqx_ack_slot> slots;  // exactly sub_limit * w
  std::vector<uint64_t> stamps;      // exactly sub_limit * w
  std::vector<uint32_t> intervals;   // exactly sub_limit
  std::vector<uint64_t> deadlines;   // exactly ref_limit
};

Tables tables(Rng& r, uint32_t sub_limit, uint32_t w, uint32_t ref_limit) {
  static const uint32_t flags[] = {3, 3, 3, 1, 3, 0, 11, 3};
  static const int64_t ages[] = {250, 101, 100, 99, 1, 0, -7};
  Tables t;
  t.w = w;
  t.sub_limit = sub_limit;
  for (uint32_t i = 0; i < ref_limit; ++i) {
    const uint32_t k = r.below(5);
    t.deadlines.push_back(k == 0 ? EMQX_RETRY_NO_EXPIRY : k == 1 ? NOW : k == 2 ? NOW - 1 : k == 3 ? NOW + 1 : r.below(2) ? 5 : NOW + 100000);
  }
  for (uint32_t i = 0; i < sub_limit; ++i) {
    emqx_window_session s{};
    s.inflight = r.below(w + 4);
    s.inflight_max = w;
    s.flags = flags[r.below(8)];
    s.dropped = r.next();
    t.table.push_back(s);
    static const uint32_t ivs[] = {100, 100, 0, 1, 200, 0x90000000u};
    t.intervals.push_back(ivs[r.below(6)]);
    const int64_t tie = ages[r.below(7)];
    for (uint32_t j = 0; j < w; ++j) {
      emqx_ack_slot e{0, 0, 0, 0};
      uint64_t stamp = r.below(8) == 0 ? mk(NOW - 3, 0, 1 + r.below(2), r.below(40)) : 0;  // a stale one
      if (r.below(3)) {
        e.pkt_id = static_cast<uint16_t>(r.below(8) == 0 ? 65535 : r.below(60));  // few ids: some rows hold one twice
        e.phase = static_cast<uint8_t>(1 + r.below(2));
        e.qos = static_cast<uint8_t>(1 + r.below(2));
        e.ref = r.below(ref_limit + 2);
        const int64_t age = r.below(2) ? tie : ages[r.below(7)];
        if (r.below(20)) stamp = mk(static_cast<uint64_t>(static_cast<int64_t>(NOW) - age), r.below(2), e.phase, e.pkt_id);
      }
      t.slots.push_back(e);
      t.stamps.push_back(stamp);
    }
  }
  return t;
}

struct Out {
  std::vector<uint64_t> offsets;
  std::vector<emqx_retry_item> items;
  std::vector<uint8_t> status;
  std::vector<uint32_t> counts, timers;
  uint64_t sum[8];
};

struct Entry {
  uint32_t slot;
  emqx_ack_slot s;
  uint64_t ts;
  uint32_t dup;
  bool stamped;
};

// The fold, one session at a time over its window as a map keyed (pkt_id, slot).
Out expect(Tables& t, const std::vector<uint32_t>* subs, uint64_t m, uint32_t mode, uint64_t interval_ms, bool per_session, bool expiry,
           uint64_t cap_out, bool update_table) {
  Out o;
  std::memset(o.sum, 0, sizeof(o.sum));
  o.sum[2] = m;
  Tables work = t;
  o.offsets.push_back(0);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = subs ? (*subs)[k] : k;
    uint32_t c[4] = {0, 0, 0, 0}, timer = EMQX_RETRY_NO_TIMER;
    uint8_t st = EMQX_A_OK;
    if (sub >= t.sub_limit) o.sum[0] |= EMQX_RETRY_F_BAD_SUB;
    if (sub >= t.sub_limit || !(t.table[sub].flags & EMQX_WINDOW_PRESENT)) st = EMQX_A_NO_SESSION;
    else if (t.table[sub].flags & EMQX_WINDOW_PASS) st = EMQX_A_PASS;
    if (st == EMQX_A_OK) {
      o.sum[1] += 1;
      std::map<std::pair<uint32_t, uint32_t>, Entry> window;
      for (uint32_t j = 0; j < t.w; ++j) {
        const emqx_ack_slot& s = t.slots[sub * t.w + j];
        if (s.phase == EMQX_ACK_EMPTY) continue;
        const uint64_t stamp = t.stamps[sub * t.w + j];
        const bool mine = mode == EMQX_RETRY_MODE_RETRY && owns(stamp, s);
        window[{s.pkt_id, j}] = Entry{j, s, mine ? stamp >> 19 : NOW, mine ? uint32_t((stamp >> 18) & 1) : 0u, mine};
      }
      if (mode == EMQX_RETRY_MODE_REPLAY) {
        for (auto& kv : window) {
          const uint8_t kind = kv.second.s.phase == EMQX_ACK_PUBREL_AWAIT ? EMQX_RETRY_PUBREL : EMQX_RETRY_PUBLISH_DUP;
          o.items.push_back({kv.second.s.pkt_id, kind, kv.second.s.qos, kv.second.s.ref});
          c[kind - 1] += 1;
        }
      } else {
        const uint64_t iv = std::min<uint64_t>(per_session ? t.intervals[sub] : interval_ms, EMQX_RETRY_MAX_INTERVAL);
        std::vector<Entry*> order;
        for (auto& kv : window) {
          if (!kv.second.stamped) {
            o.sum[7] += 1;
            o.sum[0] |= EMQX_RETRY_F_UNSTAMPED;
          }
          order.push_back(&kv.second);
        }
        std::stable_sort(order.begin(), order.end(), [](const Entry* a, const Entry* b) { return a->ts < b->ts; });
        if (!order.empty()) timer = static_cast<uint32_t>(iv);
        std::vector<uint32_t> gone;
        for (Entry* e : order) {
          const int64_t age = static_cast<int64_t>(NOW) - static_cast<int64_t>(e->ts);
          if (age < static_cast<int64_t>(iv)) {
            timer = static_cast<uint32_t>(iv - static_cast<uint64_t>(std::max<int64_t>(age, 0)));
            break;
          }
          uint8_t kind = EMQX_RETRY_PUBLISH_DUP;
          if (e->s.phase == EMQX_ACK_PUBREL_AWAIT) {
            kind = EMQX_RETRY_PUBREL;
          } else if (expiry) {
            if (e->s.ref >= t.deadlines.size()) o.sum[0] |= EMQX_RETRY_F_BAD_REF;
            else if (NOW > t.deadlines[e->s.ref]) kind = EMQX_RETRY_EXPIRED;
          }
          o.items.push_back({e->s.pkt_id, kind, e->s.qos, e->s.ref});
          c[kind - 1] += 1;
          e->ts = NOW;
          e->dup = kind == EMQX_RETRY_PUBLISH_DUP;
          if (kind == EMQX_RETRY_EXPIRED) gone.push_back(e->slot);
        }
        for (auto& kv : window) {
          const Entry& e = kv.second;
          work.stamps[sub * t.w + e.slot] = mk(e.ts, e.dup, e.s.phase, e.s.pkt_id);
        }
        for (uint32_t j : gone) {
          work.slots[sub * t.w + j] = emqx_ack_slot{0, 0, 0, 0};
          work.stamps[sub * t.w + j] = 0;
        }
      }
      c[3] = t.table[sub].inflight > c[2] ? t.table[sub].inflight - c[2] : 0;
      if (update_table) work.table[sub].inflight = c[3];
      o.sum[4] += c[0];
      o.sum[5] += c[1];
      o.sum[6] += c[2];
    }
    o.status.push_back(st);
    o.counts.insert(o.counts.end(), c, c + 4);
    o.timers.push_back(timer);
    o.offsets.push_back(o.items.size());
  }
  o.sum[3] = o.items.size();
  if (o.items.size() > cap_out) {
    o.sum[0] |= EMQX_RETRY_F_OUTPUT_FULL;
    o.items.clear();
  } else if (mode == EMQX_RETRY_MODE_RETRY) {
    t = work;
  }
  return o;
}

int expected_rc(const Out& o) {
  if (o.sum[0] & EMQX_RETRY_F_OUTPUT_FULL) return EMQX_EOVERFLOW;
  return (o.sum[0] & EMQX_RETRY_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK;
}

void sweep_round(emqx_retry* h, Rng& r, uint32_t w, uint32_t sub_limit, uint32_t mode, bool whole) {
  const uint32_t ref_limit = 1 + r.below(12);
  Tables t = tables(r, sub_limit, w, ref_limit);
  std::vector<uint32_t> subs;
  for (uint32_t i = 0; i < sub_limit; ++i)
    if (whole || r.below(3)) subs.push_back(i);
  if (!whole) {
    for (size_t i = subs.size(); i > 1; --i) std::swap(subs[i - 1], subs[r.below(i)]);
    if (r.below(2)) subs.push_back(sub_limit + r.below(3));
  }
  const uint64_t m = subs.size();
  const bool per_session = r.below(2), expiry = r.below(3) != 0, update = r.below(2);
  const uint64_t interval = 100;
  Tables want = t;
  const Out all = expect(want, whole ? nullptr : &subs, m, mode, interval, per_session, expiry, ~0ull, update);
  const uint64_t need = all.sum[3];
  for (int pass = 0; pass < 2; ++pass) {  // one item short (nothing changes), then exact
    if (pass == 0 && need == 0) continue;
    const uint64_t cap_out = pass == 0 ? need - 1 : need;
    Tables got = t, ref = t;
    const Out o = expect(ref, whole ? nullptr : &subs, m, mode, interval, per_session, expiry, cap_out, update);
    std::vector<uint64_t> offsets(m + 1, 77);
    std::vector<emqx_retry_item> items(cap_out);
    std::vector<uint8_t> status(m, 77);
    std::vector<uint32_t> counts(4 * m, 77), timers(m, 77);
    emqx_retry_sweep_args b{};
    b.subs = whole ? nullptr : subs.data();
    b.m = b.cap_boxes = m;
    b.sessions = got.table.data();
    b.sub_limit = sub_limit;
    b.update_table = update;
    b.slots = got.slots.data();
    b.stamps = mode == EMQX_RETRY_MODE_REPLAY && r.below(2) ? nullptr : got.stamps.data();
    b.w = w;
    b.now_ms = NOW;
    b.interval_ms = interval;
    b.intervals = per_session ? got.intervals.data() : nullptr;
    b.deadlines = expiry ? got.deadlines.data() : nullptr;
    b.ref_limit = ref_limit;
    b.mode = mode;
    b.cap_out = cap_out;
    b.out_offsets = offsets.data();
    b.out_items = items.data();
    b.out_status = status.data();
    b.out_counts = counts.data();
    b.out_timers = timers.data();
    uint64_t sum[8];
    CHECK(emqx_retry_sweep_host(h, &b, sum) == expected_rc(o));
    CHECK(same(sum, o.sum, sizeof(sum)));
    CHECK(offsets == o.offsets && status == o.status && counts == o.counts && timers == o.timers);
    CHECK(same(items.data(), o.items.data(), o.items.size() * sizeof(emqx_retry_item)));
    CHECK(same(got.slots.data(), ref.slots.data(), ref.slots.size() * sizeof(emqx_ack_slot)));
    CHECK(got.stamps == ref.stamps);
    CHECK(same(got.table.data(), ref.table.data(), ref.table.size() * sizeof(emqx_window_session)));
    if (pass == 0) {
      CHECK(same(got.slots.data(), t.slots.data(), t.slots.size() * sizeof(emqx_ack_slot)) && got.stamps == t.stamps);
      CHECK(same(got.table.data(), t.table.data(), t.table.size() * sizeof(emqx_window_session)));
    }
  }
}

void stamp_round(emqx_retry* h, Rng& r, uint32_t w, uint32_t sub_limit) {
  Tables t = tables(r, sub_limit, w, 4);
  std::vector<uint32_t> subs;
  for (uint32_t i = 0; i < sub_limit; ++i)
    if (r.below(2)) subs.push_back(i);
  const bool bad = r.below(2);
  if (bad) subs.push_back(sub_limit);
  std::vector<uint64_t> want = t.stamps;
  uint64_t exp[8] = {bad ? EMQX_RETRY_F_BAD_SUB : 0u, subs.size() - bad, subs.size(), 0, 0, 0, 0, 0};
  for (uint32_t sub : subs) {
    if (sub >= sub_limit) continue;
    for (uint32_t j = 0; j < w; ++j) {
      const emqx_ack_slot& s = t.slots[sub * w + j];
      uint64_t& v = want[sub * w + j];
      const uint64_t next = s.phase == 0 ? 0 : owns(v, s) ? v : mk(NOW + 5, 0, s.phase, s.pkt_id);
      if (next != v) exp[next ? 3 : 4] += 1;
      v = next;
    }
  }
  emqx_retry_stamp_args b{};
  b.subs = subs.data();
  b.m = b.cap_boxes = subs.size();
  b.slots = t.slots.data();
  b.stamps = t.stamps.data();
  b.w = w;
  b.sub_limit = sub_limit;
  b.now_ms = NOW + 5;
  uint64_t sum[8];
  CHECK(emqx_retry_stamp_host(h, &b, sum) == (bad ? EMQX_EINVAL : EMQX_OK));
  CHECK(same(sum, exp, sizeof(sum)) && t.stamps == want);
}

void errors(emqx_retry* h) {
  Rng r{5};
  Tables t = tables(r, 4, 8, 2);
  uint64_t off[5];
  emqx_retry_item items[32];
  uint8_t status[4];
  uint32_t counts[16], timers[4];
  emqx_retry_sweep_args b{};
  b.m = b.cap_boxes = 4;
  b.sessions = t.table.data();
  b.sub_limit = 4;
  b.slots = t.slots.data();
  b.stamps = t.stamps.data();
  b.w = 8;
  b.now_ms = NOW;
  b.interval_ms = 100;
  b.cap_out = 32;
  b.out_offsets = off;
  b.out_items = items;
  b.out_status = status;
  b.out_counts = counts;
  b.out_timers = timers;
  CHECK(emqx_retry_sweep_host(h, &b, nullptr) == EMQX_OK);
  CHECK(emqx_retry_sweep_host(nullptr, &b, nullptr) == EMQX_EINVAL && emqx_retry_sweep_host(h, nullptr, nullptr) == EMQX_EINVAL);
  emqx_retry_sweep_args x = b;
  x.w = 12;
  CHECK(emqx_retry_sweep_host(h, &x, nullptr) == EMQX_EINVAL);
  x = b;
  x.mode = 2;
  CHECK(emqx_retry_sweep_host(h, &x, nullptr) == EMQX_EINVAL);
  x = b;
  x.interval_ms = EMQX_RETRY_MAX_INTERVAL + 1;
  CHECK(emqx_retry_sweep_host(h, &x, nullptr) == EMQX_EINVAL);
  x = b;
  x.now_ms = EMQX_RETRY_MAX_NOW;
  CHECK(emqx_retry_sweep_host(h, &x, nullptr) == EMQX_EINVAL);
  x = b;
  x.stamps = nullptr;
  CHECK(emqx_retry_sweep_host(h, &x, nullptr) == EMQX_EINVAL);
  x = b;
  x.m = x.cap_boxes = 5;  // subs NULL: more sessions than the table holds
  uint64_t sum[8];
  CHECK(emqx_retry_sweep_host(h, &x, sum) == EMQX_EINVAL && sum[0] == EMQX_RETRY_F_INPUT_REFUSED && sum[2] == 5);
  CHECK(emqx_retry_sweep_batch(h, &b, nullptr) == EMQX_EDEVICE && emqx_retry_sweep_batch_device(h, &b, nullptr, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_retry_sweep_batch_device_async(h, &b, sum, nullptr) == EMQX_EDEVICE && emqx_retry_reserve(h, 4, 8) == EMQX_EDEVICE);
  emqx_retry* dev = nullptr;
  CHECK(emqx_retry_create(0, &dev) == EMQX_EDEVICE && dev == nullptr && emqx_retry_create(-5, &dev) == EMQX_EINVAL);
  CHECK(emqx_retry_set_tuning(h, "max_blocks", 0) == EMQX_EINVAL && emqx_retry_set_tuning(h, "scan_chunk", 2) == EMQX_OK);
  CHECK(emqx_retry_set_tuning(h, "rematch", 0) == EMQX_ENOTFOUND);
  emqx_retry_stats s{};
  s.size = sizeof(s);
  CHECK(emqx_retry_stats_get(h, &s) == EMQX_OK && s.calls >= 1 && s.size == sizeof(s));
}

}  // namespace

int main() {
  emqx_retry* h = nullptr;
  CHECK(emqx_retry_create(EMQX_RETRY_HOST_ONLY, &h) == EMQX_OK && h);
  Rng r{20240229};
  static const uint32_t widths[] = {8, 16, 32, 64};
  for (uint32_t round = 0; round < 160; ++round) {
    const uint32_t w = widths[round % 4], sub_limit = round < 8 ? round / 4 : 1 + r.below(40);
    sweep_round(h, r, w, sub_limit, round % 5 == 4 ? EMQX_RETRY_MODE_REPLAY : EMQX_RETRY_MODE_RETRY, round % 7 == 3);
    stamp_round(h, r, w, sub_limit);
  }
  errors(h);
  CHECK(emqx_retry_destroy(h) == EMQX_OK);
  std::printf("retry host ok\n");
  return 0;
}
