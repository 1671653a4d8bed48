// Stand-alone program over the host-only build of the window stage (emqx_amd/csrc/window.cpp with
// EMQX_WINDOW_NO_DEVICE): generated batches of inboxes over random session records, checked
// against the session's fold written here one delivery at a time with a real queue; inboxes
// without deliveries, subscriber ids at and above sub_limit, the write-back, the refusals and the
// argument errors.  Every buffer has exactly the size the contract gives it, so an access past it
// is the sanitizer's to find.  Run plainly and under ASan + UBSan (tests/test_window_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "../../include/emqx_window.h"

namespace {

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 32);
  }
  uint32_t below(uint64_t n) { return static_cast<uint32_t>((static_cast<uint64_t>(next()) * n) >> 32); }
};

struct Batch {
  std::vector<uint32_t> subs;
  std::vector<uint64_t> offsets{0};
  std::vector<uint8_t> opts;
  std::vector<emqx_window_session> table;
};

emqx_window_session record(Rng& r) {
  static const uint32_t maxes[] = {0, 1, 4, 32, 100000}, lens[] = {0, 1, 3, 10, 1000};
  static const uint32_t flags[] = {3, 3, 3, 1, 5, 0, 11, 7};
  emqx_window_session s{};
  s.inflight = r.below(40);
  s.inflight_max = maxes[r.below(5)];
  s.mq_len = r.below(12);
  s.mq_max = lens[r.below(5)];
  s.next_pkt_id = 1 + r.below(65535);
  s.flags = flags[r.below(8)];
  s.dropped = (static_cast<uint64_t>(r.next()) << 8) | r.below(256);
  return s;
}

// `boxes` inboxes of up to max_len deliveries over a table of sub_limit records; one inbox in
// eight names an id at or above the limit when `bad` is set.
Batch make(Rng& r, uint64_t boxes, uint32_t max_len, uint32_t sub_limit, bool bad) {
  Batch b;
  for (uint32_t i = 0; i < sub_limit; ++i) b.table.push_back(record(r));
  for (uint64_t k = 0; k < boxes; ++k) {
    b.subs.push_back(bad && r.below(8) == 0 ? sub_limit + r.below(3) : r.below(sub_limit ? sub_limit : 1));
    const uint32_t n = r.below(5) == 0 ? 0 : r.below(max_len + 1);
    for (uint32_t j = 0; j < n; ++j) {
      uint8_t o = static_cast<uint8_t>(r.next());
      if (r.below(10) < 8) o &= 0x0F;
      b.opts.push_back(o);
    }
    b.offsets.push_back(b.opts.size());
  }
  return b;
}

struct Out {
  std::vector<uint8_t> verdicts;
  std::vector<uint16_t> ids;
  std::vector<emqx_window_session> recs;
  std::vector<uint32_t> counts;
  uint64_t summary[EMQX_WINDOW_SUMMARY_WORDS];
  int rc = 0;
};

Out run(emqx_window* h, Batch& b, bool update, const uint64_t* n_boxes = nullptr) {
  Out o;
  const uint64_t m = b.subs.size(), total = b.opts.size();
  o.verdicts.assign(total, 0xA5);
  o.ids.assign(total, 0xA5A5);
  o.recs.resize(m);
  if (m) std::memset(o.recs.data(), 0xA5, m * sizeof(emqx_window_session));
  o.counts.assign(4 * m, 0xA5A5A5A5u);
  for (uint64_t& w : o.summary) w = 0xA5;
  emqx_window_batch a{};
  a.inbox_subs = b.subs.data();
  a.inbox_offsets = b.offsets.data();
  a.box_opts = b.opts.data();
  a.n_boxes = n_boxes;
  a.m = n_boxes ? 0 : m;
  a.cap_in = total;
  a.cap_boxes = m;
  a.sessions = b.table.data();
  a.sub_limit = b.table.size();
  a.update_table = update ? 1 : 0;
  a.verdicts = o.verdicts.data();
  a.pkt_ids = o.ids.data();
  a.out_sessions = o.recs.data();
  a.out_counts = o.counts.data();
  o.rc = emqx_window_run_host(h, &a, o.summary);
  return o;
}

// The contract, one delivery after the other (emqx_session:deliver/2, enqueue/2, emqx_mqueue:in/2).
void check(const Batch& b, const std::vector<emqx_window_session>& table, const Out& o) {
  const uint64_t m = b.subs.size();
  uint64_t sum[EMQX_WINDOW_SUMMARY_WORDS] = {0, b.opts.size(), m, 0, 0, 0, 0, 0};
  for (uint64_t k = 0; k < m; ++k) {
    const bool ok = b.subs[k] < table.size();
    emqx_window_session s{};
    if (ok) s = table[b.subs[k]];
    else sum[0] |= EMQX_WINDOW_F_BAD_SUB;
    const bool live_box = ok && (s.flags & EMQX_WINDOW_PRESENT) && !(s.flags & EMQX_WINDOW_PASS);
    std::deque<int64_t> queue(live_box ? s.mq_len : 0, -1);  // -1: queued before the batch
    std::vector<uint8_t> want(b.offsets[k + 1] - b.offsets[k]);
    std::vector<uint16_t> ids(want.size(), 0);
    uint32_t c[4] = {0, 0, 0, 0};
    uint64_t drops = 0;
    for (size_t d = 0; d < want.size(); ++d) {
      const uint8_t op = b.opts[b.offsets[k] + d];
      const uint32_t q = op & EMQX_DELIVER_QOS_MASK;
      if (op & EMQX_DELIVER_DROP_NO_LOCAL) want[d] = EMQX_W_SKIP_NO_LOCAL;
      else if (op & EMQX_DELIVER_BAD_MESSAGE) want[d] = EMQX_W_BAD_MESSAGE;
      else if (!ok || !(s.flags & EMQX_WINDOW_PRESENT)) want[d] = EMQX_W_NO_SESSION;
      else if (s.flags & EMQX_WINDOW_PASS) want[d] = EMQX_W_PASS;
      else {
        if (s.flags & EMQX_WINDOW_CONNECTED) {
          if (q == 0) {
            want[d] = EMQX_W_SEND_QOS0;
            ++c[1];
            continue;
          }
          if (!(s.inflight_max != 0 && s.inflight >= s.inflight_max)) {
            want[d] = EMQX_W_SEND;
            ids[d] = static_cast<uint16_t>(s.next_pkt_id);
            ++s.inflight;
            s.next_pkt_id = s.next_pkt_id == 0xFFFF ? 1 : s.next_pkt_id + 1;
            ++c[0];
            continue;
          }
        } else if (q == 0 && !(s.flags & EMQX_WINDOW_STORE_QOS0)) {
          want[d] = EMQX_W_DROP_QOS0;
          ++drops;
          continue;
        }
        if (s.mq_max != 0 && queue.size() == s.mq_max) {
          const int64_t out = queue.front();
          queue.pop_front();
          if (out < 0) ++c[3];
          else want[out] = EMQX_W_QUEUED_DROPPED | (want[out] & EMQX_W_EVICTS);
          queue.push_back(static_cast<int64_t>(d));
          ++s.dropped;
          ++drops;
          want[d] = EMQX_W_QUEUED | EMQX_W_EVICTS;
        } else {
          queue.push_back(static_cast<int64_t>(d));
          want[d] = EMQX_W_QUEUED;
        }
      }
    }
    if (live_box) s.mq_len = static_cast<uint32_t>(queue.size());
    for (size_t d = 0; d < want.size(); ++d) {
      CHECK(o.verdicts[b.offsets[k] + d] == want[d]);
      CHECK(o.ids[b.offsets[k] + d] == ids[d]);
      if ((want[d] & EMQX_W_VERDICT_MASK) == EMQX_W_QUEUED) ++c[2];
    }
    CHECK(std::memcmp(&o.recs[k], &s, sizeof(s)) == 0);
    for (int j = 0; j < 4; ++j) CHECK(o.counts[4 * k + j] == c[j]);
    sum[3] += c[0], sum[4] += c[1], sum[5] += c[2], sum[6] += drops, sum[7] += c[0] > 65535;
  }
  CHECK(o.rc == ((sum[0] & EMQX_WINDOW_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  for (int w = 0; w < EMQX_WINDOW_SUMMARY_WORDS; ++w) CHECK(o.summary[w] == sum[w]);
}

bool same(const std::vector<emqx_window_session>& x, const std::vector<emqx_window_session>& y) {
  return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
}

void round_trip(emqx_window* h, Batch b) {
  const std::vector<emqx_window_session> before = b.table;
  const Out plain = run(h, b, false);
  check(b, before, plain);
  CHECK(same(b.table, before));
  const uint64_t m = b.subs.size();
  const Out counted = run(h, b, false, &m);  // the count read through n_boxes
  CHECK(counted.verdicts == plain.verdicts && counted.ids == plain.ids && counted.counts == plain.counts);
  const Out upd = run(h, b, true);
  check(b, before, upd);
  // the table now holds the records after the batch of the inboxes that changed state; of two
  // inboxes naming one subscriber the later one's
  std::vector<emqx_window_session> want = before;
  for (uint64_t k = 0; k < m; ++k) {
    const emqx_window_session& r = upd.recs[k];
    if (b.subs[k] < want.size() && (r.flags & EMQX_WINDOW_PRESENT) && !(r.flags & EMQX_WINDOW_PASS)) want[b.subs[k]] = r;
  }
  CHECK(same(b.table, want));
}

}  // namespace

int main() {
  emqx_window* h = nullptr;
  CHECK(emqx_window_create(0, &h) == EMQX_EDEVICE && h == nullptr);  // this build has no device
  CHECK(emqx_window_create(-7, &h) == EMQX_EINVAL);
  CHECK(emqx_window_create(EMQX_WINDOW_HOST_ONLY, &h) == EMQX_OK && h);
  CHECK(emqx_window_reserve(h, 100, 100) == EMQX_EDEVICE);
  Rng r{42};
  uint64_t deliveries = 0;
  for (int round = 0; round < 40; ++round) {
    Batch b = make(r, 1 + r.below(60), round % 4 == 0 ? 300 : 25, 1 + r.below(50), round % 2 == 1);
    deliveries += b.opts.size();
    round_trip(h, b);
  }
  round_trip(h, make(r, 0, 0, 4, false));     // no inbox
  round_trip(h, make(r, 7, 0, 4, true));      // inboxes without deliveries
  round_trip(h, make(r, 5, 10, 0, true));     // an empty table: every subscriber is bad
  round_trip(h, make(r, 2, 80000, 3, false)); // long inboxes: the ids wrap
  {
    // refusals: nothing but the summary is written
    Batch b = make(r, 20, 20, 10, false);
    const uint64_t total = b.opts.size(), m = b.subs.size();
    CHECK(total > 10);
    Out o = run(h, b, false);
    emqx_window_batch a{};
    a.inbox_subs = b.subs.data(), a.inbox_offsets = b.offsets.data(), a.box_opts = b.opts.data();
    a.m = m, a.cap_in = total - 1, a.cap_boxes = m, a.sessions = b.table.data(), a.sub_limit = b.table.size();
    std::fill(o.verdicts.begin(), o.verdicts.end(), 0xA5);
    a.verdicts = o.verdicts.data(), a.pkt_ids = o.ids.data(), a.out_sessions = o.recs.data(), a.out_counts = o.counts.data();
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    CHECK(o.summary[0] == EMQX_WINDOW_F_INPUT_REFUSED && o.summary[1] == total && o.summary[2] == m && o.summary[3] == 0);
    for (uint8_t v : o.verdicts) CHECK(v == 0xA5);
    const uint64_t over = m + 1;
    a.cap_in = total, a.n_boxes = &over;
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    CHECK(o.summary[0] == EMQX_WINDOW_F_INPUT_REFUSED && o.summary[1] == 0 && o.summary[2] == m + 1);
    a.n_boxes = nullptr;
    // argument errors
    a.box_opts = nullptr;
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    a.box_opts = b.opts.data();
    a.cap_boxes = m - 1;
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    a.cap_boxes = m;
    const uint64_t keep = b.offsets[3];
    b.offsets[3] = b.offsets[4] + 1;  // a decrease behind it
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    b.offsets[3] = keep;
    b.offsets[0] = 1;
    CHECK(emqx_window_run_host(h, &a, o.summary) == EMQX_EINVAL);
    b.offsets[0] = 0;
    for (uint8_t v : o.verdicts) CHECK(v == 0xA5);
    CHECK(emqx_window_run_host(h, &a, nullptr) == EMQX_OK);
    CHECK(emqx_window_run_host(nullptr, &a, nullptr) == EMQX_EINVAL && emqx_window_run_host(h, nullptr, nullptr) == EMQX_EINVAL);
    CHECK(emqx_window_run_batch(h, &a, nullptr) == EMQX_EDEVICE && emqx_window_run_batch_device(h, &a, nullptr, nullptr) == EMQX_EDEVICE);
    CHECK(emqx_window_run_batch_device_async(h, &a, o.summary, nullptr) == EMQX_EDEVICE);
  }
  {
    emqx_window_stats s{};
    s.size = sizeof(s);
    CHECK(emqx_window_stats_get(h, &s) == EMQX_OK && s.size == sizeof(s) && s.calls > 100 && s.cap_in == 0);
    CHECK(emqx_window_set_tuning(h, "path", 0) == EMQX_OK && emqx_window_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
    CHECK(emqx_window_set_tuning(h, "path", 1) == EMQX_OK && emqx_window_set_tuning(h, "path", 2) == EMQX_EINVAL);
    CHECK(emqx_window_set_tuning(h, "max_blocks", 2) == EMQX_OK && emqx_window_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
  }
  CHECK(emqx_window_destroy(h) == EMQX_OK);
  CHECK(emqx_window_destroy(nullptr) == EMQX_EINVAL);
  std::printf("window host ok: %llu deliveries\n", static_cast<unsigned long long>(deliveries));
  return 0;
}
