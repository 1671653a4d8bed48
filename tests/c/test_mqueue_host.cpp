// Stand-alone program over the host-only build of the mqueue stage (emqx_amd/csrc/mqueue.cpp with
// EMQX_MQUEUE_NO_DEVICE): generated ring tables, headers and session records; put checked against
// emqx_mqueue:in/2 folded here over a std::deque one delivery at a time, take against dequeue/3 and
// deliver_msg/2 folded over the same deque; the overflow and its repeat, subscriber ids at and above
// sub_limit, the whole-table take, malformed headers, the refusals and the argument errors.  Every
// buffer has exactly the size the contract gives it, so an access past it is the sanitizer's to
// find.  Run plainly and under ASan + UBSan (tests/test_mqueue_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "../../include/emqx_mqueue.h"

namespace {

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 32);
  }
  uint32_t below(uint64_t n) { return static_cast<uint32_t>((static_cast<uint64_t>(next()) * n) >> 32); }
};

constexpr uint64_t NOW = 1700000000000ull;

struct Msg {
  uint32_t ref;
  uint8_t opts;
};

struct Tables {
  uint32_t q = 0, sub_limit = 0;
  std::vector<emqx_window_session> table;  // exactly sub_limit
  std::vector<emqx_mqueue_entry> ring;     // exactly sub_limit * q
  std::vector<emqx_mqueue_ring> heads;     // exactly sub_limit
  std::vector<uint64_t> deadlines;         // exactly ref_limit
};

Tables tables(Rng& r, uint32_t sub_limit, uint32_t q, uint32_t ref_limit) {
  static const uint32_t flags[] = {3, 3, 3, 1, 3, 0, 11, 3};
  Tables t;
  t.q = q;
  t.sub_limit = sub_limit;
  t.table.resize(sub_limit);
  t.ring.resize(static_cast<size_t>(sub_limit) * q);
  t.heads.resize(sub_limit);
  t.deadlines.resize(ref_limit);
  for (auto& d : t.deadlines) d = r.below(3) == 0 ? NOW - 1 - r.below(5) : r.below(2) ? NOW + r.below(5) : EMQX_RETRY_NO_EXPIRY;
  for (auto& e : t.ring) e = emqx_mqueue_entry{0xAB000000u + r.below(1000), 0x55, {0, 0, 0}};
  for (uint32_t s = 0; s < sub_limit; ++s) {
    const uint32_t len = r.below(4) == 0 ? q : r.below(q + 1), head = r.below(q);
    for (uint32_t i = 0; i < len; ++i)
      t.ring[static_cast<size_t>(s) * q + (head + i) % q] = emqx_mqueue_entry{r.below(ref_limit + ref_limit / 8 + 1), static_cast<uint8_t>(r.below(3)), {0, 0, 0}};
    t.heads[s] = emqx_mqueue_ring{head, len};
    if (r.below(16) == 0) t.heads[s] = emqx_mqueue_ring{head + q * r.below(3), len + r.below(2 * q)};  // malformed
    emqx_window_session& rec = t.table[s];
    std::memset(&rec, 0, sizeof(rec));
    rec.inflight_max = r.below(4) == 0 ? 0 : 1 + r.below(q);
    rec.inflight = r.below(rec.inflight_max + 2);
    rec.mq_len = r.below(8) == 0 ? len + 1 : std::min(len, q);
    rec.mq_max = q;
    rec.next_pkt_id = r.below(3) == 0 ? 65535 - r.below(3) : 1 + r.below(65535);
    rec.flags = flags[r.below(8)];
    rec.dropped = r.below(100);
  }
  return t;
}

std::deque<Msg> queue_of(const Tables& t, uint32_t sub, uint32_t* head, bool* bad) {
  const uint32_t q = t.q;
  *bad = t.heads[sub].head >= q || t.heads[sub].len > q;
  *head = t.heads[sub].head % q;
  const uint32_t len = std::min(t.heads[sub].len, q);
  std::deque<Msg> d;
  for (uint32_t i = 0; i < len; ++i) {
    const emqx_mqueue_entry& e = t.ring[static_cast<size_t>(sub) * q + (*head + i) % q];
    d.push_back(Msg{e.ref, e.opts});
  }
  return d;
}

// ---- take ---------------------------------------------------------------------------------------

struct Took {
  std::vector<uint64_t> offsets;
  std::vector<uint8_t> opts, verdicts, status;
  std::vector<uint16_t> ids;
  std::vector<uint32_t> refs, counts;
  uint64_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// dequeue/1 of the sessions, one message at a time; the tables after it in *after.
Took model_take(const Tables& t, const std::vector<uint32_t>* subs, uint64_t m, bool use_deadlines, uint64_t cap_out, bool update,
                Tables* after) {
  Took o;
  *after = t;
  o.offsets.push_back(0);
  o.sum[2] = m;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t sub = subs ? (*subs)[k] : k;
    uint32_t c[4] = {0, 0, 0, 0};
    uint8_t st = EMQX_A_OK;
    if (sub >= t.sub_limit) {
      st = EMQX_A_NO_SESSION;
      o.sum[0] |= EMQX_MQ_F_BAD_SUB;
    } else if (!(t.table[sub].flags & EMQX_WINDOW_PRESENT)) {
      st = EMQX_A_NO_SESSION;
    } else if (t.table[sub].flags & EMQX_WINDOW_PASS) {
      st = EMQX_A_PASS;
    }
    o.status.push_back(st);
    if (st == EMQX_A_OK) {
      o.sum[1] += 1;
      uint32_t head;
      bool bad;
      std::deque<Msg> dq = queue_of(t, static_cast<uint32_t>(sub), &head, &bad);
      if (bad) o.sum[0] |= EMQX_MQ_F_BAD_RING;
      emqx_window_session rec = t.table[sub];
      if (rec.mq_len != dq.size()) {
        o.sum[7] += 1;
        o.sum[0] |= EMQX_MQ_F_LEN_MISMATCH;
      }
      uint32_t cnt = rec.inflight_max == 0 ? 1000u : (rec.inflight_max > rec.inflight ? rec.inflight_max - rec.inflight : 0u);
      uint32_t popped = 0;
      while (cnt != 0 && !dq.empty()) {  // dequeue/3
        const Msg msg = dq.front();
        dq.pop_front();
        ++popped;
        bool expired = false;
        if (use_deadlines) {
          if (msg.ref >= t.deadlines.size()) o.sum[0] |= EMQX_MQ_F_BAD_REF;
          else expired = NOW > t.deadlines[msg.ref];
        }
        o.opts.push_back(msg.opts);
        o.refs.push_back(msg.ref);
        if (expired) {
          o.verdicts.push_back(EMQX_MQ_EXPIRED);
          o.ids.push_back(0);
          c[2] += 1;
        } else if ((msg.opts & 3) == 0) {  // deliver_msg/2, first clause
          o.verdicts.push_back(EMQX_W_SEND_QOS0);
          o.ids.push_back(0);
          c[1] += 1;
        } else {
          CHECK(rec.inflight_max == 0 || rec.inflight < rec.inflight_max);  // never full: nothing is re-queued
          o.verdicts.push_back(EMQX_W_SEND);
          o.ids.push_back(static_cast<uint16_t>(rec.next_pkt_id));
          rec.next_pkt_id = rec.next_pkt_id == 0xFFFF ? 1 : rec.next_pkt_id + 1;
          rec.inflight += 1;
          cnt -= 1;
          c[0] += 1;
        }
      }
      c[3] = static_cast<uint32_t>(dq.size());
      rec.mq_len = c[3];
      after->table[sub] = rec;
      after->heads[sub] = emqx_mqueue_ring{(head + popped) % t.q, c[3]};
      o.sum[4] += c[0];
      o.sum[5] += c[1];
      o.sum[6] += c[2];
    }
    o.counts.insert(o.counts.end(), c, c + 4);
    o.offsets.push_back(o.opts.size());
  }
  o.sum[3] = o.opts.size();
  if (o.opts.size() > cap_out) {
    o.sum[0] |= EMQX_MQ_F_OUTPUT_FULL;
    *after = t;
  } else if (!update) {
    *after = t;
  }
  return o;
}

// memcmp without its demand for non-null pointers to nothing
bool same(const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

bool same_tables(const Tables& a, const Tables& b) {
  return same(a.table.data(), b.table.data(), a.table.size() * sizeof(a.table[0])) &&
         same(a.ring.data(), b.ring.data(), a.ring.size() * sizeof(a.ring[0])) &&
         same(a.heads.data(), b.heads.data(), a.heads.size() * sizeof(a.heads[0]));
}

void run_take(emqx_mqueue* h, Rng& r, uint32_t sub_limit, uint32_t q, bool whole, bool use_deadlines, bool update, int shrink) {
  const uint32_t ref_limit = 64;
  const Tables t = tables(r, sub_limit, q, ref_limit);
  std::vector<uint32_t> subs;
  if (!whole) {
    for (uint32_t s = 0; s < sub_limit; ++s)
      if (r.below(4) != 0) subs.push_back(s);
    for (size_t i = subs.size(); i > 1; --i) std::swap(subs[i - 1], subs[r.below(i)]);
    subs.push_back(sub_limit);       // at sub_limit
    subs.push_back(sub_limit + 77);  // above it
  }
  const uint64_t m = whole ? sub_limit : subs.size();
  Tables want_after;
  Took probe = model_take(t, whole ? nullptr : &subs, m, use_deadlines, ~0ull, update, &want_after);
  const uint64_t items = probe.opts.size();
  const uint64_t cap_out = shrink && items ? items - 1 : items;
  const Took want = model_take(t, whole ? nullptr : &subs, m, use_deadlines, cap_out, update, &want_after);
  Tables got = t;
  std::vector<uint64_t> off(m + 1, 99);
  std::vector<uint8_t> opts(cap_out, 9), ver(cap_out, 9), status(m, 9);
  std::vector<uint16_t> ids(cap_out, 9);
  std::vector<uint32_t> refs(cap_out, 9), counts(4 * m, 9);
  emqx_mqueue_take_args b{};
  b.subs = whole ? nullptr : subs.data();
  b.m = m;
  b.cap_boxes = m;
  b.sessions = got.table.data();
  b.sub_limit = sub_limit;
  b.update_table = update ? 1 : 0;
  b.ring = got.ring.data();
  b.heads = got.heads.data();
  b.q = q;
  b.now_ms = NOW;
  b.deadlines = use_deadlines ? t.deadlines.data() : nullptr;
  b.ref_limit = use_deadlines ? ref_limit : 0;
  b.cap_out = cap_out;
  b.out_offsets = off.data();
  b.out_opts = opts.data();
  b.out_verdicts = ver.data();
  b.out_pkt_ids = ids.data();
  b.out_refs = refs.data();
  b.out_status = status.data();
  b.out_counts = counts.data();
  uint64_t sum[8];
  const int rc = emqx_mqueue_take_host(h, &b, sum);
  const bool full = (want.sum[0] & EMQX_MQ_F_OUTPUT_FULL) != 0;
  CHECK(rc == (full ? EMQX_EOVERFLOW : (want.sum[0] & EMQX_MQ_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  CHECK(std::memcmp(sum, want.sum, sizeof(sum)) == 0);
  CHECK(off == want.offsets && status == want.status && counts == want.counts);
  if (!full) CHECK(opts == want.opts && ver == want.verdicts && ids == want.ids && refs == want.refs);
  else for (uint64_t i = 0; i < cap_out; ++i) CHECK(opts[i] == 9 && refs[i] == 9);  // untouched
  CHECK(same_tables(got, want_after));
  if (full) {  // the call again with the room it asked for
    CHECK(sum[3] == items);
    opts.assign(items, 9), ver.assign(items, 9), ids.assign(items, 9), refs.assign(items, 9);
    b.cap_out = items;
    b.out_opts = opts.data(), b.out_verdicts = ver.data(), b.out_pkt_ids = ids.data(), b.out_refs = refs.data();
    const int rc2 = emqx_mqueue_take_host(h, &b, sum);
    CHECK(rc2 == ((probe.sum[0] & EMQX_MQ_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK) && std::memcmp(sum, probe.sum, sizeof(sum)) == 0);
    CHECK(opts == probe.opts && ver == probe.verdicts && ids == probe.ids && refs == probe.refs && off == probe.offsets);
    Tables after2;
    (void)model_take(t, whole ? nullptr : &subs, m, use_deadlines, items, update, &after2);
    CHECK(same_tables(got, after2));
  }
}

// ---- put ----------------------------------------------------------------------------------------

void run_put(emqx_mqueue* h, Rng& r, uint32_t sub_limit, uint32_t q, bool with_refs, bool with_sessions) {
  const Tables t = tables(r, sub_limit, q, 64);
  // inboxes of distinct subscribers, two of them beyond the table; the verdicts are what in/2 would
  // say of a queue of max_len M <= q
  std::vector<uint32_t> subs;
  for (uint32_t s = 0; s < sub_limit; ++s)
    if (r.below(3) != 0) subs.push_back(s);
  for (size_t i = subs.size(); i > 1; --i) std::swap(subs[i - 1], subs[r.below(i)]);
  subs.push_back(sub_limit);
  subs.push_back(sub_limit + 5);
  const uint64_t m = subs.size();
  std::vector<uint64_t> off(m + 1, 0);
  std::vector<uint8_t> opts, ver;
  Tables want = t;
  std::vector<emqx_mqueue_entry> want_ev;
  std::vector<uint32_t> want_un(m, 0);
  uint64_t ws[8] = {0, 0, m, 0, 0, 0, 0, 0};
  for (uint64_t k = 0; k < m; ++k) {
    const uint32_t sub = subs[k];
    const uint32_t n = r.below(4) == 0 ? 0 : r.below(3 * q);
    if (sub >= sub_limit) {
      ws[0] |= EMQX_MQ_F_BAD_SUB;
      for (uint32_t i = 0; i < n; ++i) {
        opts.push_back(1);
        ver.push_back(EMQX_W_QUEUED);
        want_ev.push_back(emqx_mqueue_entry{EMQX_MQ_NO_REF, 0, {0, 0, 0}});
      }
      want_un[k] = n;
      ws[5] += n;
      off[k + 1] = opts.size();
      continue;
    }
    uint32_t head;
    bool bad;
    std::deque<Msg> old = queue_of(t, sub, &head, &bad);
    if (bad) ws[0] |= EMQX_MQ_F_BAD_RING;
    const uint32_t M = std::max<uint32_t>(static_cast<uint32_t>(old.size()), 1 + r.below(q));  // L <= M <= q
    // the queue as (is_old, index): in/2 one delivery at a time
    std::deque<std::pair<bool, uint64_t>> dq;
    for (uint64_t i = 0; i < old.size(); ++i) dq.emplace_back(true, i);
    uint32_t gone_old = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t d = opts.size();
      const uint32_t kind = r.below(8);
      want_ev.push_back(emqx_mqueue_entry{EMQX_MQ_NO_REF, 0, {0, 0, 0}});
      if (kind == 0) {  // sent, not queued
        opts.push_back(static_cast<uint8_t>(1 + r.below(2)));
        ver.push_back(EMQX_W_SEND);
        continue;
      }
      opts.push_back(static_cast<uint8_t>(r.below(3)));
      uint8_t v = EMQX_W_QUEUED;
      if (dq.size() == M) {  // reached max length, drop the oldest message
        const auto out = dq.front();
        dq.pop_front();
        v |= EMQX_W_EVICTS;
        if (out.first) {
          want_ev[d] = emqx_mqueue_entry{old[out.second].ref, old[out.second].opts, {0, 0, 0}};
          ++gone_old;
        } else {
          ver[out.second] = static_cast<uint8_t>(EMQX_W_QUEUED_DROPPED | (ver[out.second] & EMQX_W_EVICTS));
        }
      }
      dq.emplace_back(false, d);
      ver.push_back(v);
    }
    const uint32_t new_head = (head + gone_old) % q;
    uint32_t i = 0;
    for (const auto& e : dq) {
      if (!e.first) {
        const uint32_t ref = with_refs ? static_cast<uint32_t>(e.second * 3 + 7) : static_cast<uint32_t>(e.second);
        want.ring[static_cast<size_t>(sub) * q + (new_head + i) % q] = emqx_mqueue_entry{ref, opts[e.second], {0, 0, 0}};
        ws[3] += 1;
      }
      ++i;
    }
    want.heads[sub] = emqx_mqueue_ring{new_head, static_cast<uint32_t>(dq.size())};
    ws[4] += gone_old;
    if (with_sessions && t.table[sub].mq_len != dq.size()) {
      ws[7] += 1;
      ws[0] |= EMQX_MQ_F_LEN_MISMATCH;
    }
    off[k + 1] = opts.size();
  }
  const uint64_t total = opts.size();
  ws[1] = total;
  std::vector<uint32_t> refs(total);
  for (uint64_t d = 0; d < total; ++d) refs[d] = static_cast<uint32_t>(d * 3 + 7);
  Tables got = t;
  std::vector<emqx_mqueue_entry> ev(total, emqx_mqueue_entry{5, 5, {5, 5, 5}});
  std::vector<uint32_t> un(m, 99);
  emqx_mqueue_put_args b{};
  b.inbox_subs = subs.data();
  b.inbox_offsets = off.data();
  b.box_opts = opts.data();
  b.m = m;
  b.cap_in = total;
  b.cap_boxes = m;
  b.verdicts = ver.data();
  b.refs = with_refs ? refs.data() : nullptr;
  b.sessions = with_sessions ? got.table.data() : nullptr;
  b.ring = got.ring.data();
  b.heads = got.heads.data();
  b.q = q;
  b.sub_limit = sub_limit;
  b.out_evicted = ev.data();
  b.out_unstored = un.data();
  uint64_t sum[8];
  CHECK(emqx_mqueue_put_host(h, &b, sum) == EMQX_EINVAL);  // the two subscribers beyond the table
  CHECK(std::memcmp(sum, ws, sizeof(sum)) == 0);
  CHECK(un == want_un);
  CHECK(same(ev.data(), want_ev.data(), total * sizeof(ev[0])));
  CHECK(same_tables(got, want));
}

void abi(emqx_mqueue* h) {
  emqx_mqueue* none = nullptr;
  CHECK(emqx_mqueue_create(0, &none) == EMQX_EDEVICE && none == nullptr);
  CHECK(emqx_mqueue_create(-7, &none) == EMQX_EINVAL && emqx_mqueue_create(EMQX_MQUEUE_HOST_ONLY, nullptr) == EMQX_EINVAL);
  CHECK(emqx_mqueue_reserve(h, 1, 1) == EMQX_EDEVICE);
  uint64_t off[2] = {0, 0}, sum[8];
  emqx_mqueue_put_args p{};
  p.inbox_offsets = off;
  p.q = 8;
  CHECK(emqx_mqueue_put_host(h, &p, sum) == EMQX_OK && sum[0] == 0 && sum[2] == 0);
  CHECK(emqx_mqueue_put_batch(h, &p, sum) == EMQX_EDEVICE && emqx_mqueue_put_batch_device(h, &p, sum, nullptr) == EMQX_EDEVICE &&
        emqx_mqueue_put_batch_device_async(h, &p, sum, nullptr) == EMQX_EDEVICE);
  p.q = 24;
  CHECK(emqx_mqueue_put_host(h, &p, sum) == EMQX_EINVAL);
  p.q = 8;
  p.inbox_offsets = nullptr;
  CHECK(emqx_mqueue_put_host(h, &p, sum) == EMQX_EINVAL);
  emqx_mqueue_take_args t{};
  t.out_offsets = off;
  t.q = 1024;
  CHECK(emqx_mqueue_take_host(h, &t, sum) == EMQX_OK && off[0] == 0 && sum[3] == 0);
  CHECK(emqx_mqueue_take_batch(h, &t, sum) == EMQX_EDEVICE && emqx_mqueue_take_batch_device(h, &t, sum, nullptr) == EMQX_EDEVICE &&
        emqx_mqueue_take_batch_device_async(h, &t, sum, nullptr) == EMQX_EDEVICE);
  t.q = 2048;
  CHECK(emqx_mqueue_take_host(h, &t, sum) == EMQX_EINVAL);
  t.q = 8;
  t.now_ms = EMQX_RETRY_MAX_NOW;
  CHECK(emqx_mqueue_take_host(h, &t, sum) == EMQX_EINVAL);
  t.now_ms = 1;
  t.m = 1;  // subs NULL and m > sub_limit 0, cap_boxes 0: an argument error before anything is read
  CHECK(emqx_mqueue_take_host(h, &t, sum) == EMQX_EINVAL);
  CHECK(emqx_mqueue_set_tuning(h, "max_blocks", 1) == EMQX_OK && emqx_mqueue_set_tuning(h, "scan_chunk", 1025) == EMQX_EINVAL &&
        emqx_mqueue_set_tuning(h, "path", 1) == EMQX_ENOTFOUND);
  emqx_mqueue_stats s{};
  s.size = sizeof(s);
  CHECK(emqx_mqueue_stats_get(h, &s) == EMQX_OK && s.size == sizeof(s) && s.calls >= 2 && s.scratch_bytes == 0);
}

}  // namespace

int main() {
  emqx_mqueue* h = nullptr;
  CHECK(emqx_mqueue_create(EMQX_MQUEUE_HOST_ONLY, &h) == EMQX_OK && h);
  abi(h);
  Rng r{20261021};
  static const uint32_t qs[] = {8, 16, 64, 256, 1024};
  for (int round = 0; round < 40; ++round) {
    const uint32_t q = qs[round % 5], sub_limit = q >= 256 ? 1 + r.below(12) : 1 + r.below(150);
    run_take(h, r, sub_limit, q, round % 4 == 1, round % 3 != 0, round % 5 != 4, round % 7 == 3);
    run_put(h, r, sub_limit, q, round % 2 == 0, round % 3 != 1);
  }
  run_take(h, r, 0, 8, true, false, true, 0);
  CHECK(emqx_mqueue_destroy(h) == EMQX_OK && emqx_mqueue_destroy(nullptr) == EMQX_EINVAL);
  std::printf("mqueue host ok\n");
  return 0;
}
