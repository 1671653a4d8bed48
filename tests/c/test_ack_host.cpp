// Stand-alone program over the host-only build of the ack stage (emqx_amd/csrc/ack.cpp with
// EMQX_ACK_NO_DEVICE): generated batches of ack lists over random rows and session records, checked
// against the session's fold written here one ack at a time over a std::map as the inflight
// window; generated record calls checked against "fill the lowest free slots"; lists without acks,
// subscriber ids at and above sub_limit, the table update, the refusals and the argument errors.
// Every buffer has exactly the size the contract gives it, so an access past it is the
// sanitizer's to find.  Run plainly and under ASan + UBSan (tests/test_ack_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/emqx_ack.h"

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

struct Tables {
  uint32_t w = 0;
  std::vector<emqx_window_session> table;
  std::vector<emqx_ack_slot> slots;  // exactly sub_limit * w
};

Tables tables(Rng& r, uint32_t sub_limit, uint32_t w) {
  static const uint32_t flags[] = {3, 3, 3, 1, 3, 0, 11, 3};
  Tables t;
  t.w = w;
  for (uint32_t i = 0; i < sub_limit; ++i) {
    emqx_window_session s{};
    s.inflight = r.below(w + 4);
    s.inflight_max = r.below(3) == 0 ? 0 : w;
    s.mq_len = r.below(9);
    s.next_pkt_id = 1 + r.below(65535);
    s.flags = flags[r.below(8)];
    s.dropped = r.next();
    t.table.push_back(s);
    for (uint32_t j = 0; j < w; ++j) {
      emqx_ack_slot e{0, 0, 0, 0};
      if (r.below(3)) {
        e.pkt_id = static_cast<uint16_t>(r.below(40));  // few ids: some rows hold one twice
        e.phase = static_cast<uint8_t>(1 + r.below(2));
        e.qos = static_cast<uint8_t>(1 + r.below(2));
        e.ref = r.next();
      }
      t.slots.push_back(e);
    }
  }
  return t;
}

struct Lists {
  std::vector<uint32_t> subs;
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> acks;
};

// `m` lists over distinct sessions; one in eight names an id at or above the limit when `bad`.
Lists lists(Rng& r, uint64_t m, uint32_t max_len, uint32_t sub_limit, bool bad) {
  Lists l;
  std::vector<uint32_t> ids(sub_limit);
  for (uint32_t i = 0; i < sub_limit; ++i) ids[i] = i;
  for (uint32_t i = sub_limit; i > 1; --i) std::swap(ids[i - 1], ids[r.below(i)]);
  CHECK(m <= sub_limit);
  for (uint64_t k = 0; k < m; ++k) {
    l.subs.push_back(bad && r.below(8) == 0 ? sub_limit + static_cast<uint32_t>(k) : ids[k]);
    const uint32_t n = r.below(5) == 0 ? 0 : r.below(max_len + 1);
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t kind = r.below(20) == 0 ? r.below(7) : 1 + r.below(3);
      l.acks.push_back((kind << 16) | r.below(44));
    }
    l.offsets.push_back(l.acks.size());
  }
  return l;
}

struct Out {
  std::vector<uint8_t> verdicts;
  std::vector<uint32_t> refs, counts;
  uint64_t summary[EMQX_ACK_SUMMARY_WORDS];
  int rc = 0;
};

emqx_ack_run_args run_args(Lists& l, Tables& t, Out& o, bool update) {
  emqx_ack_run_args b{};
  b.ack_subs = l.subs.data();
  b.ack_offsets = l.offsets.data();
  b.acks = l.acks.data();
  b.m = l.subs.size();
  b.cap_in = l.acks.size();
  b.cap_boxes = l.subs.size();
  b.sessions = t.table.data();
  b.sub_limit = t.table.size();
  b.update_table = update ? 1 : 0;
  b.slots = t.slots.data();
  b.w = t.w;
  b.verdicts = o.verdicts.data();
  b.out_refs = o.refs.data();
  b.out_counts = o.counts.data();
  return b;
}

Out run(emqx_ack* h, Lists& l, Tables& t, bool update, const uint64_t* n_boxes = nullptr) {
  Out o;
  o.verdicts.assign(l.acks.size(), 0xA5);
  o.refs.assign(l.acks.size(), 0xA5A5A5A5u);
  o.counts.assign(4 * l.subs.size(), 0xA5A5A5A5u);
  emqx_ack_run_args b = run_args(l, t, o, update);
  b.n_boxes = n_boxes;
  o.rc = emqx_ack_run_host(h, &b, o.summary);
  return o;
}

// The fold, one ack at a time: emqx_inflight as a map from packet id to slot.
void expect_run(const Lists& l, Tables t, bool update, const Out& got, const Tables& after) {
  uint64_t sum[8] = {0, l.acks.size(), l.subs.size(), 0, 0, 0, 0, 0};
  for (size_t k = 0; k < l.subs.size(); ++k) {
    const uint32_t sub = l.subs[k];
    const bool ok = sub < t.table.size();
    if (!ok) sum[0] |= EMQX_ACK_F_BAD_SUB;
    const uint32_t flags = ok ? t.table[sub].flags : 0;
    const bool live = (flags & EMQX_WINDOW_PRESENT) && !(flags & EMQX_WINDOW_PASS);
    std::map<uint32_t, uint32_t> inflight;
    emqx_ack_slot* row = ok ? t.slots.data() + static_cast<size_t>(sub) * t.w : nullptr;
    if (live)
      for (uint32_t w = 0; w < t.w; ++w)
        if (row[w].phase != EMQX_ACK_EMPTY) inflight.emplace(row[w].pkt_id, w);  // the lowest slot stays
    uint32_t released = 0, to_pubrel = 0, errors = 0;
    for (uint64_t d = l.offsets[k]; d < l.offsets[k + 1]; ++d) {
      const uint32_t kind = l.acks[d] >> 16, id = l.acks[d] & 0xFFFF;
      uint8_t v;
      uint32_t ref = EMQX_ACK_NO_REF;
      if (!live) {
        v = (flags & EMQX_WINDOW_PRESENT) ? EMQX_A_PASS : EMQX_A_NO_SESSION;
      } else if (kind < 1 || kind > 3) {
        v = EMQX_A_BAD_KIND;
      } else if (!inflight.count(id)) {
        v = EMQX_A_NOT_FOUND;
      } else {
        emqx_ack_slot& s = row[inflight[id]];
        const bool msg = s.phase == EMQX_ACK_MSG;
        if ((kind == EMQX_ACK_PUBACK && msg) || (kind == EMQX_ACK_PUBCOMP && !msg)) {
          v = EMQX_A_OK, ref = s.ref;
          s = emqx_ack_slot{0, 0, 0, 0};
          inflight.erase(id);
          ++released;
        } else if (kind == EMQX_ACK_PUBREC && msg) {
          v = EMQX_A_OK, ref = s.ref;
          s.phase = EMQX_ACK_PUBREL_AWAIT;
          ++to_pubrel;
        } else {
          v = EMQX_A_IN_USE;
        }
      }
      CHECK(got.verdicts[d] == v);
      CHECK(got.refs[d] == ref);
      if (live && v != EMQX_A_OK) ++errors;
      sum[v == EMQX_A_OK ? 3 : v == EMQX_A_IN_USE ? 5 : v == EMQX_A_NOT_FOUND ? 6 : 7] += 1;
    }
    uint32_t want[4] = {0, 0, 0, 0};
    if (live) {
      emqx_window_session& rec = t.table[sub];
      const uint32_t left = rec.inflight > released ? rec.inflight - released : 0;
      want[0] = released, want[1] = to_pubrel, want[2] = errors;
      want[3] = rec.inflight_max == 0 ? 1000u : (rec.inflight_max > left ? rec.inflight_max - left : 0u);
      if (update) rec.inflight = left;
      sum[4] += released;
    }
    CHECK(std::memcmp(&got.counts[4 * k], want, sizeof(want)) == 0);
  }
  CHECK(std::memcmp(got.summary, sum, sizeof(sum)) == 0);
  CHECK(got.rc == ((sum[0] & EMQX_ACK_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  CHECK(same(after.slots.data(), t.slots.data(), t.slots.size() * sizeof(emqx_ack_slot)));
  CHECK(same(after.table.data(), t.table.data(), t.table.size() * sizeof(emqx_window_session)));
}

void fuzz_run(emqx_ack* h, uint64_t seed, uint32_t w, uint32_t sub_limit, uint64_t m, uint32_t max_len, bool bad, bool update) {
  Rng r{seed};
  Tables t = tables(r, sub_limit, w);
  Lists l = lists(r, m, max_len, sub_limit, bad);
  const Tables before = t;
  const Out o = run(h, l, t, update);
  expect_run(l, before, update, o, t);
}

// ---- record ------------------------------------------------------------------------------------

struct Sends {
  std::vector<uint32_t> subs;
  std::vector<uint64_t> offsets{0};
  std::vector<uint8_t> opts, verdicts;
  std::vector<uint16_t> ids;
  std::vector<uint32_t> refs;
};

void fuzz_record(emqx_ack* h, uint64_t seed, uint32_t w, uint32_t sub_limit, uint64_t m, uint32_t max_len, bool bad, bool with_refs) {
  Rng r{seed};
  Tables t = tables(r, sub_limit, w);
  const Lists l = lists(r, m, 0, sub_limit, bad);  // for the distinct subscriber ids
  Sends s;
  s.subs = l.subs;
  for (uint64_t k = 0; k < m; ++k) {
    const uint32_t n = r.below(4) == 0 ? 0 : r.below(max_len + 1);
    for (uint32_t j = 0; j < n; ++j) {
      s.verdicts.push_back(static_cast<uint8_t>(r.below(3) == 0 ? (EMQX_W_SEND | (r.below(2) ? 0x40 : 0)) : r.below(10)));
      s.opts.push_back(static_cast<uint8_t>(r.next()));
      s.ids.push_back(static_cast<uint16_t>(r.next()));
      s.refs.push_back(r.next());
    }
    s.offsets.push_back(s.verdicts.size());
  }
  Tables want = t;
  std::vector<uint32_t> unrec(m, 0), got(m, 0xA5A5A5A5u);
  uint64_t sum[8] = {0, s.verdicts.size(), m, 0, 0, 0, 0, 0};
  for (uint64_t k = 0; k < m; ++k) {
    const bool ok = s.subs[k] < sub_limit;
    if (!ok) sum[0] |= EMQX_ACK_F_BAD_SUB;
    std::vector<uint32_t> free;
    for (uint32_t j = 0; ok && j < w; ++j)
      if (t.slots[static_cast<size_t>(s.subs[k]) * w + j].phase == EMQX_ACK_EMPTY) free.push_back(j);
    size_t used = 0;
    for (uint64_t d = s.offsets[k]; d < s.offsets[k + 1]; ++d) {
      if ((s.verdicts[d] & EMQX_W_VERDICT_MASK) != EMQX_W_SEND) continue;
      ++sum[3];
      if (used == free.size()) {
        ++unrec[k];
        continue;
      }
      emqx_ack_slot& e = want.slots[static_cast<size_t>(s.subs[k]) * w + free[used++]];
      e.pkt_id = s.ids[d];
      e.phase = EMQX_ACK_MSG;
      e.qos = s.opts[d] & EMQX_DELIVER_QOS_MASK;
      e.ref = with_refs ? s.refs[d] : static_cast<uint32_t>(d);
      ++sum[4];
    }
    sum[5] += unrec[k];
    if (ok && unrec[k]) sum[6] += 1, sum[0] |= EMQX_ACK_F_ROW_FULL;
  }
  emqx_ack_record_args b{};
  b.inbox_subs = s.subs.data();
  b.inbox_offsets = s.offsets.data();
  b.box_opts = s.opts.data();
  b.m = m;
  b.cap_in = s.verdicts.size();
  b.cap_boxes = m;
  b.verdicts = s.verdicts.data();
  b.pkt_ids = s.ids.data();
  b.refs = with_refs ? s.refs.data() : nullptr;
  b.slots = t.slots.data();
  b.w = w;
  b.sub_limit = sub_limit;
  b.out_unrecorded = got.data();
  uint64_t out[8];
  const int rc = emqx_ack_record_host(h, &b, out);
  CHECK(rc == ((sum[0] & EMQX_ACK_F_BAD_SUB) ? EMQX_EINVAL : EMQX_OK));
  CHECK(std::memcmp(out, sum, sizeof(sum)) == 0);
  CHECK(got == unrec);
  CHECK(same(t.slots.data(), want.slots.data(), t.slots.size() * sizeof(emqx_ack_slot)));
}

void errors(emqx_ack* h) {
  Rng r{99};
  Tables t = tables(r, 6, 8);
  Lists l = lists(r, 4, 5, 6, false);
  const Tables before = t;
  Out o;
  o.verdicts.assign(l.acks.size(), 0xA5);
  o.refs.assign(l.acks.size(), 0xA5A5A5A5u);
  o.counts.assign(4 * l.subs.size(), 0xA5A5A5A5u);
  uint64_t summary[8];
  auto untouched = [&] {
    for (uint8_t v : o.verdicts) CHECK(v == 0xA5);
    for (uint32_t c : o.counts) CHECK(c == 0xA5A5A5A5u);
    CHECK(same(before.slots.data(), t.slots.data(), t.slots.size() * sizeof(emqx_ack_slot)));
  };
  emqx_ack_run_args b = run_args(l, t, o, true);
  CHECK(emqx_ack_run_host(nullptr, &b, summary) == EMQX_EINVAL);
  CHECK(emqx_ack_run_host(h, nullptr, summary) == EMQX_EINVAL);
  for (uint64_t w : {0ull, 4ull, 12ull, 63ull, 128ull}) {
    b = run_args(l, t, o, true);
    b.w = w;
    CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  }
  b = run_args(l, t, o, true);
  b.sessions = nullptr;
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  b = run_args(l, t, o, true);
  b.cap_boxes = b.m - 1;
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  untouched();
  // refusals: the summary alone
  b = run_args(l, t, o, true);
  b.cap_in = l.acks.size() - 1;
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  CHECK(summary[0] == EMQX_ACK_F_INPUT_REFUSED && summary[1] == l.acks.size() && summary[2] == l.subs.size() && summary[3] == 0);
  const uint64_t too_many = l.subs.size() + 1;
  b = run_args(l, t, o, true);
  b.n_boxes = &too_many;
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  CHECK(summary[0] == EMQX_ACK_F_INPUT_REFUSED && summary[1] == 0 && summary[2] == too_many);
  std::vector<uint64_t> huge{0, EMQX_ACK_MAX_ACKS};
  b = run_args(l, t, o, true);
  b.ack_offsets = huge.data();
  b.m = 1;
  b.cap_in = (1ull << 32) - 1;
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  CHECK(summary[0] == EMQX_ACK_F_INPUT_REFUSED && summary[1] == EMQX_ACK_MAX_ACKS);
  untouched();
  // offsets that decrease or do not start at 0
  std::vector<uint64_t> off = l.offsets;
  off[0] = 1;
  b = run_args(l, t, o, true);
  b.ack_offsets = off.data();
  CHECK(emqx_ack_run_host(h, &b, summary) == EMQX_EINVAL);
  untouched();
  // the device entry points of a host-only handle
  CHECK(emqx_ack_run_batch(h, &b, summary) == EMQX_EDEVICE);
  CHECK(emqx_ack_run_batch_device(h, &b, summary, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_ack_run_batch_device_async(h, &b, summary, nullptr) == EMQX_EDEVICE);
  emqx_ack_record_args rb{};
  CHECK(emqx_ack_record_batch(h, &rb, summary) == EMQX_EDEVICE);
  CHECK(emqx_ack_record_batch_device(h, &rb, summary, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_ack_record_batch_device_async(h, &rb, summary, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_ack_record_host(h, &rb, summary) == EMQX_EINVAL);
  CHECK(emqx_ack_reserve(h, 10, 10, 8) == EMQX_EDEVICE);
  emqx_ack* dev = nullptr;
  CHECK(emqx_ack_create(0, &dev) == EMQX_EDEVICE && dev == nullptr);
  CHECK(emqx_ack_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
  CHECK(emqx_ack_set_tuning(h, "rematch", 2) == EMQX_EINVAL);
  CHECK(emqx_ack_set_tuning(h, "rematch", 1) == EMQX_OK);
  CHECK(emqx_ack_set_tuning(h, "max_blocks", 2) == EMQX_OK && emqx_ack_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
  emqx_ack_stats st{};
  st.size = sizeof(st);
  CHECK(emqx_ack_stats_get(h, &st) == EMQX_OK && st.size == sizeof(st) && st.rematch == 1 && st.scratch_bytes == 0);
}

}  // namespace

int main() {
  emqx_ack* h = nullptr;
  CHECK(emqx_ack_create(EMQX_ACK_HOST_ONLY, &h) == EMQX_OK && h);
  const uint32_t widths[] = {8, 16, 32, 64};
  uint64_t seed = 1;
  for (uint32_t w : widths) {
    for (int round = 0; round < 12; ++round, ++seed) {
      fuzz_run(h, seed, w, 40, 30, 3 * w, round % 3 == 0, round % 2 == 0);
      fuzz_record(h, seed, w, 40, 30, 2 * w, round % 3 == 0, round % 2 == 0);
    }
    fuzz_run(h, ++seed, w, 5, 3, 5000, false, true);  // long lists
    fuzz_record(h, ++seed, w, 5, 3, 5000, false, true);
    fuzz_run(h, ++seed, w, 3, 0, 0, false, true);  // no lists
    fuzz_record(h, ++seed, w, 3, 0, 0, false, false);
    fuzz_run(h, ++seed, w, 0, 0, 0, false, true);  // no tables
  }
  errors(h);
  CHECK(emqx_ack_destroy(h) == EMQX_OK);
  CHECK(emqx_ack_destroy(nullptr) == EMQX_EINVAL);
  std::printf("ack host ok\n");
  return 0;
}
