// Stand-alone program over the host-only build of the inbox stage (emqx_amd/csrc/inbox.cpp with
// EMQX_INBOX_NO_DEVICE): generated CSRs with empty messages, one subscriber, distinct
// subscribers, every number of passes, n = 0, the optional outputs absent, the refusals and a
// capacity of inboxes one short, checked against std::stable_sort written here.  Every output
// buffer has exactly the size the contract gives it, so a write past it is the sanitizer's to
// find.  Run plainly and under ASan + UBSan (tests/test_inbox_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../include/emqx_inbox.h"

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

struct Csr {
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> subs, filters, subids;
  std::vector<uint8_t> opts;
  uint64_t sub_limit = 1;
};

// kind 0: random ids below the limit; 1: one subscriber; 2: distinct, descending.
Csr make(Rng& r, uint64_t n, uint32_t max_row, uint64_t sub_limit, int kind) {
  Csr c;
  c.sub_limit = sub_limit;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t k = r.below(4) == 0 ? 0 : r.below(max_row + 1);
    for (uint32_t j = 0; j < k; ++j) {
      c.subs.push_back(kind == 1 ? static_cast<uint32_t>(sub_limit - 1) : r.below(sub_limit));
      c.filters.push_back(r.next());  // the flag bits among them
      c.opts.push_back(static_cast<uint8_t>(r.next()));
      c.subids.push_back(r.next() >> 4);
    }
    c.offsets.push_back(c.subs.size());
  }
  if (kind == 2) {
    CHECK(c.subs.size() <= sub_limit);
    for (size_t d = 0; d < c.subs.size(); ++d) c.subs[d] = static_cast<uint32_t>(c.subs.size() - 1 - d);
  }
  return c;
}

struct Out {
  std::vector<uint32_t> msgs, filters, subids, src, inbox_subs;
  std::vector<uint8_t> opts;
  std::vector<uint64_t> inbox_offsets;
  uint64_t summary[EMQX_INBOX_SUMMARY_WORDS];
  uint64_t n_boxes = 0;
  int rc = 0;
};

Out run(emqx_inbox* h, const Csr& c, uint64_t cap_boxes, bool with_opts, bool with_subids, bool with_src,
        uint64_t cap_in) {
  Out o;
  const uint64_t total = c.subs.size();
  const uint64_t room = std::min(total, cap_in);
  o.msgs.assign(room, 0xA5A5A5A5u);
  o.filters.assign(room, 0xA5A5A5A5u);
  if (with_opts) o.opts.assign(room, 0xA5);
  if (with_subids) o.subids.assign(room, 0xA5A5A5A5u);
  if (with_src) o.src.assign(room, 0xA5A5A5A5u);
  o.inbox_subs.assign(cap_boxes, 0xA5A5A5A5u);
  o.inbox_offsets.assign(cap_boxes + 1, 0xA5A5A5A5A5A5A5A5ull);
  emqx_inbox_batch b{};
  b.offsets = c.offsets.data();
  b.subs = c.subs.data();
  b.filters = c.filters.data();
  b.opts = with_opts ? c.opts.data() : nullptr;
  b.subids = with_subids ? c.subids.data() : nullptr;
  b.n = c.offsets.size() - 1;
  b.cap_in = cap_in;
  b.sub_limit = c.sub_limit;
  // (a vector of size 0 may hand out NULL: the stage requires the pointers only with capacity)
  b.box_msgs = o.msgs.data();
  b.box_filters = o.filters.data();
  b.box_opts = with_opts ? o.opts.data() : nullptr;
  b.box_subids = with_subids ? o.subids.data() : nullptr;
  b.box_src = with_src ? o.src.data() : nullptr;
  b.inbox_subs = o.inbox_subs.data();
  b.inbox_offsets = o.inbox_offsets.data();
  b.cap_boxes = cap_boxes;
  o.rc = emqx_inbox_group_host(h, &b, &o.n_boxes, o.summary);
  return o;
}

// The contract, from std::stable_sort.
void check(const Csr& c, const Out& o, uint64_t cap_boxes, bool with_opts, bool with_subids, bool with_src) {
  const uint64_t total = c.subs.size(), n = c.offsets.size() - 1;
  std::vector<uint32_t> perm(total);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return c.subs[x] < c.subs[y]; });
  std::vector<uint32_t> msg_of(total);
  uint64_t messages = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (c.offsets[i + 1] > c.offsets[i]) ++messages;
    for (uint64_t d = c.offsets[i]; d < c.offsets[i + 1]; ++d) msg_of[d] = static_cast<uint32_t>(i);
  }
  std::vector<uint32_t> ids;
  std::vector<uint64_t> starts;
  for (uint64_t k = 0; k < total; ++k) {
    CHECK(o.msgs[k] == msg_of[perm[k]]);
    CHECK(o.filters[k] == c.filters[perm[k]]);
    if (with_opts) CHECK(o.opts[k] == c.opts[perm[k]]);
    if (with_subids) CHECK(o.subids[k] == c.subids[perm[k]]);
    if (with_src) CHECK(o.src[k] == perm[k]);
    if (k == 0 || c.subs[perm[k]] != c.subs[perm[k - 1]]) {
      ids.push_back(c.subs[perm[k]]);
      starts.push_back(k);
    }
  }
  starts.push_back(total);
  const uint64_t m = ids.size();
  uint64_t longest = 0;
  for (uint64_t r = 0; r < m; ++r) longest = std::max(longest, starts[r + 1] - starts[r]);
  const bool over = m > cap_boxes;
  CHECK(o.rc == (over ? EMQX_EOVERFLOW : EMQX_OK));
  CHECK(o.n_boxes == m);
  CHECK(o.summary[0] == (over ? EMQX_INBOX_F_BOX_OVERFLOW : 0u));
  CHECK(o.summary[1] == total && o.summary[2] == m && o.summary[3] == longest && o.summary[4] == messages);
  CHECK(o.summary[5] == 0 && o.summary[6] == 0 && o.summary[7] == 0);
  const uint64_t shown = std::min(m, cap_boxes);
  for (uint64_t r = 0; r < shown; ++r) CHECK(o.inbox_subs[r] == ids[r]);
  for (uint64_t r = 0; r <= shown; ++r) CHECK(o.inbox_offsets[r] == starts[r]);
  for (uint64_t r = shown; r < cap_boxes; ++r) CHECK(o.inbox_subs[r] == 0xA5A5A5A5u);
  for (uint64_t r = shown + 1; r <= cap_boxes; ++r) CHECK(o.inbox_offsets[r] == 0xA5A5A5A5A5A5A5A5ull);
}

void round_trip(emqx_inbox* h, const Csr& c) {
  const uint64_t total = c.subs.size();
  const uint64_t fit = std::min<uint64_t>(total, c.sub_limit);
  const Out full = run(h, c, fit, true, true, true, total);
  check(c, full, fit, true, true, true);
  for (int skip = 0; skip < 3; ++skip) {
    const Out o = run(h, c, fit, skip != 0, skip != 1, skip != 2, total);
    check(c, o, fit, skip != 0, skip != 1, skip != 2);
  }
  const uint64_t m = full.n_boxes;
  for (uint64_t cap : {m ? m - 1 : 0, uint64_t{1}, uint64_t{0}}) {
    if (cap >= m) continue;
    const Out o = run(h, c, cap, true, true, true, total);
    check(c, o, cap, true, true, true);
  }
}

}  // namespace

int main() {
  emqx_inbox* h = nullptr;
  CHECK(emqx_inbox_create(0, &h) == EMQX_EDEVICE && h == nullptr);  // this build has no device
  CHECK(emqx_inbox_create(-7, &h) == EMQX_EINVAL);
  CHECK(emqx_inbox_create(EMQX_INBOX_HOST_ONLY, &h) == EMQX_OK && h);
  CHECK(emqx_inbox_reserve(h, 100, 100) == EMQX_EDEVICE);
  Rng r{42};
  const uint64_t limits[] = {1, 2, 255, 256, 257, 65536, 65537, 1ull << 24, (1ull << 24) + 1, 1ull << 32};
  uint64_t deliveries = 0;
  for (uint64_t limit : limits) {
    for (int kind = 0; kind < 2; ++kind) {
      const Csr c = make(r, 200, 40, limit, kind);
      deliveries += c.subs.size();
      round_trip(h, c);
    }
  }
  round_trip(h, make(r, 300, 30, 1ull << 20, 2));  // every delivery its own inbox, reversed
  round_trip(h, make(r, 3, 10000, 1000, 0));       // long messages
  round_trip(h, make(r, 0, 0, 16, 0));             // n = 0
  {
    Csr c = make(r, 5, 0, 16, 0);  // five empty messages
    CHECK(c.subs.empty());
    round_trip(h, c);
  }
  {
    // refusals: nothing but the summary is written
    Csr c = make(r, 50, 20, 100, 0);
    const uint64_t total = c.subs.size();
    CHECK(total > 10);
    Out o = run(h, c, total, true, true, true, total - 1);
    CHECK(o.rc == EMQX_EINVAL && o.summary[0] == EMQX_INBOX_F_INPUT_REFUSED && o.summary[1] == total && o.summary[2] == 0);
    for (uint32_t v : o.msgs) CHECK(v == 0xA5A5A5A5u);
    for (uint64_t v : o.inbox_offsets) CHECK(v == 0xA5A5A5A5A5A5A5A5ull);
    c.subs[total / 2] = 100;  // == sub_limit
    o = run(h, c, total, true, true, true, total);
    CHECK(o.rc == EMQX_EINVAL && o.summary[0] == EMQX_INBOX_F_BAD_SUB && o.summary[1] == total && o.summary[2] == 0);
    c.subs[total / 2] = 99;
    const uint64_t keep = c.offsets[3];
    c.offsets[3] = c.offsets[4] + 1;  // a decrease behind it
    o = run(h, c, total, true, true, true, total);
    CHECK(o.rc == EMQX_EINVAL);
    c.offsets[3] = keep;
    c.offsets[0] = 1;
    o = run(h, c, total, true, true, true, total);
    CHECK(o.rc == EMQX_EINVAL);
    for (uint32_t v : o.msgs) CHECK(v == 0xA5A5A5A5u);
  }
  {
    emqx_inbox_stats s{};
    s.size = sizeof(s);
    CHECK(emqx_inbox_stats_get(h, &s) == EMQX_OK && s.size == sizeof(s) && s.calls > 100 && s.last_passes >= 1);
    CHECK(emqx_inbox_set_tuning(h, "path", 1) == EMQX_OK && emqx_inbox_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
    CHECK(emqx_inbox_set_tuning(h, "max_blocks", 2) == EMQX_OK && emqx_inbox_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
  }
  CHECK(emqx_inbox_destroy(h) == EMQX_OK);
  CHECK(emqx_inbox_destroy(nullptr) == EMQX_EINVAL);
  std::printf("inbox host ok: %llu deliveries\n", static_cast<unsigned long long>(deliveries));
  return 0;
}
