// Stand-alone program over the host-only build of the owner table (emqx_amd/csrc/select.cpp
// with EMQX_SELECT_NO_DEVICE): a generated table of 3 000 owners over 500 filter ids (lists of
// 0..3 and 65 ids, duplicates within a list, disabled and match-all owners), CSRs with empty
// messages, one 3 000-entry message, repeated and unknown ids and n = 0, under every kind of
// class mask, checked against a checker written here from the contract of
// include/emqx_select.h with std::set.  Run plainly and under ASan + UBSan
// (tests/test_select_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../../include/emqx_select.h"

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
    return static_cast<uint32_t>(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

struct Rec {
  uint32_t class_bit, flags;
  std::set<uint32_t> filters;
};
using Table = std::map<uint32_t, Rec>;

struct Csr {
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> filters, classes;
  void message(Rng& r, uint32_t count, uint32_t n_filters) {
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t kind = r.below(30);
      filters.push_back(kind == 0 ? 0xFFFFFFFFu : kind == 1 ? n_filters + r.below(50) : r.below(n_filters));
    }
    if (count >= 2) filters.back() = filters[filters.size() - count];  // one id twice
    offsets.push_back(filters.size());
    const uint32_t m = r.below(6);
    classes.push_back(m == 0 ? 0u : m == 1 ? EMQX_SELECT_ALL_CLASSES : m == 2 ? 1u : m == 3 ? (1u << 31) : r.next());
  }
};

void run(emqx_owntab* h, const Table& t, const Csr& c, bool with_classes) {
  const uint64_t n = c.offsets.size() - 1, total = c.filters.size();
  std::map<uint32_t, std::set<uint32_t>> post;
  std::set<uint32_t> every;
  for (const auto& kv : t) {
    if (kv.second.flags & EMQX_OWNER_MATCH_ALL) every.insert(kv.first);
    else
      for (uint32_t f : kv.second.filters) post[f].insert(kv.first);
  }
  // the expected sets
  std::vector<std::vector<uint32_t>> want(n);
  uint64_t selected = 0, postings = 0, dups = 0, unknown = 0, msgs = 0, most = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t mask = with_classes ? c.classes[i] : EMQX_SELECT_ALL_CLASSES;
    auto ok = [&](uint32_t o) {
      const Rec& r = t.at(o);
      return (r.flags & EMQX_OWNER_ENABLED) && ((mask >> r.class_bit) & 1u);
    };
    std::set<uint32_t> got;
    uint64_t passing = 0;
    for (uint64_t d = c.offsets[i]; d < c.offsets[i + 1]; ++d) {
      const auto it = post.find(c.filters[d]);
      if (it == post.end()) {
        ++unknown;
        continue;
      }
      postings += it->second.size();
      for (uint32_t o : it->second)
        if (ok(o)) {
          ++passing;
          got.insert(o);
        }
    }
    dups += passing - got.size();
    for (uint32_t o : every)
      if (ok(o)) got.insert(o);
    want[i].assign(got.begin(), got.end());
    selected += got.size();
    msgs += !got.empty();
    most = std::max<uint64_t>(most, got.size());
  }
  std::vector<uint64_t> ooff(n + 1, ~0ull);
  std::vector<uint32_t> owners(selected + 1, 0xEEEEEEEE);
  struct emqx_select_batch b{};
  b.offsets = c.offsets.data();
  b.filters = c.filters.data();
  b.n = n;
  b.cap_in = total;
  b.msg_classes = with_classes ? c.classes.data() : nullptr;
  b.out_offsets = ooff.data();
  b.out_owners = owners.data();
  b.cap_out = selected;  // exactly enough
  uint64_t n_out = ~0ull, sum[EMQX_SELECT_SUMMARY_WORDS];
  CHECK(emqx_select_host(h, &b, &n_out, sum) == EMQX_OK);
  CHECK(n_out == selected && ooff[0] == 0 && ooff[n] == selected);
  CHECK(owners[selected] == 0xEEEEEEEE);  // nothing past the end
  for (uint64_t i = 0; i < n; ++i) {
    std::vector<uint32_t> got(owners.begin() + ooff[i], owners.begin() + ooff[i + 1]);
    std::sort(got.begin(), got.end());
    CHECK(got == want[i]);  // the same set, no owner twice
  }
  CHECK(sum[0] == 0 && sum[1] == total && sum[2] == postings && sum[3] == selected && sum[4] == msgs);
  CHECK(sum[5] == dups && sum[6] == unknown && sum[7] == most);
  if (selected > 0) {  // one short: offsets complete, owners untouched
    std::vector<uint32_t> untouched(selected, 0xEEEEEEEE);
    std::vector<uint64_t> ooff2(n + 1, ~0ull);
    b.out_owners = untouched.data();
    b.out_offsets = ooff2.data();
    b.cap_out = selected - 1;
    CHECK(emqx_select_host(h, &b, &n_out, sum) == EMQX_EOVERFLOW);
    CHECK(n_out == selected && ooff2 == ooff && (sum[0] & EMQX_SELECT_F_OUT_OVERFLOW) && sum[3] == selected);
    for (uint32_t x : untouched) CHECK(x == 0xEEEEEEEE);
  }
}

}  // namespace

int main() {
  constexpr uint32_t N_FILTERS = 500, N_OWNERS = 3000;
  emqx_owntab* h = nullptr;
  CHECK(emqx_owntab_create(0, &h) == EMQX_EDEVICE && h == nullptr);  // this build has no device
  CHECK(emqx_owntab_create(EMQX_SELECT_HOST_ONLY, &h) == EMQX_OK && h);
  CHECK(emqx_owntab_set_tuning(h, "max_blocks", 7) == EMQX_OK && emqx_owntab_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
  CHECK(emqx_owntab_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
  Rng r{977};
  Table t;
  for (uint32_t k = 0; k < N_OWNERS; ++k) {
    const uint32_t owner = 2 * k + r.below(2);  // sparse ids
    Rec rec{r.below(32), (r.below(9) ? EMQX_OWNER_ENABLED : 0u) | (k % 500 == 7 ? EMQX_OWNER_MATCH_ALL : 0u), {}};
    std::vector<uint32_t> ids;
    const uint32_t size = k % 97 == 0 ? 65 : r.below(4);
    for (uint32_t j = 0; j < size; ++j) ids.push_back(r.below(N_FILTERS));
    if (size >= 2) ids.push_back(ids[0]);  // a duplicate within the list
    if (k % 3 == 0) ids.push_back(N_FILTERS - 1 - k % 2);  // two crowded lists
    rec.filters.insert(ids.begin(), ids.end());
    CHECK(emqx_owntab_set(h, owner, rec.class_bit, rec.flags, ids.data(), ids.size()) == EMQX_OK);
    t[owner] = rec;
  }
  // rejected calls change nothing
  const uint32_t one = 1, big = EMQX_SELECT_MAX_FILTER;
  CHECK(emqx_owntab_set(h, 1, 32, EMQX_OWNER_ENABLED, &one, 1) == EMQX_EINVAL);
  CHECK(emqx_owntab_set(h, 1, 0, 4, &one, 1) == EMQX_EINVAL);
  CHECK(emqx_owntab_set(h, 1, 0, EMQX_OWNER_ENABLED, &big, 1) == EMQX_EINVAL);
  CHECK(emqx_owntab_set(h, EMQX_SELECT_MAX_OWNER, 0, EMQX_OWNER_ENABLED, &one, 1) == EMQX_EINVAL);
  CHECK(emqx_owntab_set(h, 1, 0, EMQX_OWNER_ENABLED, nullptr, 1) == EMQX_EINVAL);
  CHECK(emqx_owntab_commit(h) == EMQX_OK);
  emqx_owntab_stats st{};
  st.size = sizeof(st);
  CHECK(emqx_owntab_stats_get(h, &st) == EMQX_OK);
  CHECK(st.n_owners == t.size() && st.epoch == 1 && st.n_match_all == 6 && st.max_list >= 400 && st.n_filters <= N_FILTERS);
  std::printf("%llu owners, %llu postings over %llu filters, longest list %llu\n",
              static_cast<unsigned long long>(st.n_owners), static_cast<unsigned long long>(st.n_postings),
              static_cast<unsigned long long>(st.n_filters), static_cast<unsigned long long>(st.max_list));

  Csr empty;  // n = 0
  run(h, t, empty, true);
  Csr big_one;  // empty messages around one 3 000-entry message
  for (uint32_t c : {0u, 0u, 1u, 3000u, 0u, 3u, 0u}) big_one.message(r, c, N_FILTERS);
  run(h, t, big_one, true);
  run(h, t, big_one, false);
  Csr many;
  for (int i = 0; i < 2000; ++i) many.message(r, r.below(4) == 0 ? 0 : r.below(40), N_FILTERS);
  run(h, t, many, true);

  // enable and remove act at the next commit
  std::vector<uint32_t> off, gone;
  for (auto it = t.begin(); it != t.end();) {
    if (it->first % 7 == 0) {
      gone.push_back(it->first);
      it = t.erase(it);
      continue;
    }
    if (it->first % 5 == 0) {
      off.push_back(it->first);
      it->second.flags &= ~EMQX_OWNER_ENABLED;
    }
    ++it;
  }
  gone.push_back(2 * N_OWNERS + 11);  // an unknown owner is ignored
  off.push_back(2 * N_OWNERS + 12);
  CHECK(emqx_owntab_enable(h, off.data(), off.size(), 0) == EMQX_OK);
  CHECK(emqx_owntab_remove(h, gone.data(), gone.size()) == EMQX_OK);
  CHECK(emqx_owntab_commit(h) == EMQX_OK);
  CHECK(emqx_owntab_stats_get(h, &st) == EMQX_OK && st.n_owners == t.size() && st.epoch == 2);
  run(h, t, many, true);
  run(h, t, big_one, true);

  // refused inputs
  struct emqx_select_batch b{};
  const uint64_t dec[3] = {0, 2, 1};
  const uint32_t two[2] = {1, 2};
  uint64_t ooff[3];
  uint32_t own[8];
  b.offsets = dec;
  b.filters = two;
  b.n = 2;
  b.cap_in = 2;
  b.out_offsets = ooff;
  b.out_owners = own;
  b.cap_out = 8;
  CHECK(emqx_select_host(h, &b, nullptr, nullptr) == EMQX_EINVAL);
  const uint64_t over[3] = {0, 1, 3};  // offsets[n] > cap_in
  b.offsets = over;
  CHECK(emqx_select_host(h, &b, nullptr, nullptr) == EMQX_EINVAL);
  CHECK(emqx_select_batch(h, &b, nullptr, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_select_batch_device(h, &b, nullptr, nullptr, nullptr) == EMQX_EDEVICE);
  uint64_t sum[8];
  CHECK(emqx_select_batch_device_async(h, &b, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_owntab_destroy(h) == EMQX_OK);
  std::printf("select host ok\n");
  return 0;
}
