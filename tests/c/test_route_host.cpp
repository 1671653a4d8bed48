// Stand-alone program over the host-only build of the route table (emqx_amd/csrc/route.cpp with
// EMQX_ROUTE_NO_DEVICE): a generated bag of dests over 600 filter ids and up to 64 nodes (plain
// routes on one to four nodes, a few on every node, grouped dests with one group on several
// nodes), changed by add / remove / purge, and CSRs with empty messages, one 5 000-entry message,
// repeated and unknown ids and n = 0, checked against a checker written here from the contract
// of include/emqx_route.h with std::map and std::set.  Run plainly and under ASan + UBSan
// (tests/test_route_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../include/emqx_route.h"

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
    return static_cast<uint32_t>(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

using Dest = std::pair<uint32_t, uint32_t>;               // (node, group)
using Bag = std::map<uint32_t, std::vector<Dest>>;        // filter -> dests in insertion order

struct Csr {
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> filters;
  void message(Rng& r, uint32_t count, uint32_t n_filters) {
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t kind = r.below(40);
      filters.push_back(kind == 0 ? 0xFFFFFFFFu : kind == 1 ? n_filters + r.below(50) : kind == 2 ? (1u << 30) : r.below(n_filters));
    }
    if (count >= 2) filters.back() = filters[filters.size() - count];  // one id twice
    offsets.push_back(filters.size());
  }
};

void add(emqx_routetab* h, Bag& bag, uint32_t f, uint32_t v, uint32_t g) {
  CHECK(emqx_routetab_add(h, &f, &v, g == EMQX_NO_GROUP ? nullptr : &g, 1) == EMQX_OK);
  auto& d = bag[f];
  if (std::find(d.begin(), d.end(), Dest{v, g}) == d.end()) d.push_back({v, g});
}

void run(emqx_routetab* h, const Bag& bag, uint32_t local, const Csr& c) {
  const uint64_t n = c.offsets.size() - 1, total = c.filters.size();
  std::vector<uint8_t> want_flags(total);
  std::vector<uint32_t> want_routes(n), want_local;
  std::vector<uint64_t> want_loff(n + 1);
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> lists(EMQX_ROUTE_MAX_NODES);
  uint64_t dropped = 0, fwd_msgs = 0, unknown = 0;
  for (uint64_t i = 0; i < n; ++i) {
    want_loff[i] = want_local.size();
    bool fwd = false;
    for (uint64_t d = c.offsets[i]; d < c.offsets[i + 1]; ++d) {
      const auto it = bag.find(c.filters[d]);
      uint8_t fl = 0;
      if (it != bag.end()) {
        std::set<uint32_t> groups;
        for (const Dest& x : it->second) {
          if (x.second != EMQX_NO_GROUP) {
            groups.insert(x.second);
          } else if (x.first == local) {
            fl |= EMQX_ROUTE_LOCAL;
            ++want_routes[i];
          } else {
            fl |= EMQX_ROUTE_REMOTE;
            ++want_routes[i];
            lists[x.first].push_back({static_cast<uint32_t>(i), c.filters[d]});
            fwd = true;
          }
        }
        if (!groups.empty()) fl |= EMQX_ROUTE_SHARE;
        want_routes[i] += static_cast<uint32_t>(groups.size());
      }
      want_flags[d] = fl;
      unknown += fl == 0;
      if (fl & (EMQX_ROUTE_LOCAL | EMQX_ROUTE_SHARE)) want_local.push_back(c.filters[d]);
    }
    dropped += want_routes[i] == 0;
    fwd_msgs += fwd;
  }
  want_loff[n] = want_local.size();
  uint64_t forwards = 0, nodes = 0;
  for (const auto& l : lists) {
    forwards += l.size();
    nodes += !l.empty();
  }

  std::vector<uint8_t> flags(total + 1, 0xEE);
  std::vector<uint32_t> routes(n + 1, 0xEEEEEEEE), fm(forwards + 1, 0xEEEEEEEE), ff(forwards + 1, 0xEEEEEEEE),
      lfil(total + 1, 0xEEEEEEEE);
  std::vector<uint64_t> node_off(EMQX_ROUTE_MAX_NODES + 2, ~0ull), loff(n + 2, ~0ull);
  struct emqx_route_batch b{};
  b.offsets = c.offsets.data();
  b.filters = c.filters.data();
  b.n = n;
  b.cap_in = total;
  b.entry_flags = flags.data();
  b.msg_routes = routes.data();
  b.node_offsets = node_off.data();
  b.fwd_msgs = fm.data();
  b.fwd_filters = ff.data();
  b.cap_fwd = forwards;  // exactly enough
  b.local_offsets = loff.data();
  b.local_filters = lfil.data();
  uint64_t n_fwd = ~0ull, sum[EMQX_ROUTE_SUMMARY_WORDS];
  CHECK(emqx_route_host(h, &b, &n_fwd, sum) == EMQX_OK);
  CHECK(n_fwd == forwards);
  CHECK(flags[total] == 0xEE && routes[n] == 0xEEEEEEEE && fm[forwards] == 0xEEEEEEEE && ff[forwards] == 0xEEEEEEEE);
  CHECK(lfil[total] == 0xEEEEEEEE && node_off[EMQX_ROUTE_MAX_NODES + 1] == ~0ull && loff[n + 1] == ~0ull);
  for (uint64_t d = 0; d < total; ++d) CHECK(flags[d] == want_flags[d]);
  for (uint64_t i = 0; i < n; ++i) CHECK(routes[i] == want_routes[i]);
  for (uint64_t i = 0; i <= n; ++i) CHECK(loff[i] == want_loff[i]);
  for (uint64_t k = 0; k < want_local.size(); ++k) CHECK(lfil[k] == want_local[k]);
  CHECK(node_off[0] == 0 && node_off[EMQX_ROUTE_MAX_NODES] == forwards);
  for (uint32_t v = 0; v < EMQX_ROUTE_MAX_NODES; ++v) {
    CHECK(node_off[v + 1] - node_off[v] == lists[v].size());
    for (uint64_t k = 0; k < lists[v].size(); ++k)
      CHECK(fm[node_off[v] + k] == lists[v][k].first && ff[node_off[v] + k] == lists[v][k].second);
  }
  CHECK(lists[local].empty());
  CHECK(sum[0] == 0 && sum[1] == total && sum[2] == forwards && sum[3] == dropped && sum[4] == fwd_msgs);
  CHECK(sum[5] == want_local.size() && sum[6] == unknown && sum[7] == nodes);
  if (forwards > 0) {  // one short: node_offsets complete, the lists untouched
    std::vector<uint32_t> untouched(forwards, 0xEEEEEEEE);
    std::vector<uint64_t> node_off2(EMQX_ROUTE_MAX_NODES + 1, ~0ull);
    b.fwd_msgs = b.fwd_filters = untouched.data();
    b.node_offsets = node_off2.data();
    b.cap_fwd = forwards - 1;
    b.entry_flags = nullptr;  // the optional outputs left out
    b.local_offsets = nullptr;
    b.local_filters = nullptr;
    CHECK(emqx_route_host(h, &b, &n_fwd, sum) == EMQX_EOVERFLOW);
    CHECK(n_fwd == forwards && (sum[0] & EMQX_ROUTE_F_FWD_OVERFLOW) && sum[2] == forwards && sum[5] == want_local.size());
    for (uint32_t v = 0; v <= EMQX_ROUTE_MAX_NODES; ++v) CHECK(node_off2[v] == node_off[v]);
    for (uint32_t x : untouched) CHECK(x == 0xEEEEEEEE);
  }
}

void same_lookup(emqx_routetab* h, const Bag& bag, uint32_t n_filters) {
  for (uint32_t f = 0; f < n_filters; ++f) {
    uint32_t nodes[256], groups[256];
    uint64_t n = ~0ull;
    CHECK(emqx_routetab_lookup(h, f, nodes, groups, 256, &n) == EMQX_OK);
    const auto it = bag.find(f);
    CHECK(n == (it == bag.end() ? 0 : it->second.size()));
    for (uint64_t k = 0; k < n; ++k) CHECK(nodes[k] == it->second[k].first && groups[k] == it->second[k].second);
  }
}

}  // namespace

int main() {
  constexpr uint32_t N_FILTERS = 600, LOCAL = 5;
  emqx_routetab* h = nullptr;
  CHECK(emqx_routetab_create(0, LOCAL, &h) == EMQX_EDEVICE && h == nullptr);  // this build has no device
  CHECK(emqx_routetab_create(EMQX_ROUTE_HOST_ONLY, EMQX_ROUTE_MAX_NODES, &h) == EMQX_EINVAL);
  CHECK(emqx_routetab_create(EMQX_ROUTE_HOST_ONLY, LOCAL, &h) == EMQX_OK && h);
  CHECK(emqx_routetab_set_tuning(h, "max_blocks", 7) == EMQX_OK && emqx_routetab_set_tuning(h, "path", 1) == EMQX_OK);
  CHECK(emqx_routetab_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
  CHECK(emqx_routetab_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
  Rng r{4242};
  Bag bag;
  Csr before;  // against the empty table: nothing is known
  for (uint32_t c : {3u, 0u, 2u}) before.message(r, c, N_FILTERS);
  run(h, bag, LOCAL, before);
  for (uint32_t f = 0; f < N_FILTERS; ++f) {
    if (f % 11 == 10) continue;  // an id without a dest
    const uint32_t span = f % 3 == 0 ? 64 : 8;
    const uint32_t plain = f % 97 == 0 ? 64 : f % 13 == 12 ? 0 : 1 + (r.below(10) == 0 ? r.below(4) : 0);
    for (uint32_t k = 0; k < plain; ++k) add(h, bag, f, plain == 64 ? k : r.below(span), EMQX_NO_GROUP);
    if (f % 13 == 12 || r.below(8) == 0) {
      const uint32_t g = r.below(5);
      add(h, bag, f, r.below(span), g);
      add(h, bag, f, r.below(span), g);  // the same group on another node counts once
      if (r.below(2)) add(h, bag, f, r.below(span), g + 5);
    }
    if (f % 7 == 0) add(h, bag, f, bag[f][0].first, bag[f][0].second);  // idempotent
  }
  const uint32_t bad_f = EMQX_ROUTE_MAX_FILTER, bad_v = EMQX_ROUTE_MAX_NODES, zero = 0;
  CHECK(emqx_routetab_add(h, &bad_f, &zero, nullptr, 1) == EMQX_EINVAL);
  CHECK(emqx_routetab_add(h, &zero, &bad_v, nullptr, 1) == EMQX_EINVAL);
  CHECK(emqx_routetab_remove(h, &zero, &bad_v, nullptr, 1) == EMQX_EINVAL);
  CHECK(emqx_routetab_add(h, nullptr, &zero, nullptr, 1) == EMQX_EINVAL);
  same_lookup(h, bag, N_FILTERS + 5);
  CHECK(emqx_routetab_commit(h) == EMQX_OK);
  emqx_routetab_stats st{};
  st.size = sizeof(st);
  CHECK(emqx_routetab_stats_get(h, &st) == EMQX_OK);
  uint64_t plain = 0, grouped = 0;
  for (const auto& kv : bag)
    for (const Dest& d : kv.second) (d.second == EMQX_NO_GROUP ? plain : grouped) += 1;
  CHECK(st.n_filters == bag.size() && st.n_plain == plain && st.n_grouped == grouped && st.n_nodes == 64 && st.epoch == 1);
  std::printf("%llu filters, %llu plain and %llu grouped routes on %llu nodes\n",
              static_cast<unsigned long long>(st.n_filters), static_cast<unsigned long long>(st.n_plain),
              static_cast<unsigned long long>(st.n_grouped), static_cast<unsigned long long>(st.n_nodes));

  Csr empty;  // n = 0
  run(h, bag, LOCAL, empty);
  Csr big_one;  // empty messages around one 5 000-entry message
  for (uint32_t c : {0u, 0u, 1u, 5000u, 0u, 3u, 0u}) big_one.message(r, c, N_FILTERS);
  run(h, bag, LOCAL, big_one);
  Csr many;
  for (int i = 0; i < 2000; ++i) many.message(r, r.below(4) == 0 ? 0 : r.below(40), N_FILTERS);
  run(h, bag, LOCAL, many);

  // remove acts at the next commit; absent triples are ignored
  Bag old = bag;
  for (auto it = bag.begin(); it != bag.end();) {
    if (it->first % 5 == 0) {
      const Dest d = it->second.front();
      const uint32_t f = it->first;
      CHECK(emqx_routetab_remove(h, &f, &d.first, &d.second, 1) == EMQX_OK);
      CHECK(emqx_routetab_remove(h, &f, &d.first, &d.second, 1) == EMQX_OK);
      it->second.erase(it->second.begin());
      if (it->second.empty()) {
        it = bag.erase(it);
        continue;
      }
    }
    ++it;
  }
  run(h, old, LOCAL, many);  // the committed snapshot still answers
  same_lookup(h, bag, N_FILTERS);
  CHECK(emqx_routetab_commit(h) == EMQX_OK);
  run(h, bag, LOCAL, many);

  // a node goes down
  const uint32_t gone = 2;
  const Bag pre = bag;
  std::vector<uint32_t> want_emptied;
  for (auto it = bag.begin(); it != bag.end();) {
    auto& d = it->second;
    d.erase(std::remove_if(d.begin(), d.end(), [](const Dest& x) { return x.first == gone; }), d.end());
    if (d.empty()) {
      want_emptied.push_back(it->first);
      it = bag.erase(it);
    } else {
      ++it;
    }
  }
  CHECK(want_emptied.size() >= 2);
  std::vector<uint32_t> emptied(want_emptied.size(), 0xEEEEEEEE);
  uint64_t n_emptied = 0;
  CHECK(emqx_routetab_purge_node(h, gone, emptied.data(), emptied.size() - 1, &n_emptied) == EMQX_EOVERFLOW);
  CHECK(n_emptied == want_emptied.size() && emptied[0] == 0xEEEEEEEE);
  same_lookup(h, pre, N_FILTERS);  // nothing was removed
  CHECK(emqx_routetab_purge_node(h, gone, emptied.data(), emptied.size(), &n_emptied) == EMQX_OK);
  CHECK(n_emptied == want_emptied.size() && emptied == want_emptied);
  same_lookup(h, bag, N_FILTERS);
  CHECK(emqx_routetab_commit(h) == EMQX_OK);
  CHECK(emqx_routetab_stats_get(h, &st) == EMQX_OK && st.n_filters == bag.size() && st.epoch == 3 && st.n_nodes == 63);
  run(h, bag, LOCAL, many);
  run(h, bag, LOCAL, big_one);

  // refused inputs
  struct emqx_route_batch b{};
  const uint64_t dec[3] = {0, 2, 1};
  const uint32_t two[2] = {1, 2};
  uint32_t routes[2], fm[8], ff[8];
  uint64_t node_off[EMQX_ROUTE_MAX_NODES + 1];
  b.offsets = dec;
  b.filters = two;
  b.n = 2;
  b.cap_in = 2;
  b.msg_routes = routes;
  b.node_offsets = node_off;
  b.fwd_msgs = fm;
  b.fwd_filters = ff;
  b.cap_fwd = 8;
  CHECK(emqx_route_host(h, &b, nullptr, nullptr) == EMQX_EINVAL);
  const uint64_t over[3] = {0, 1, 3};  // offsets[n] > cap_in
  b.offsets = over;
  CHECK(emqx_route_host(h, &b, nullptr, nullptr) == EMQX_EINVAL);
  const uint64_t fine[3] = {0, 1, 2};
  b.offsets = fine;
  CHECK(emqx_route_host(h, &b, nullptr, nullptr) == EMQX_OK);
  CHECK(emqx_route_batch(h, &b, nullptr, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_route_batch_device(h, &b, nullptr, nullptr, nullptr) == EMQX_EDEVICE);
  uint64_t sum[8];
  CHECK(emqx_route_batch_device_async(h, &b, sum, nullptr) == EMQX_EDEVICE);
  CHECK(emqx_routetab_destroy(h) == EMQX_OK);
  std::printf("route host ok\n");
  return 0;
}
