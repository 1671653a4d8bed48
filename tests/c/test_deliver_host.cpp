// Stand-alone program over the host-only build of the delivery-options table
// (emqx_amd/csrc/deliver.cpp with EMQX_DELIVER_NO_DEVICE): a generated table of 20 K entries at
// max_load_pct 50 and 90, CSRs with empty messages, one 10 000-delivery message and n = 0,
// checked against a checker written here from the same Erlang lines
// (apps/emqx/src/emqx_session.erl:280-291, :569-598).  Run plainly and under ASan + UBSan
// (tests/test_deliver_host_san.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../include/emqx_deliver.h"

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

struct SubOpt {
  int qos, nl, rap;
  bool upgrade;
  uint32_t subid;  // 0: the map has no subid key
};
using Table = std::map<std::pair<uint32_t, uint32_t>, SubOpt>;  // (filter, subscriber)

// One delivery as the reference treats it.
void expect(const Table& t, uint32_t sub, uint32_t word, uint32_t qos, uint32_t flags, uint32_t from, uint8_t* byte,
            uint32_t* subid) {
  *subid = 0;
  if (qos > 2 || (flags & ~3u)) {
    *byte = EMQX_DELIVER_BAD_MESSAGE;
    return;
  }
  bool retain = flags & EMQX_MSG_RETAIN;
  const bool retained_hdr = flags & EMQX_MSG_RETAINED;
  const uint32_t f = word & ~(EMQX_FANOUT_SHARED_BIT | EMQX_FANOUT_RETRY_BIT);
  const auto it = t.find({f, sub});  // maps:find(Topic, Subs), :283 and :570
  uint32_t out = 0;
  if (it == t.end()) {  // :288 _ -> false; :575 error -> []; :578 [] -> Msg
    out = qos | EMQX_DELIVER_NO_SUBOPTS;
  } else {
    const SubOpt& o = it->second;
    if (o.nl == 1 && from != EMQX_DELIVER_NO_SENDER && sub == from) out |= EMQX_DELIVER_DROP_NO_LOCAL;  // :284-287
    if (o.nl == 1) out |= EMQX_DELIVER_NL;                                                              // :579-580
    out |= o.upgrade ? (static_cast<uint32_t>(o.qos) > qos ? o.qos : qos)                               // :583-585
                     : (static_cast<uint32_t>(o.qos) < qos ? o.qos : qos);                              // :586-588
    if (o.rap == 0 && !retained_hdr) retain = false;                                                    // :589-594
    *subid = o.subid;                                                                                   // :595-598
  }
  if (retain) out |= EMQX_DELIVER_RETAIN;
  *byte = static_cast<uint8_t>(out);
}

struct Csr {
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> subs, filters, from;
  std::vector<uint8_t> qos, flags;
  void message(Rng& r, uint32_t count, uint32_t n_filters, uint32_t n_subs) {
    const uint32_t sender = r.below(n_subs);
    for (uint32_t k = 0; k < count; ++k) {
      subs.push_back(r.below(4) == 0 ? sender : r.below(n_subs));
      uint32_t w = r.below(n_filters + n_filters / 4);  // a fifth of the filters is in no key
      if (r.below(5) == 0) w |= EMQX_FANOUT_SHARED_BIT | (r.below(2) ? EMQX_FANOUT_RETRY_BIT : 0u);
      filters.push_back(w);
    }
    offsets.push_back(subs.size());
    const uint32_t kind = r.below(50);
    qos.push_back(kind == 0 ? 3 : static_cast<uint8_t>(r.below(3)));
    flags.push_back(static_cast<uint8_t>(kind == 1 ? 0x80 : r.below(4)));
    from.push_back(r.below(8) == 0 ? EMQX_DELIVER_NO_SENDER : sender);
  }
};

void run(emqx_subopts* h, const Table& t, const Csr& c, bool with_from) {
  const uint64_t n = c.offsets.size() - 1, total = c.subs.size();
  std::vector<uint8_t> opts(total + 1, 0xEE), kopts(total + 1, 0xEE);
  std::vector<uint32_t> ids(total + 1, 0xEEEEEEEE), ksubs(total + 1, 0xEEEEEEEE), kfil(total + 1, 0xEEEEEEEE),
      kids(total + 1, 0xEEEEEEEE);
  std::vector<uint64_t> koff(n + 1, ~0ull);
  emqx_deliver_batch b{};
  b.offsets = c.offsets.data();
  b.subs = c.subs.data();
  b.filters = c.filters.data();
  b.n = n;
  b.cap_in = total;
  b.msg_qos = c.qos.data();
  b.msg_flags = c.flags.data();
  b.msg_from = with_from ? c.from.data() : nullptr;
  b.out_opts = opts.data();
  b.out_subids = ids.data();
  b.kept_offsets = koff.data();
  b.kept_subs = ksubs.data();
  b.kept_filters = kfil.data();
  b.kept_opts = kopts.data();
  b.kept_subids = kids.data();
  b.cap_kept = total;
  uint64_t n_kept = ~0ull, sum[EMQX_DELIVER_SUMMARY_WORDS];
  CHECK(emqx_deliver_enrich_host(h, &b, &n_kept, sum) == EMQX_OK);
  uint64_t pos = 0, dropped = 0, none = 0, by_qos[3] = {0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(koff[i] == pos);
    for (uint64_t d = c.offsets[i]; d < c.offsets[i + 1]; ++d) {
      uint8_t byte;
      uint32_t subid;
      expect(t, c.subs[d], c.filters[d], c.qos[i], c.flags[i], with_from ? c.from[i] : EMQX_DELIVER_NO_SENDER, &byte,
             &subid);
      CHECK(opts[d] == byte);
      CHECK(ids[d] == subid);
      none += (byte & EMQX_DELIVER_NO_SUBOPTS) != 0;
      if (byte & EMQX_DELIVER_DROP_NO_LOCAL) {
        ++dropped;
        continue;
      }
      CHECK(ksubs[pos] == c.subs[d] && kfil[pos] == c.filters[d] && kopts[pos] == byte && kids[pos] == subid);
      if (!(byte & EMQX_DELIVER_BAD_MESSAGE)) ++by_qos[byte & 3];
      ++pos;
    }
  }
  CHECK(koff[n] == pos && n_kept == pos);
  CHECK(opts[total] == 0xEE && kopts[pos] == 0xEE && ksubs[pos] == 0xEEEEEEEE);  // nothing past the end
  CHECK(sum[0] == 0 && sum[1] == total && sum[2] == pos && sum[3] == dropped && sum[4] == none);
  CHECK(sum[5] == by_qos[0] && sum[6] == by_qos[1] && sum[7] == by_qos[2]);
  if (with_from && total > 100) CHECK(dropped > 0 && dropped < total);
  // annotate only, and a kept capacity one short
  b.kept_offsets = nullptr;
  std::vector<uint8_t> opts2(total + 1, 0xEE);
  b.out_opts = opts2.data();
  CHECK(emqx_deliver_enrich_host(h, &b, nullptr, nullptr) == EMQX_OK);
  CHECK(opts2 == opts);
  if (pos > 0) {
    b.kept_offsets = koff.data();
    b.cap_kept = pos - 1;
    std::vector<uint32_t> untouched(total + 1, 0xEEEEEEEE);
    b.kept_subs = untouched.data();
    CHECK(emqx_deliver_enrich_host(h, &b, &n_kept, sum) == EMQX_EOVERFLOW);
    CHECK(n_kept == pos && koff[n] == pos && (sum[0] & EMQX_DELIVER_F_KEPT_OVERFLOW));
    for (uint32_t x : untouched) CHECK(x == 0xEEEEEEEE);
  }
}

}  // namespace

int main() {
  constexpr uint32_t N_FILTERS = 200, N_SUBS = 1000, N_ENTRIES = 20000;
  for (int pct : {50, 90}) {
    emqx_subopts* h = nullptr;
    CHECK(emqx_subopts_create(0, &h) == EMQX_EDEVICE && h == nullptr);  // this build has no device
    CHECK(emqx_subopts_create(EMQX_DELIVER_HOST_ONLY, &h) == EMQX_OK && h);
    CHECK(emqx_subopts_set_tuning(h, "max_load_pct", pct) == EMQX_OK);
    CHECK(emqx_subopts_set_tuning(h, "nope", 1) == EMQX_ENOTFOUND);
    CHECK(emqx_subopts_set_tuning(h, "max_blocks", 2) == EMQX_OK && emqx_subopts_set_tuning(h, "scan_chunk", 3) == EMQX_OK);
    Rng r{static_cast<uint64_t>(pct) * 977};
    Table t;
    std::vector<uint32_t> f, s, ids;
    std::vector<uint8_t> w;
    while (t.size() < N_ENTRIES) {
      const uint32_t fi = r.below(N_FILTERS), si = r.below(N_SUBS);
      SubOpt o{static_cast<int>(r.below(3)), static_cast<int>(r.below(2)), static_cast<int>(r.below(2)), si % 3 == 0,
               r.below(2) ? 1 + r.below(EMQX_DELIVER_MAX_SUBID) : 0};
      t[{fi, si}] = o;  // a later set of the same pair replaces the earlier one, here and there
      f.push_back(fi);
      s.push_back(si);
      ids.push_back(o.subid);
      w.push_back(static_cast<uint8_t>(o.qos | (o.nl ? EMQX_SUBOPT_NL : 0) | (o.rap ? EMQX_SUBOPT_RAP : 0) |
                                       (o.upgrade ? EMQX_SUBOPT_UPGRADE_QOS : 0) | (o.subid ? EMQX_SUBOPT_HAS_SUBID : 0)));
    }
    CHECK(emqx_subopts_set(h, f.data(), s.data(), w.data(), ids.data(), f.size()) == EMQX_OK);
    // rejected calls change nothing
    const uint32_t bad_f = EMQX_DELIVER_MAX_FILTER, one = 1, zero = 0;
    const uint8_t ok_w = 1, qos3 = 3, reserved = 0x40, has_id = EMQX_SUBOPT_HAS_SUBID;
    CHECK(emqx_subopts_set(h, &bad_f, &one, &ok_w, nullptr, 1) == EMQX_EINVAL);
    CHECK(emqx_subopts_set(h, &one, &one, &qos3, nullptr, 1) == EMQX_EINVAL);
    CHECK(emqx_subopts_set(h, &one, &one, &reserved, nullptr, 1) == EMQX_EINVAL);
    CHECK(emqx_subopts_set(h, &one, &one, &has_id, &zero, 1) == EMQX_EINVAL);
    CHECK(emqx_subopts_set(h, &one, &one, &has_id, nullptr, 1) == EMQX_EINVAL);
    CHECK(emqx_subopts_commit(h) == EMQX_OK);
    emqx_subopts_stats st{};
    st.size = sizeof(st);
    CHECK(emqx_subopts_stats_get(h, &st) == EMQX_OK);
    CHECK(st.n_entries == N_ENTRIES && st.n_slots == (N_ENTRIES * 100ull + pct - 1) / pct && st.epoch == 1);
    CHECK(st.max_probe >= 1 && st.max_probe < st.n_slots && st.table_bytes == st.n_slots * 16);
    std::printf("load %d%%: %llu slots, longest probe run %llu\n", pct, static_cast<unsigned long long>(st.n_slots),
                static_cast<unsigned long long>(st.max_probe));

    Csr empty;  // n = 0
    run(h, t, empty, true);
    Csr big;  // empty messages around one 10 000-delivery message
    for (uint32_t c : {0u, 0u, 1u, 10000u, 0u, 3u, 0u}) big.message(r, c, N_FILTERS, N_SUBS);
    run(h, t, big, true);
    run(h, t, big, false);
    Csr many;
    for (int i = 0; i < 3000; ++i) many.message(r, r.below(4) == 0 ? 0 : r.below(40), N_FILTERS, N_SUBS);
    run(h, t, many, true);

    // remove and drop_subscribers act at the next commit
    std::vector<uint32_t> rf, rs, gone = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
    for (auto it = t.begin(); it != t.end();) {
      const bool drop = it->first.second < 10;
      const bool rem = !drop && (it->first.first % 7 == 0);
      if (rem) {
        rf.push_back(it->first.first);
        rs.push_back(it->first.second);
      }
      it = (drop || rem) ? t.erase(it) : std::next(it);
    }
    rf.push_back(N_FILTERS + 5);  // an absent pair is ignored
    rs.push_back(3);
    CHECK(emqx_subopts_remove(h, rf.data(), rs.data(), rf.size()) == EMQX_OK);
    CHECK(emqx_subopts_drop_subscribers(h, gone.data(), gone.size()) == EMQX_OK);
    CHECK(emqx_subopts_commit(h) == EMQX_OK);
    CHECK(emqx_subopts_stats_get(h, &st) == EMQX_OK && st.n_entries == t.size() && st.epoch == 2);
    run(h, t, many, true);

    // refused inputs
    emqx_deliver_batch b{};
    const uint64_t dec[3] = {0, 2, 1};
    const uint32_t two[2] = {1, 2};
    const uint8_t q[2] = {0, 0};
    uint8_t o[2];
    b.offsets = dec;
    b.subs = two;
    b.filters = two;
    b.n = 2;
    b.cap_in = 2;
    b.msg_qos = q;
    b.msg_flags = q;
    b.out_opts = o;
    CHECK(emqx_deliver_enrich_host(h, &b, nullptr, nullptr) == EMQX_EINVAL);
    CHECK(emqx_deliver_enrich_batch(h, &b, nullptr, nullptr) == EMQX_EDEVICE);
    CHECK(emqx_deliver_enrich_batch_device(h, &b, nullptr, nullptr, nullptr) == EMQX_EDEVICE);
    uint64_t sum[8];
    CHECK(emqx_deliver_enrich_batch_device_async(h, &b, sum, nullptr) == EMQX_EDEVICE);
    CHECK(emqx_subopts_destroy(h) == EMQX_OK);
  }
  std::printf("deliver host ok\n");
  return 0;
}
