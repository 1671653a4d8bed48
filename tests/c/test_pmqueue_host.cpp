// The host side of the priority mqueue stage (emqx_amd/csrc/pmqueue.cpp with EMQX_PMQUEUE_NO_DEVICE)
// against a fold of its own: one std::deque per class, the list of classes as a std::vector in list
// order, a message at a time, as emqx_mqueue:in/2 and out/1 do it: a seeded fuzz at C 4, Qc 8, then the
// worlds of the cases q128_full_bytes and q128_above_max of tests/pmqueue_cases.py (C 8 and 3, Qc 128:
// lengths of 128 and heads of 127, the top of the byte fields the state is packed into).  Built and run by
// tests/test_pmqueue_host_san.py, plainly and under AddressSanitizer and UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "../../include/emqx_pmqueue.h"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

namespace {

constexpr uint32_t MAXC = EMQX_PMQ_MAX_CLASSES;

struct Msg {
  uint32_t ref;
  uint8_t opts;
  int64_t born;  // the delivery position in the put that brought it, -1: an old one
};

struct Model {
  std::vector<uint32_t> order;  // class indices in list order
  std::deque<Msg> q[MAXC];
  int64_t credit = 0;
  bool last = false;
  uint64_t dropped = 0;
  uint32_t len() const {
    uint32_t n = 0;
    for (auto& d : q) n += static_cast<uint32_t>(d.size());
    return n;
  }
};

// The key of a class in Erlang term order: -P, and the atom `infinity` above every number.
double key_of(const emqx_pmqueue_table& t, uint32_t c) { return t.prio[c] == EMQX_PMQ_PRIO_INFINITY ? 1e18 : -static_cast<double>(t.prio[c]); }

void pq_in(Model& m, const emqx_pmqueue_table& t, uint32_t c, Msg x) {
  const bool present = std::find(m.order.begin(), m.order.end(), c) != m.order.end();
  m.q[c].push_back(x);
  if (present) return;
  if (t.prio[c] == EMQX_PMQ_PRIO_INFINITY) {
    m.order.insert(m.order.begin(), c);
    return;
  }
  auto by_key = [&](uint32_t a, uint32_t b) { return key_of(t, a) < key_of(t, b); };
  if (!m.order.empty() && t.prio[m.order[0]] == EMQX_PMQ_PRIO_INFINITY) {
    m.order.insert(m.order.begin() + 1, c);
    std::stable_sort(m.order.begin() + 1, m.order.end(), by_key);
  } else {
    m.order.insert(m.order.begin(), c);
    std::stable_sort(m.order.begin(), m.order.end(), by_key);
  }
}

// emqx_mqueue:in/2: the dropped message's `born` through *gone (-2: none).
void mq_in(Model& m, const emqx_pmqueue_table& t, uint32_t c, Msg x, Msg* gone, bool* dropped) {
  *dropped = false;
  if (m.q[c].size() == t.max_len) {
    *gone = m.q[c].front();
    *dropped = true;
    m.q[c].pop_front();
    if (m.q[c].empty()) m.order.erase(std::find(m.order.begin(), m.order.end(), c));
    m.dropped += 1;
  }
  pq_in(m, t, c, x);
}

bool mq_out(Model& m, const emqx_pmqueue_table& t, Msg* x, uint32_t* cls) {
  for (;;) {
    if (m.len() == 0) return false;
    if (m.last && m.credit == 0) {
      std::rotate(m.order.begin(), m.order.begin() + 1, m.order.end());
      m.last = false;
      continue;
    }
    const uint32_t c = m.order[0];
    if (!m.last) {
      m.last = true;
      const int64_t p = t.prio[c] == EMQX_PMQ_PRIO_INFINITY ? 1000000 : t.prio[c];
      m.credit = (p + t.base + 1) * static_cast<int64_t>(t.mult) - 1;
    } else {
      m.credit -= 1;
    }
    *x = m.q[c].front();
    *cls = c;
    m.q[c].pop_front();
    if (m.q[c].empty()) m.order.erase(m.order.begin());
    return true;
  }
}

struct World {
  uint32_t n, c, qc;
  std::vector<emqx_pmqueue_table> tables;
  std::vector<emqx_window_session> sessions;
  std::vector<emqx_mqueue_entry> ring;
  emqx_pmqueue_head* heads;
  void* heads_raw;
  std::vector<Model> models;
  World(uint32_t n_, uint32_t c_, uint32_t qc_) : n(n_), c(c_), qc(qc_) {
    sessions.assign(n, emqx_window_session{});
    ring.assign(static_cast<size_t>(n) * c * qc, emqx_mqueue_entry{0, 0, {0, 0, 0}});
    CHECK(posix_memalign(&heads_raw, 64, n * sizeof(emqx_pmqueue_head)) == 0);
    heads = static_cast<emqx_pmqueue_head*>(heads_raw);
    std::memset(heads, 0, n * sizeof(emqx_pmqueue_head));
    models.resize(n);
    for (uint32_t s = 0; s < n; ++s) {
      sessions[s].flags = EMQX_WINDOW_PRESENT | EMQX_WINDOW_CONNECTED;
      sessions[s].next_pkt_id = 1;
      heads[s].order = 0xFFFFFFFFu;
    }
  }
  ~World() { std::free(heads_raw); }
  World(const World&) = delete;
  World& operator=(const World&) = delete;
  const emqx_pmqueue_table& table_of(uint32_t s) const { return tables[heads[s].table]; }
  // `len` entries of class k of session s from ring position `head`, oldest first; the order list ascends
  void fill(uint32_t s, uint32_t k, uint32_t head, uint32_t len, uint32_t first_ref) {
    for (uint32_t i = 0; i < len; ++i) {
      const uint32_t pos = (head + i) % qc;
      const Msg x{first_ref + i, static_cast<uint8_t>(pos % 3), -1};
      ring[(static_cast<size_t>(s) * c + k) * qc + pos] = emqx_mqueue_entry{x.ref, x.opts, {0, 0, 0}};
      models[s].q[k].push_back(x);
    }
    heads[s].head[k] = static_cast<uint16_t>(head);
    heads[s].len[k] = static_cast<uint16_t>(len);
    if (len) {
      models[s].order.push_back(k);
      uint32_t word = 0xFFFFFFFFu;
      for (size_t p = 0; p < models[s].order.size(); ++p) word = (word & ~(0xFu << (4 * p))) | (models[s].order[p] << (4 * p));
      heads[s].order = word;
    }
    sessions[s].mq_len += len;
  }
};

void check_state(const World& w) {
  for (uint32_t s = 0; s < w.n; ++s) {
    const Model& m = w.models[s];
    const emqx_pmqueue_head& h = w.heads[s];
    for (uint32_t c = 0; c < MAXC; ++c) {
      CHECK(h.len[c] == m.q[c].size() && h.head[c] < w.qc);
      for (uint32_t i = 0; i < h.len[c]; ++i) {
        const emqx_mqueue_entry& e = w.ring[(static_cast<size_t>(s) * w.c + c) * w.qc + (h.head[c] + i) % w.qc];
        CHECK(e.ref == m.q[c][i].ref && e.opts == m.q[c][i].opts);
      }
    }
    for (uint32_t p = 0; p < 8; ++p) {
      const uint32_t nib = (h.order >> (4 * p)) & 0xF;
      CHECK(nib == (p < m.order.size() ? m.order[p] : 0xFu));
    }
    CHECK(h.flags == (m.last ? 1u : 0u));
    CHECK(h.credit == (m.credit < 0 ? -1 : m.credit));
    CHECK(w.sessions[s].mq_len == m.len() && w.sessions[s].dropped == m.dropped);
  }
}

struct Inboxes {
  std::vector<uint32_t> subs;
  std::vector<uint64_t> off{0};
  std::vector<uint8_t> opts, ver, cls;  // cls: the class byte of a delivery's message, the same for every table
  std::vector<uint32_t> refs;
};

// One put call against in/2 played a delivery at a time; returns the evictions.
uint64_t put_and_check(emqx_pmqueue* h, World& w, const Inboxes& in, uint64_t want_flags) {
  const uint64_t total = in.opts.size(), n_tables = w.tables.size();
  std::vector<uint32_t> src(total);
  std::vector<uint8_t> cls_bytes;
  for (uint64_t d = 0; d < total; ++d) {
    src[d] = static_cast<uint32_t>(d);
    for (uint64_t t = 0; t < n_tables; ++t) cls_bytes.push_back(in.cls[d]);
  }
  std::vector<uint8_t> o_ver(total + 1), o_cls(total + 1);
  std::vector<emqx_mqueue_entry> o_ev(total + 1);
  std::vector<uint32_t> o_cnt(8 * in.subs.size());
  emqx_pmqueue_put_args pa{};
  pa.inbox_subs = in.subs.data();
  pa.inbox_offsets = in.off.data();
  pa.box_opts = in.opts.data();
  pa.m = in.subs.size();
  pa.cap_in = total;
  pa.cap_boxes = in.subs.size();
  pa.verdicts = in.ver.data();
  pa.refs = in.refs.data();
  pa.box_src = src.data();
  pa.msg_class = cls_bytes.data();
  pa.n_msgs = total;
  pa.tables = w.tables.data();
  pa.n_tables = n_tables;
  pa.sessions = w.sessions.data();
  pa.sub_limit = w.n;
  pa.update_table = 1;
  pa.ring = w.ring.data();
  pa.heads = w.heads;
  pa.c = w.c;
  pa.qc = w.qc;
  pa.out_verdicts = o_ver.data();
  pa.out_class = o_cls.data();
  pa.out_evicted = o_ev.data();
  pa.out_counts = o_cnt.data();
  uint64_t sum[8];
  CHECK(emqx_pmqueue_put_host(h, &pa, sum) == EMQX_OK);
  CHECK(sum[0] == want_flags && sum[1] == total && sum[2] == in.subs.size() && sum[7] == in.subs.size());
  std::vector<uint8_t> want_ver(total, 0);
  uint64_t evictions = 0, unstored = 0;
  for (size_t k = 0; k < in.subs.size(); ++k) {
    Model& m = w.models[in.subs[k]];
    const emqx_pmqueue_table& t = w.table_of(in.subs[k]);
    for (auto& d : m.q)
      for (auto& x : d) x.born = -1;
    for (uint64_t d = in.off[k]; d < in.off[k + 1]; ++d) {
      if (in.ver[d] != EMQX_W_QUEUED) {
        CHECK(o_cls[d] == EMQX_PMQ_NO_CLASS && o_ev[d].ref == EMQX_MQ_NO_REF);
        continue;
      }
      const uint8_t b = in.cls[d];
      const uint32_t c = b < t.n_classes ? b : t.default_class;
      CHECK(o_cls[d] == c);
      want_ver[d] = EMQX_W_QUEUED;
      if (m.q[c].size() >= w.qc && m.q[c].size() != t.max_len) {  // a full ring above max_len: the stage's own limit
        CHECK(o_ev[d].ref == EMQX_MQ_NO_REF);
        ++unstored;
        continue;
      }
      Msg gone{};
      bool dropped;
      mq_in(m, t, c, Msg{in.refs[d], in.opts[d], static_cast<int64_t>(d)}, &gone, &dropped);
      if (dropped) {
        want_ver[d] |= EMQX_W_EVICTS;
        ++evictions;
        if (gone.born < 0) {
          CHECK(o_ev[d].ref == gone.ref && o_ev[d].opts == gone.opts);
        } else {
          want_ver[gone.born] = static_cast<uint8_t>(EMQX_W_QUEUED_DROPPED | (want_ver[gone.born] & EMQX_W_EVICTS));
          CHECK(o_ev[d].ref == EMQX_MQ_NO_REF);
        }
      } else {
        CHECK(o_ev[d].ref == EMQX_MQ_NO_REF);
      }
    }
  }
  for (uint64_t d = 0; d < total; ++d) CHECK(o_ver[d] == want_ver[d]);
  CHECK(sum[6] == unstored && sum[4] + sum[5] == evictions);
  check_state(w);
  return evictions;
}

// One take call (every window open at entry) against out/1 played an item at a time; returns the items.
uint64_t take_and_check(emqx_pmqueue* h, World& w, const std::vector<uint32_t>* tk) {
  for (auto& s : w.sessions) s.inflight = 0;
  const uint64_t mt = tk ? tk->size() : w.n;
  const uint64_t cap = mt * w.c * w.qc;
  std::vector<uint64_t> t_off(mt + 1);
  std::vector<uint8_t> t_opts(cap), t_ver(cap), t_cls(cap), t_status(mt);
  std::vector<uint16_t> t_ids(cap);
  std::vector<uint32_t> t_refs(cap), t_cnt(4 * mt);
  emqx_pmqueue_take_args ta{};
  ta.subs = tk ? tk->data() : nullptr;
  ta.m = mt;
  ta.cap_boxes = mt;
  ta.sessions = w.sessions.data();
  ta.sub_limit = w.n;
  ta.update_table = 1;
  ta.tables = w.tables.data();
  ta.n_tables = w.tables.size();
  ta.ring = w.ring.data();
  ta.heads = w.heads;
  ta.c = w.c;
  ta.qc = w.qc;
  ta.cap_out = cap;
  ta.out_offsets = t_off.data();
  ta.out_opts = t_opts.data();
  ta.out_verdicts = t_ver.data();
  ta.out_pkt_ids = t_ids.data();
  ta.out_refs = t_refs.data();
  ta.out_class = t_cls.data();
  ta.out_status = t_status.data();
  ta.out_counts = t_cnt.data();
  uint64_t sum[8];
  CHECK(emqx_pmqueue_take_host(h, &ta, sum) == EMQX_OK);
  uint64_t at = 0;
  for (uint64_t k = 0; k < mt; ++k) {
    const uint32_t s = tk ? (*tk)[k] : static_cast<uint32_t>(k);
    Model& m = w.models[s];
    const emqx_window_session& rec = w.sessions[s];
    CHECK(t_off[k] == at && t_status[k] == EMQX_A_OK);
    uint32_t n = rec.inflight_max ? rec.inflight_max : 1000;  // (inflight was 0 at entry; the call added its sends)
    while (n > 0) {
      Msg x{};
      uint32_t c;
      if (!mq_out(m, w.table_of(s), &x, &c)) break;
      CHECK(t_refs[at] == x.ref && t_opts[at] == x.opts && t_cls[at] == c);
      if ((x.opts & 3) == 0) {
        CHECK(t_ver[at] == EMQX_W_SEND_QOS0 && t_ids[at] == 0);
      } else {
        CHECK(t_ver[at] == EMQX_W_SEND && t_ids[at] >= 1);
        --n;
      }
      ++at;
    }
    CHECK(t_cnt[4 * k + 3] == m.len());
  }
  CHECK(t_off[mt] == at && sum[3] == at);
  check_state(w);
  return at;
}

emqx_pmqueue_table table_of(std::vector<int32_t> prios, uint32_t default_class, uint32_t max_len, uint32_t mult, uint32_t base) {
  emqx_pmqueue_table t{};
  t.n_classes = static_cast<uint32_t>(prios.size());
  for (size_t c = 0; c < prios.size(); ++c) t.prio[c] = prios[c];
  t.default_class = default_class;
  t.max_len = max_len;
  t.mult = mult;
  t.base = base;
  return t;
}

// q128_full_bytes: 8 rings of 128, every one full, heads up to 127; 1, 2 and 130 candidates a class evict across
// the ring end (130: the first two of this very inbox as well); then everything is handed out.
void q128_full_bytes(emqx_pmqueue* h, std::mt19937& rng) {
  const uint32_t heads[8] = {127, 0, 1, 64, 126, 63, 65, 2};
  World w(3, 8, 128);
  w.tables.push_back(table_of({EMQX_PMQ_PRIO_INFINITY, 7, 6, 5, 4, 3, 2, -1}, 6, 128, 1, 0));
  for (uint32_t s = 0; s < 3; ++s)
    for (uint32_t k = 0; k < 8; ++k) w.fill(s, k, heads[k], 128, 1024 * s + 128 * k);
  check_state(w);
  Inboxes in;
  in.subs = {2, 0, 1};
  for (uint32_t e : {1u, 2u, 130u}) {
    std::vector<uint8_t> box;
    for (uint8_t k = 0; k < 8; ++k) box.insert(box.end(), e, k);
    std::shuffle(box.begin(), box.end(), rng);
    for (uint8_t k : box) {
      in.cls.push_back(k);
      in.opts.push_back(static_cast<uint8_t>(in.opts.size() % 3));
      in.ver.push_back(EMQX_W_QUEUED);
      in.refs.push_back(5000 + static_cast<uint32_t>(in.refs.size()));
    }
    in.off.push_back(in.opts.size());
  }
  CHECK(put_and_check(h, w, in, 0) == 8 * 133);
  for (uint32_t s = 0; s < 3; ++s)
    for (uint32_t k = 0; k < 8; ++k) CHECK(w.heads[s].len[k] == 128 && w.heads[s].head[k] == (heads[k] + (s == 2 ? 1 : s == 0 ? 2 : 128)) % 128);
  CHECK(take_and_check(h, w, nullptr) == 3 * 1024 && w.sessions[1].mq_len == 0);  // (a third of the entries are QoS 0: under 1000 sends)
}

// q128_above_max: max_len 100 and rings that hold 101, 127 and 128: room for all, for one, for none.
void q128_above_max(emqx_pmqueue* h) {
  World w(2, 3, 128);
  w.tables.push_back(table_of({5, 2, 0}, 1, 100, 1, 0));
  w.fill(1, 0, 120, 101, 1000);
  w.fill(1, 1, 5, 127, 2000);
  w.fill(1, 2, 127, 128, 3000);
  Inboxes in;
  in.subs = {1};
  for (uint8_t k : {0, 1, 0, 2, 1, 0, 0, 2, 1, 0}) {
    in.cls.push_back(k);
    in.opts.push_back(1);
    in.ver.push_back(EMQX_W_QUEUED);
    in.refs.push_back(7000 + static_cast<uint32_t>(in.refs.size()));
  }
  in.off.push_back(10);
  CHECK(put_and_check(h, w, in, EMQX_PMQ_F_ROW_FULL) == 0);
  CHECK(w.heads[1].len[0] == 106 && w.heads[1].len[1] == 128 && w.heads[1].len[2] == 128 && w.sessions[1].mq_len == 362);
  CHECK(take_and_check(h, w, nullptr) == 362);
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  auto pick = [&](uint32_t n) { return static_cast<uint32_t>(rng() % n); };
  emqx_pmqueue* h = nullptr;
  CHECK(emqx_pmqueue_create(0, &h) == EMQX_EDEVICE && h == nullptr);
  CHECK(emqx_pmqueue_create(EMQX_PMQUEUE_HOST_ONLY, &h) == EMQX_OK && h);
  constexpr uint32_t N = 96;
  World w(N, 4, 8);
  const int32_t pool[5] = {EMQX_PMQ_PRIO_INFINITY, 5, 2, 0, -1};
  for (uint32_t t = 0; t < 7; ++t) {
    emqx_pmqueue_table tab{};
    uint32_t mask = 0;
    tab.n_classes = 2 + pick(3);
    while (static_cast<uint32_t>(__builtin_popcount(mask)) < tab.n_classes) mask |= 1u << pick(5);
    uint32_t at = 0;
    for (uint32_t i = 0; i < 5; ++i)
      if (mask & (1u << i)) tab.prio[at++] = pool[i];
    tab.default_class = pick(tab.n_classes);
    tab.max_len = 2 + pick(2);
    tab.mult = 1 + pick(2);
    w.tables.push_back(tab);
  }
  for (uint32_t s = 0; s < N; ++s) {
    w.sessions[s].inflight_max = 1 + pick(4);
    w.sessions[s].next_pkt_id = 65530 + pick(5);
    w.heads[s].table = s % 7;
  }
  uint32_t next_ref = 0;
  uint64_t evictions = 0, items_total = 0;
  for (uint32_t round = 0; round < 60; ++round) {
    // a put: every second session gets an inbox of 0..7 deliveries
    Inboxes in;
    for (uint32_t s = round % 2; s < N; s += 2) {
      in.subs.push_back(s);
      const uint32_t k = pick(8);
      for (uint32_t i = 0; i < k; ++i) {
        in.opts.push_back(static_cast<uint8_t>(pick(3)));
        in.ver.push_back(pick(5) ? EMQX_W_QUEUED : EMQX_W_SEND);
        in.refs.push_back(next_ref++);
        in.cls.push_back(static_cast<uint8_t>(pick(6) == 5 ? 0xFF : pick(5)));
      }
      in.off.push_back(in.opts.size());
    }
    evictions += put_and_check(h, w, in, 0);
    // the acks reopen the windows; a take of a third of the sessions, every third round of all (subs NULL)
    std::vector<uint32_t> tk;
    for (uint32_t s = round % 3; s < N; s += 3) tk.push_back(s);
    items_total += take_and_check(h, w, round % 3 == 2 ? nullptr : &tk);
  }
  CHECK(evictions > 300 && items_total > 1000);
  emqx_pmqueue_stats st{};
  st.size = sizeof(st);
  CHECK(emqx_pmqueue_stats_get(h, &st) == EMQX_OK && st.calls == 120 && st.group == 4);
  q128_full_bytes(h, rng);
  q128_above_max(h);
  CHECK(emqx_pmqueue_set_tuning(h, "group", 16) == EMQX_OK && emqx_pmqueue_set_tuning(h, "group", 3) == EMQX_EINVAL);
  CHECK(emqx_pmqueue_reserve(h, 1, 1) == EMQX_EDEVICE);
  CHECK(emqx_pmqueue_destroy(h) == EMQX_OK);
  std::printf("pmqueue host ok: %llu evictions, %llu items\n", static_cast<unsigned long long>(evictions),
              static_cast<unsigned long long>(items_total));
  return 0;
}
