// The host side of the priority mqueue stage (emqx_amd/csrc/pmqueue.cpp with EMQX_PMQUEUE_NO_DEVICE)
// against a fold of its own: one std::deque per class, the list of classes as a std::vector in list
// order, a message at a time, as emqx_mqueue:in/2 and out/1 do it.  Built and run by
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

constexpr uint32_t N = 96, C = 4, QC = 8;

struct Msg {
  uint32_t ref;
  uint8_t opts;
  int64_t born;  // the delivery position in the put that brought it, -1: an old one
};

struct Model {
  std::vector<uint32_t> order;  // class indices in list order
  std::deque<Msg> q[C];
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
  std::vector<emqx_pmqueue_table> tables;
  std::vector<emqx_window_session> sessions;
  std::vector<emqx_mqueue_entry> ring;
  emqx_pmqueue_head* heads;
  void* heads_raw;
  std::vector<Model> models;
};

void check_state(const World& w) {
  for (uint32_t s = 0; s < N; ++s) {
    const Model& m = w.models[s];
    const emqx_pmqueue_head& h = w.heads[s];
    for (uint32_t c = 0; c < C; ++c) {
      CHECK(h.len[c] == m.q[c].size() && h.head[c] < QC);
      for (uint32_t i = 0; i < h.len[c]; ++i) {
        const emqx_mqueue_entry& e = w.ring[(s * C + c) * QC + (h.head[c] + i) % QC];
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

}  // namespace

int main() {
  std::mt19937 rng(12345);
  auto pick = [&](uint32_t n) { return static_cast<uint32_t>(rng() % n); };
  emqx_pmqueue* h = nullptr;
  CHECK(emqx_pmqueue_create(0, &h) == EMQX_EDEVICE && h == nullptr);
  CHECK(emqx_pmqueue_create(EMQX_PMQUEUE_HOST_ONLY, &h) == EMQX_OK && h);
  World w;
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
  w.sessions.assign(N, emqx_window_session{});
  w.ring.assign(static_cast<size_t>(N) * C * QC, emqx_mqueue_entry{0, 0, {0, 0, 0}});
  CHECK(posix_memalign(&w.heads_raw, 64, N * sizeof(emqx_pmqueue_head)) == 0);
  w.heads = static_cast<emqx_pmqueue_head*>(w.heads_raw);
  std::memset(w.heads, 0, N * sizeof(emqx_pmqueue_head));
  w.models.resize(N);
  for (uint32_t s = 0; s < N; ++s) {
    w.sessions[s].flags = EMQX_WINDOW_PRESENT | EMQX_WINDOW_CONNECTED;
    w.sessions[s].inflight_max = 1 + pick(4);
    w.sessions[s].next_pkt_id = 65530 + pick(5);
    w.heads[s].order = 0xFFFFFFFFu;
    w.heads[s].table = s % 7;
  }
  uint32_t next_ref = 0;
  uint64_t evictions = 0, items_total = 0;
  for (uint32_t round = 0; round < 60; ++round) {
    // a put: every second session gets an inbox of 0..7 deliveries
    std::vector<uint32_t> subs;
    std::vector<uint64_t> off{0};
    std::vector<uint8_t> opts, ver, cls_bytes;
    std::vector<uint32_t> refs, src;
    for (uint32_t s = round % 2; s < N; s += 2) {
      subs.push_back(s);
      const uint32_t k = pick(8);
      for (uint32_t i = 0; i < k; ++i) {
        opts.push_back(static_cast<uint8_t>(pick(3)));
        ver.push_back(pick(5) ? EMQX_W_QUEUED : EMQX_W_SEND);
        refs.push_back(next_ref++);
        src.push_back(static_cast<uint32_t>(src.size()));
        const uint8_t b = static_cast<uint8_t>(pick(6) == 5 ? 0xFF : pick(5));
        for (uint32_t t = 0; t < 7; ++t) cls_bytes.push_back(b);
      }
      off.push_back(opts.size());
    }
    const uint64_t total = opts.size();
    std::vector<uint8_t> o_ver(total + 1), o_cls(total + 1);
    std::vector<emqx_mqueue_entry> o_ev(total + 1);
    std::vector<uint32_t> o_cnt(8 * subs.size());
    emqx_pmqueue_put_args pa{};
    pa.inbox_subs = subs.data();
    pa.inbox_offsets = off.data();
    pa.box_opts = opts.data();
    pa.m = subs.size();
    pa.cap_in = total;
    pa.cap_boxes = subs.size();
    pa.verdicts = ver.data();
    pa.refs = refs.data();
    pa.box_src = src.data();
    pa.msg_class = cls_bytes.data();
    pa.n_msgs = total;
    pa.tables = w.tables.data();
    pa.n_tables = 7;
    pa.sessions = w.sessions.data();
    pa.sub_limit = N;
    pa.update_table = 1;
    pa.ring = w.ring.data();
    pa.heads = w.heads;
    pa.c = C;
    pa.qc = QC;
    pa.out_verdicts = o_ver.data();
    pa.out_class = o_cls.data();
    pa.out_evicted = o_ev.data();
    pa.out_counts = o_cnt.data();
    uint64_t sum[8];
    CHECK(emqx_pmqueue_put_host(h, &pa, sum) == EMQX_OK);
    CHECK(sum[0] == 0 && sum[1] == total && sum[2] == subs.size() && sum[7] == subs.size());
    std::vector<uint8_t> want_ver(total, 0);
    for (size_t k = 0; k < subs.size(); ++k) {
      Model& m = w.models[subs[k]];
      const emqx_pmqueue_table& t = w.tables[subs[k] % 7];
      for (auto& d : m.q)
        for (auto& x : d) x.born = -1;
      for (uint64_t d = off[k]; d < off[k + 1]; ++d) {
        if (ver[d] != EMQX_W_QUEUED) {
          CHECK(o_cls[d] == EMQX_PMQ_NO_CLASS && o_ev[d].ref == EMQX_MQ_NO_REF);
          continue;
        }
        const uint8_t b = cls_bytes[d * 7];
        const uint32_t c = b < t.n_classes ? b : t.default_class;
        CHECK(o_cls[d] == c);
        Msg gone{};
        bool dropped;
        mq_in(m, t, c, Msg{refs[d], opts[d], static_cast<int64_t>(d)}, &gone, &dropped);
        want_ver[d] = EMQX_W_QUEUED;
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
    check_state(w);
    // the acks reopen the windows; a take of a third of the sessions, every third round of all (subs NULL)
    for (auto& s : w.sessions) s.inflight = 0;
    std::vector<uint32_t> tk;
    for (uint32_t s = round % 3; s < N; s += 3) tk.push_back(s);
    const bool sweep = round % 3 == 2;
    const uint64_t mt = sweep ? N : tk.size();
    const uint64_t cap = mt * C * QC;
    std::vector<uint64_t> t_off(mt + 1);
    std::vector<uint8_t> t_opts(cap), t_ver(cap), t_cls(cap), t_status(mt);
    std::vector<uint16_t> t_ids(cap);
    std::vector<uint32_t> t_refs(cap), t_cnt(4 * mt);
    emqx_pmqueue_take_args ta{};
    ta.subs = sweep ? nullptr : tk.data();
    ta.m = mt;
    ta.cap_boxes = mt;
    ta.sessions = w.sessions.data();
    ta.sub_limit = N;
    ta.update_table = 1;
    ta.tables = w.tables.data();
    ta.n_tables = 7;
    ta.ring = w.ring.data();
    ta.heads = w.heads;
    ta.c = C;
    ta.qc = QC;
    ta.cap_out = cap;
    ta.out_offsets = t_off.data();
    ta.out_opts = t_opts.data();
    ta.out_verdicts = t_ver.data();
    ta.out_pkt_ids = t_ids.data();
    ta.out_refs = t_refs.data();
    ta.out_class = t_cls.data();
    ta.out_status = t_status.data();
    ta.out_counts = t_cnt.data();
    CHECK(emqx_pmqueue_take_host(h, &ta, sum) == EMQX_OK);
    uint64_t at = 0;
    for (uint64_t k = 0; k < mt; ++k) {
      const uint32_t s = sweep ? static_cast<uint32_t>(k) : tk[k];
      Model& m = w.models[s];
      emqx_window_session& rec = w.sessions[s];
      CHECK(t_off[k] == at && t_status[k] == EMQX_A_OK);
      uint32_t n = rec.inflight_max;  // (inflight was 0 at entry; the call added its sends)
      while (n > 0) {
        Msg x{};
        uint32_t c;
        if (!mq_out(m, w.tables[s % 7], &x, &c)) break;
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
    items_total += at;
    check_state(w);
  }
  CHECK(evictions > 300 && items_total > 1000);
  emqx_pmqueue_stats st{};
  st.size = sizeof(st);
  CHECK(emqx_pmqueue_stats_get(h, &st) == EMQX_OK && st.calls == 120 && st.group == 4);
  CHECK(emqx_pmqueue_set_tuning(h, "group", 16) == EMQX_OK && emqx_pmqueue_set_tuning(h, "group", 3) == EMQX_EINVAL);
  CHECK(emqx_pmqueue_reserve(h, 1, 1) == EMQX_EDEVICE);
  CHECK(emqx_pmqueue_destroy(h) == EMQX_OK);
  std::free(w.heads_raw);
  std::printf("pmqueue host ok: %llu evictions, %llu items\n", static_cast<unsigned long long>(evictions),
              static_cast<unsigned long long>(items_total));
  return 0;
}
