// Host-only build of the authorization table (emqx_amd/csrc/authz.cpp with EMQX_AUTHZ_NO_DEVICE)
// under AddressSanitizer / UBSan: a table with keyed lists, the quirk cases of
// include/emqx_authz.h's semantics, and a few thousand generated requests — 65535-byte topics
// and principals among them — against a word-list matcher written here from
// emqx_topic:match/2 (apps/emqx/src/emqx_topic.erl:74-87).  Prints "authz host ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/emqx_authz.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

struct Packed {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> offs{0};
  uint32_t add(const std::string& s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    offs.push_back(bytes.size());
    return static_cast<uint32_t>(offs.size() - 2);
  }
  const uint8_t* data() const { return bytes.empty() ? reinterpret_cast<const uint8_t*>("") : bytes.data(); }
  uint64_t n() const { return offs.size() - 1; }
};

// A list of single-filter rules with who = all, the shape of the built-in database's rules.
struct SimpleRule {
  uint8_t permission, action;
  std::string filter;
  uint32_t tag;
};

int set_simple(emqx_authz* a, uint32_t source, uint32_t scope, const std::string& key, const std::vector<SimpleRule>& rs,
               char* err = nullptr, uint64_t cap = 0) {
  Packed s;
  std::vector<emqx_authz_rule> rules;
  for (auto& r : rs) {
    emqx_authz_rule x{};
    x.permission = r.permission;
    x.action = r.action;
    x.who_op = EMQX_AUTHZ_WHO_ALL;
    x.first_topic = s.add(r.filter);
    x.n_topics = 1;
    x.tag = r.tag;
    rules.push_back(x);
  }
  return emqx_authz_list_set(a, source, scope, reinterpret_cast<const uint8_t*>(key.data()), key.size(), rules.data(),
                             rules.size(), nullptr, 0, s.data(), s.offs.data(), s.n(), err, cap);
}

struct Client {
  std::string clientid, username;
  uint8_t present;
  uint32_t ipv4;
};

void set_clients(emqx_authz* a, const std::vector<Client>& cs) {
  Packed c, u;
  std::vector<uint32_t> ids, ip;
  std::vector<uint8_t> present;
  for (size_t i = 0; i < cs.size(); ++i) {
    ids.push_back(static_cast<uint32_t>(i));
    c.add(cs[i].clientid);
    u.add(cs[i].username);
    ip.push_back(cs[i].ipv4);
    present.push_back(cs[i].present);
  }
  CHECK(emqx_authz_clients_set(a, ids.data(), ids.size(), c.data(), c.offs.data(), u.data(), u.offs.data(), ip.data(),
                               present.data(), nullptr) == EMQX_OK);
}

struct Answer {
  uint8_t verdict;
  uint32_t tag;
};

Answer ask(emqx_authz* a, uint32_t client, uint8_t action, const std::string& topic) {
  Packed t;
  t.add(topic);
  uint8_t v = 99;
  uint32_t tag = 0;
  CHECK(emqx_authz_check_host(a, &client, &action, t.data(), t.offs.data(), 1, &v, &tag) == EMQX_OK);
  return {v, tag};
}

// ---- the matcher of this file: words as strings plus an atom flag -----------------------------
struct Word {
  std::string s;
  bool atom;  // '', '+', '#'
  bool operator==(const Word& o) const { return atom == o.atom && s == o.s; }
};

std::vector<Word> words(const std::string& t) {
  std::vector<Word> out;
  size_t s = 0;
  for (;;) {
    const size_t e = t.find('/', s);
    const std::string w = t.substr(s, e == std::string::npos ? std::string::npos : e - s);
    out.push_back({w, w.empty() || w == "+" || w == "#"});
    if (e == std::string::npos) return out;
    s = e + 1;
  }
}

bool match(const std::vector<Word>& n, size_t i, const std::vector<Word>& f, size_t j) {
  const bool ne = i == n.size(), fe = j == f.size();
  if (ne && fe) return true;
  if (!ne && !fe && n[i] == f[j]) return match(n, i + 1, f, j + 1);
  if (!ne && !fe && f[j].atom && f[j].s == "+") return match(n, i + 1, f, j + 1);
  return j + 1 == f.size() && f[j].atom && f[j].s == "#";
}

bool filter_matches(const std::string& topic, std::string filter, const Client& c) {
  if (filter.compare(0, 3, "eq ") == 0) return topic == filter.substr(3);
  std::vector<Word> f = words(filter);
  for (auto& w : f) {  // feed_var/3
    if (w.s == "${clientid}" && (c.present & EMQX_AUTHZ_HAS_CLIENTID)) w = {c.clientid, false};
    else if (w.s == "${username}" && (c.present & EMQX_AUTHZ_HAS_USERNAME)) w = {c.username, false};
  }
  return match(words(topic), 0, f, 0);
}

Answer expect(const std::vector<const std::vector<SimpleRule>*>& lists, const Client& c, uint8_t action,
              const std::string& topic) {
  for (auto* l : lists)
    for (auto& r : *l)
      if ((r.action & action) && filter_matches(topic, r.filter, c)) return {r.permission, r.tag};
  return {EMQX_AUTHZ_NOMATCH, EMQX_AUTHZ_TAG_NONE};
}

}  // namespace

int main() {
  emqx_authz* a = nullptr;
  CHECK(emqx_authz_create(0, &a) == EMQX_EDEVICE);  // this build has no device
  CHECK(emqx_authz_create(EMQX_AUTHZ_HOST_ONLY, &a) == EMQX_OK);

  const uint8_t ALLOW = EMQX_AUTHZ_ALLOW, DENY = EMQX_AUTHZ_DENY, PUB = EMQX_AUTHZ_PUBLISH, SUB = EMQX_AUTHZ_SUBSCRIBE,
                ALL = EMQX_AUTHZ_ALL;
  const std::string big(65535, 'x');
  std::vector<Client> clients = {
      {"c1", "u1", 7, (10u << 24) | 1},  {"a/b", "+", 3, 0}, {"#", "", 3, 0}, {"", "", 0, 0},
      {big, big, 3, 0},                  {"c1", "other", 3, 0},
  };
  // source 0: keyed lists for c1 / u1 and an all list; source 1: an all list
  const std::vector<SimpleRule> by_c1 = {{DENY, PUB, "t/c", 100}, {ALLOW, ALL, "x/${clientid}", 101}};
  const std::vector<SimpleRule> by_u1 = {{ALLOW, ALL, "t/c", 200}, {ALLOW, ALL, "t/u", 201}, {DENY, SUB, "y/${username}", 202}};
  const std::vector<SimpleRule> all0 = {
      {ALLOW, ALL, "eq #", 1},       {ALLOW, ALL, "eq lit/${username}", 2}, {DENY, PUB, "+/x", 3},
      {ALLOW, SUB, "s/+", 4},        {ALLOW, ALL, "a/#", 5},                {DENY, ALL, "a${clientid}", 6},
      {ALLOW, ALL, "x/${clientid}", 7}, {ALLOW, ALL, "y/${username}", 8},    {ALLOW, ALL, "e//l", 9},
      {ALLOW, ALL, "", 10},          {ALLOW, ALL, "p/" + big.substr(0, 65533), 11}, {DENY, ALL, "eq " + big, 12},
  };
  const std::vector<SimpleRule> all1 = {{DENY, ALL, "#", 300}};
  CHECK(set_simple(a, 0, EMQX_AUTHZ_SCOPE_CLIENTID, "c1", by_c1) == EMQX_OK);
  CHECK(set_simple(a, 0, EMQX_AUTHZ_SCOPE_USERNAME, "u1", by_u1) == EMQX_OK);
  CHECK(set_simple(a, 0, EMQX_AUTHZ_SCOPE_ALL, "", all0) == EMQX_OK);
  CHECK(set_simple(a, 1, EMQX_AUTHZ_SCOPE_ALL, "", all1) == EMQX_OK);
  set_clients(a, clients);
  CHECK(emqx_authz_commit(a) == EMQX_OK);

  auto is = [&](uint32_t c, uint8_t act, const std::string& t, uint8_t v, uint32_t tag) {
    const Answer r = ask(a, c, act, t);
    if (r.verdict != v || r.tag != tag) {
      std::fprintf(stderr, "client %u action %u topic %.40s: got %u/%u, want %u/%u\n", c, act, t.c_str(), r.verdict,
                   r.tag, v, tag);
      std::exit(1);
    }
  };
  is(0, PUB, "$SYS/x", DENY, 3);                   // Q1: '+' matches a '$' level
  is(3, SUB, "$SYS/y", DENY, 300);                 // Q1: '#' too
  is(0, SUB, "#", ALLOW, 1);                       // Q2
  is(0, PUB, "lit/${username}", ALLOW, 2);         // Q2: no substitution in eq
  is(0, PUB, "lit/u1", DENY, 300);
  is(1, PUB, "x/a/b", DENY, 300);                  // Q3: the value is one word
  is(1, SUB, "y/+", DENY, 300);                    // Q3: the value '+' is no wildcard, nor equals the level '+'
  is(2, SUB, "x/#", DENY, 300);
  is(2, PUB, "y/", DENY, 300);                     // Q3: the value <<>> is not the level ''
  is(3, PUB, "x/${clientid}", ALLOW, 7);           // Q4
  is(0, PUB, "ac1", DENY, 300);                    // Q5
  is(0, PUB, "a${clientid}", DENY, 6);
  is(0, SUB, "s/#", ALLOW, 4);                     // Q6: '+' matches the level '#'
  is(0, SUB, "a", ALLOW, 5);                       // Q6: 'a/#' matches 'a'
  is(0, SUB, "#/q", EMQX_AUTHZ_NOMATCH, EMQX_AUTHZ_TAG_NONE);  // Q6: the equal-heads clause comes before ['#']
  is(0, PUB, "e//l", ALLOW, 9);                    // Q7
  is(0, PUB, "", ALLOW, 10);                       // Q7: the empty topic is one empty level
  is(0, PUB, "t/c", DENY, 100);                    // clientid list before username list
  is(5, PUB, "t/c", DENY, 100);
  is(0, PUB, "t/u", ALLOW, 201);
  is(5, PUB, "t/u", DENY, 300);
  is(0, SUB, "y/u1", DENY, 202);                   // keyed list before the all list
  is(4, PUB, "x/" + big, ALLOW, 7);                // 65535-byte principal, 65537-byte topic
  is(4, PUB, big, DENY, 12);                       // 65535-byte eq filter
  is(4, PUB, "p/" + big.substr(0, 65533), ALLOW, 11);
  is(9, PUB, "t", EMQX_AUTHZ_BAD_REQUEST, EMQX_AUTHZ_TAG_NONE);
  is(0, 3, "t", EMQX_AUTHZ_BAD_REQUEST, EMQX_AUTHZ_TAG_NONE);

  // rejected inputs store nothing
  char err[128];
  CHECK(set_simple(a, 0, EMQX_AUTHZ_SCOPE_ALL, "", {{ALLOW, ALL, "#", 0}, {ALLOW, ALL, big + "y", 1}}, err, sizeof err) ==
        EMQX_EINVAL);
  CHECK(err[0] != 0);
  CHECK(set_simple(a, 8, EMQX_AUTHZ_SCOPE_ALL, "", {{ALLOW, ALL, "#", 0}}, err, 4) == EMQX_EINVAL);  // a short buffer
  CHECK(err[3] == 0);
  {
    Packed s;
    s.add("#");
    s.add("fe80::/10");
    emqx_authz_rule r{};
    r.permission = ALLOW, r.action = ALL, r.who_op = EMQX_AUTHZ_WHO_ONE, r.n_who = 1, r.n_topics = 1;
    emqx_authz_who w{EMQX_AUTHZ_WHO_CIDR, 1, 1};
    CHECK(emqx_authz_list_set(a, 0, 0, nullptr, 0, &r, 1, &w, 1, s.data(), s.offs.data(), 2, err, sizeof err) == EMQX_EINVAL);
    w.count = 5;  // runs past the strings
    CHECK(emqx_authz_list_set(a, 0, 0, nullptr, 0, &r, 1, &w, 1, s.data(), s.offs.data(), 2, err, sizeof err) == EMQX_EINVAL);
  }
  CHECK(emqx_authz_commit(a) == EMQX_OK);
  is(0, PUB, "zzz", DENY, 300);  // the all list of source 0 is still the old one (a '#' allow would answer)

  // generated requests, one batch
  std::mt19937 rng(7);
  const char* vocab[] = {"a", "x", "s", "t", "c", "u", "", "$SYS", "+", "#", "c1", "u1", "lit", "${clientid}", "${username}", "e", "l", "y"};
  Packed topics;
  std::vector<uint32_t> cl;
  std::vector<uint8_t> act;
  std::vector<std::string> ts;
  for (int i = 0; i < 4000; ++i) {
    std::string t;
    const int levels = 1 + rng() % 4;
    for (int k = 0; k < levels; ++k) t += (k ? "/" : "") + std::string(vocab[rng() % 18]);
    if (i % 500 == 0) t = "x/" + big;
    if (i % 500 == 1) t = big;
    ts.push_back(t);
    topics.add(t);
    cl.push_back(rng() % clients.size());
    act.push_back(1 + rng() % 2);
  }
  std::vector<uint8_t> v(ts.size());
  std::vector<uint32_t> tag(ts.size());
  CHECK(emqx_authz_check_host(a, cl.data(), act.data(), topics.data(), topics.offs.data(), ts.size(), v.data(),
                              tag.data()) == EMQX_OK);
  for (size_t i = 0; i < ts.size(); ++i) {
    const Client& c = clients[cl[i]];
    std::vector<const std::vector<SimpleRule>*> lists;
    if ((c.present & 1) && c.clientid == "c1") lists.push_back(&by_c1);
    if ((c.present & 2) && c.username == "u1") lists.push_back(&by_u1);
    lists.push_back(&all0);
    lists.push_back(&all1);
    const Answer e = expect(lists, c, act[i], ts[i]);
    if (v[i] != e.verdict || tag[i] != e.tag) {
      std::fprintf(stderr, "request %zu client %u action %u topic %.60s: got %u/%u, want %u/%u\n", i, cl[i], act[i],
                   ts[i].c_str(), v[i], tag[i], e.verdict, e.tag);
      return 1;
    }
  }
  // decreasing offsets, and the batch entry points of a handle without a device
  uint64_t bad_offs[3] = {0, 2, 1};
  CHECK(emqx_authz_check_host(a, cl.data(), act.data(), topics.data(), bad_offs, 2, v.data(), tag.data()) == EMQX_EINVAL);
  CHECK(emqx_authz_check_batch(a, cl.data(), act.data(), topics.data(), topics.offs.data(), 1, v.data(), tag.data()) ==
        EMQX_EDEVICE);
  emqx_authz_stats st{};
  st.size = sizeof st;
  CHECK(emqx_authz_stats_get(a, &st) == EMQX_OK);
  CHECK(st.n_rules == by_c1.size() + by_u1.size() + all0.size() + all1.size() && st.n_clients == clients.size());
  const uint32_t drop[2] = {0, 77};
  CHECK(emqx_authz_clients_drop(a, drop, 2) == EMQX_OK);
  CHECK(emqx_authz_source_clear(a, 0) == EMQX_OK);
  CHECK(emqx_authz_commit(a) == EMQX_OK);
  is(0, PUB, "t", EMQX_AUTHZ_BAD_REQUEST, EMQX_AUTHZ_TAG_NONE);
  is(1, PUB, "a/b", DENY, 300);
  CHECK(emqx_authz_destroy(a) == EMQX_OK);
  std::puts("authz host ok");
  return 0;
}
