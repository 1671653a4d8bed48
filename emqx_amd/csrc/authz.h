// Snapshot layout of the authorization table and the per-pair predicate, shared by the host
// evaluator (authz.cpp, emqx_authz_check_host) and the HIP kernels (authz_kernels.hip): both
// run the functions below over the same flat arrays.  Compiles with a plain C++ compiler.
//
// Reference: apps/emqx_authz/src/emqx_authz_rule.erl (line numbers below are that file's).
//   matches/4   :108-115   first rule that matches decides       -> az_check
//   match/4     :117-125   action, who, topics                   -> az_entry_hit
//   match_who/2 :132-165                                          -> az_who / az_leaf
//   match_topic/2 :177-180 eq: words equal; else emqx_topic:match on word LISTS
//                          (apps/emqx/src/emqx_topic.erl:74-87: no '$' rule)  -> az_match_filter
//   feed_var/3  :182-195   a placeholder level becomes the client's value as ONE literal word,
//                          or stays as written when the field is undefined
#pragma once

#include <stdint.h>

#include "layout.h"

namespace emqx {

enum : uint32_t { AZ_PLAIN = 0, AZ_EQ = 1, AZ_PATTERN = 2 };            // AzEntry.kind
enum : uint32_t { AZ_WHO_ALL = 0, AZ_WHO_ONE = 1, AZ_WHO_AND = 2, AZ_WHO_OR = 3 };
enum : uint32_t { AZ_LEAF_USERNAME = 1, AZ_LEAF_CLIENTID = 2, AZ_LEAF_CIDR = 3, AZ_LEAF_FLAG = 4 };
enum : uint32_t { AZ_HAS_CLIENTID = 1, AZ_HAS_USERNAME = 2, AZ_HAS_IPV4 = 4, AZ_REGISTERED = 0x80000000u };
enum : uint32_t { AZ_NOMATCH = 0, AZ_ALLOW = 1, AZ_DENY = 2, AZ_BAD = 3 };
constexpr uint32_t AZ_TAG_NONE = 0xFFFFFFFFu;
constexpr uint32_t AZ_MAX_SOURCES = 8;
constexpr uint32_t AZ_SEG_STRIDE = 3 * AZ_MAX_SOURCES;  // entry ranges per client at most

// One topic filter of one rule; entries of a list are in evaluation order (rule order, then
// the rule's filter order), lists are contiguous.
struct alignas(16) AzEntry {
  uint32_t off;   // filter bytes in the arena
  uint16_t len;
  uint8_t kind;   // AZ_PLAIN / AZ_EQ / AZ_PATTERN
  uint8_t pad0;
  uint32_t rule;  // index into rules
  uint32_t pad1;
};
static_assert(sizeof(AzEntry) == 16, "AzEntry must be 16 bytes");

struct alignas(16) AzRule {
  uint8_t permission;   // AZ_ALLOW / AZ_DENY
  uint8_t action_mask;  // bit 0 publish, bit 1 subscribe
  uint8_t who_op;       // AZ_WHO_*
  uint8_t pad;
  uint32_t who_begin;   // leaves [who_begin, who_begin + n_who)
  uint32_t n_who;
  uint32_t tag;
};
static_assert(sizeof(AzRule) == 16, "AzRule must be 16 bytes");

struct alignas(16) AzLeaf {
  uint32_t kind;  // AZ_LEAF_*
  uint32_t a;     // eq: arena offset | cidr: first range | flag: bit number
  uint32_t b;     // eq: length       | cidr: number of ranges (ipaddrs: any of them)
  uint32_t pad;
};
static_assert(sizeof(AzLeaf) == 16, "AzLeaf must be 16 bytes");

struct AzRange {
  uint32_t lo, hi;  // cidr: first and last address, host order | segment: entries [lo, hi)
};

struct alignas(16) AzClient {
  uint32_t cid_off, user_off;  // bytes in the client arena
  uint16_t cid_len, user_len;
  uint32_t present;            // AZ_HAS_* | AZ_REGISTERED (0: no such client)
  uint32_t ipv4;               // host order
  uint32_t n_seg;              // entry ranges of this client in segs[id * AZ_SEG_STRIDE ...]
  uint64_t flags;              // caller-evaluated who terms (regexes)
};
static_assert(sizeof(AzClient) == 32, "AzClient must be 32 bytes");

// Kernel-argument view of one committed snapshot (host or device pointers).
struct AzView {
  const AzEntry* entries;
  const AzRule* rules;
  const AzLeaf* leaves;
  const AzRange* cidrs;
  const uint8_t* arena;
  const AzClient* clients;
  const uint8_t* carena;
  const AzRange* segs;
  uint32_t n_clients;  // client ids < n_clients index `clients`
  uint32_t n_entries;
};

EMQX_HD bool az_bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// End of the level that starts at s: the next '/' or n.
EMQX_HD uint32_t az_level_end(const uint8_t* p, uint32_t s, uint32_t n) {
  while (s < n && p[s] != '/') ++s;
  return s;
}

// Is p[s, e) the level "${clientid}" (1) or "${username}" (2)?  0 otherwise.
EMQX_HD uint32_t az_placeholder(const uint8_t* p, uint32_t s, uint32_t e) {
  if (e - s != 11 || p[s] != '$' || p[s + 1] != '{' || p[e - 1] != '}') return 0;
  const char* c = "clientid";
  const char* u = "username";
  bool ic = true, iu = true;
  for (uint32_t i = 0; i < 8; ++i) {
    ic = ic && p[s + 2 + i] == static_cast<uint8_t>(c[i]);
    iu = iu && p[s + 2 + i] == static_cast<uint8_t>(u[i]);
  }
  return ic ? 1u : iu ? 2u : 0u;
}

// emqx_topic:match/2 on word lists (emqx_topic.erl:74-87) of topic t[0, tn) against filter
// f[0, fn), clause by clause.  words/1 maps the levels "", "+", "#" to atoms and every other
// level to itself, so two levels of the strings are equal words iff their bytes are equal; a
// substituted placeholder is a binary, which equals a topic level only if that level is not one
// of the three atoms.  `pattern`: substitute placeholder levels from the client (feed_var/3).
EMQX_HD bool az_match_filter(const uint8_t* t, uint32_t tn, const uint8_t* f, uint32_t fn, bool pattern,
                             const AzClient& c, const uint8_t* carena) {
  uint32_t ts = 0, fs = 0;
  bool tend = false, fend = false;  // word list exhausted (a string always has one level)
  for (;;) {
    if (fend) return tend;  // match([], []) / match([_|_], [])
    const uint32_t fe = az_level_end(f, fs, fn);
    const bool flast = fe == fn;
    const bool fhash = flast && fe - fs == 1 && f[fs] == '#';
    if (tend) return fhash;  // match([], ['#']) / match([], [_|_])
    const uint32_t te = az_level_end(t, ts, tn);
    const uint32_t tl = te - ts, fl = fe - fs;
    bool equal;
    const uint32_t ph = pattern ? az_placeholder(f, fs, fe) : 0u;
    if (ph == 1 && (c.present & AZ_HAS_CLIENTID)) {
      const bool atom = tl == 0 || (tl == 1 && (t[ts] == '+' || t[ts] == '#'));
      equal = !atom && tl == c.cid_len && az_bytes_eq(t + ts, carena + c.cid_off, tl);
    } else if (ph == 2 && (c.present & AZ_HAS_USERNAME)) {
      const bool atom = tl == 0 || (tl == 1 && (t[ts] == '+' || t[ts] == '#'));
      equal = !atom && tl == c.user_len && az_bytes_eq(t + ts, carena + c.user_off, tl);
    } else {
      equal = tl == fl && az_bytes_eq(t + ts, f + fs, tl);
    }
    if (!equal && !(fl == 1 && f[fs] == '+')) return fhash;  // match(_, ['#']) or the false clauses
    // match([H|T1], [H|T2]) and match([_|T1], ['+'|T2])
    if (te == tn) tend = true; else ts = te + 1;
    if (flast) fend = true; else fs = fe + 1;
  }
}

EMQX_HD bool az_leaf(const AzView& v, const AzLeaf& l, const AzClient& c) {
  switch (l.kind) {
    case AZ_LEAF_USERNAME:
      return (c.present & AZ_HAS_USERNAME) && l.b == c.user_len && az_bytes_eq(v.arena + l.a, v.carena + c.user_off, l.b);
    case AZ_LEAF_CLIENTID:
      return (c.present & AZ_HAS_CLIENTID) && l.b == c.cid_len && az_bytes_eq(v.arena + l.a, v.carena + c.cid_off, l.b);
    case AZ_LEAF_CIDR: {
      if (!(c.present & AZ_HAS_IPV4)) return false;
      for (uint32_t i = 0; i < l.b; ++i)
        if (v.cidrs[l.a + i].lo <= c.ipv4 && c.ipv4 <= v.cidrs[l.a + i].hi) return true;
      return false;
    }
    case AZ_LEAF_FLAG:
      return ((c.flags >> (l.a & 63u)) & 1u) != 0;
    default:
      return false;
  }
}

// match_who/2: 'and' folds from true, 'or' from false (:157-164).
EMQX_HD bool az_who(const AzView& v, const AzRule& r, const AzClient& c) {
  if (r.who_op == AZ_WHO_ALL) return true;
  const bool conj = r.who_op == AZ_WHO_AND;
  if (r.who_op == AZ_WHO_ONE) return r.n_who == 1 && az_leaf(v, v.leaves[r.who_begin], c);
  for (uint32_t i = 0; i < r.n_who; ++i)
    if (az_leaf(v, v.leaves[r.who_begin + i], c) != conj) return !conj;
  return conj;
}

// Does entry e decide the request (client c, action bit, topic)?  match/4 for the entry's rule
// restricted to this one filter of it: a rule matches iff one of its entries does.
EMQX_HD bool az_entry_hit(const AzView& v, const AzEntry& e, const AzClient& c, uint32_t action_bit,
                          const uint8_t* t, uint32_t tn) {
  const AzRule& r = v.rules[e.rule];
  if (!(r.action_mask & action_bit)) return false;
  const uint8_t* f = v.arena + e.off;
  const bool m = e.kind == AZ_EQ ? (tn == e.len && az_bytes_eq(t, f, tn))
                                 : az_match_filter(t, tn, f, e.len, e.kind == AZ_PATTERN, c, v.carena);
  return m && az_who(v, r, c);
}

// The whole check of one request on one thread: the host evaluator, and the kernels' path for
// one lane per request.  Returns the verdict; *tag = the deciding rule's tag; *evals += entries tried.
EMQX_HD uint32_t az_check(const AzView& v, uint32_t client, uint32_t action, const uint8_t* t, uint64_t tn,
                          uint32_t* tag, uint64_t* evals) {
  *tag = AZ_TAG_NONE;
  if (client >= v.n_clients || action < 1 || action > 2 || tn > 0xFFFFFFFFull) return AZ_BAD;
  const AzClient& c = v.clients[client];
  if (!(c.present & AZ_REGISTERED)) return AZ_BAD;
  const AzRange* segs = v.segs + static_cast<uint64_t>(client) * AZ_SEG_STRIDE;
  for (uint32_t s = 0; s < c.n_seg; ++s)
    for (uint32_t i = segs[s].lo; i < segs[s].hi; ++i) {
      ++*evals;
      if (az_entry_hit(v, v.entries[i], c, action, t, static_cast<uint32_t>(tn))) {
        const AzRule& r = v.rules[v.entries[i].rule];
        *tag = r.tag;
        return r.permission;
      }
    }
  return AZ_NOMATCH;
}

}  // namespace emqx
