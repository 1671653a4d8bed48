/*
 * emqx_authz.h — C ABI of the batched authorization (ACL) table (libemqxmatch.so).
 *
 * The check every PUBLISH and every SUBSCRIBE filter passes before the route lookup, for the
 * sources that hold their rules in memory.  Paths are relative to the reference checkout
 * (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_channel:check_pub_authz/2, check_sub_authzs/2   apps/emqx/src/emqx_channel.erl:1515-1547
 *     -> emqx_access_control:authorize/3 -> 'client.authorize' -> emqx_authz:authorize/5
 *     -> do_authorize/4 over the sources in order       apps/emqx_authz/src/emqx_authz.erl:270-314
 *       -> emqx_authz_check_batch* / emqx_authz_check_host: sources 0..7 in index order
 *   emqx_authz_file (one ordered rule list)             -> a source with only an ALL list
 *   emqx_authz_mnesia:authorize/4                       apps/emqx_authz/src/emqx_authz_mnesia.erl:95-111
 *       clientid rules ++ username rules ++ all rules   -> the three scopes of a source, in that order
 *   emqx_authz_rule:compile/1                           apps/emqx_authz/src/emqx_authz_rule.erl:55-94
 *       -> emqx_authz_list_set ("eq " prefix, ${clientid} / ${username} whole levels, CIDRs)
 *   emqx_authz_rule:matches/4, match/4                  emqx_authz_rule.erl:108-130
 *       first rule whose action, who and one topic filter match decides
 *   emqx_authz_rule:match_who/2                         emqx_authz_rule.erl:132-165
 *   emqx_authz_rule:match_topics/3, feed_var/2          emqx_authz_rule.erl:167-195
 *       emqx_topic:match/2 on word LISTS (apps/emqx/src/emqx_topic.erl:74-87): the '$' clauses
 *       (:68-71) are binary clauses and do not apply, so '#' and '+/...' match '$SYS/...' here.
 *       That is why emqx_topic_match (emqx_match.h), which applies the '$' rule, is not this check.
 *
 * Kept by the caller: the no_match default (emqx_authz.erl:294-301; verdict 0 is returned as
 * such), superuser, the authz cache, metrics, logging.  Regex who terms ({username, {re, _}},
 * {clientid, {re, _}}, PCRE on the Erlang side) are inputs: the caller runs re:run/2 once per
 * client and rule regex at connect time, sets a bit of the client's 64-bit flag word, and the
 * rule carries a who leaf EMQX_AUTHZ_WHO_FLAG naming that bit.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes, packed byte buffers + uint64
 * offsets[n+1].  One writer (list_set / source_clear / clients_set / clients_drop / commit) at
 * a time; any number of concurrent check callers read the committed, immutable snapshot.
 */
#ifndef EMQX_AUTHZ_H
#define EMQX_AUTHZ_H

#include <stdint.h>

#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_authz emqx_authz;

#define EMQX_AUTHZ_MAX_SOURCES 8
#define EMQX_AUTHZ_HOST_ONLY (-2) /* `device` of a handle without a device */

enum { EMQX_AUTHZ_SCOPE_ALL = 0, EMQX_AUTHZ_SCOPE_CLIENTID = 1, EMQX_AUTHZ_SCOPE_USERNAME = 2 };
enum { EMQX_AUTHZ_ALLOW = 1, EMQX_AUTHZ_DENY = 2 };                        /* permission, verdict */
enum { EMQX_AUTHZ_NOMATCH = 0, EMQX_AUTHZ_BAD_REQUEST = 3 };               /* verdict only        */
enum { EMQX_AUTHZ_PUBLISH = 1, EMQX_AUTHZ_SUBSCRIBE = 2, EMQX_AUTHZ_ALL = 3 }; /* action (requests: 1..2) */
enum { EMQX_AUTHZ_WHO_ALL = 0, EMQX_AUTHZ_WHO_ONE = 1, EMQX_AUTHZ_WHO_AND = 2, EMQX_AUTHZ_WHO_OR = 3 };
enum { EMQX_AUTHZ_WHO_USERNAME = 1, EMQX_AUTHZ_WHO_CLIENTID = 2, EMQX_AUTHZ_WHO_CIDR = 3, EMQX_AUTHZ_WHO_FLAG = 4 };
enum { EMQX_AUTHZ_HAS_CLIENTID = 1, EMQX_AUTHZ_HAS_USERNAME = 2, EMQX_AUTHZ_HAS_IPV4 = 4 }; /* present[] bits */
#define EMQX_AUTHZ_TAG_NONE 0xFFFFFFFFu

/* One rule {permission, who, action, topic_filters} (emqx_authz_rule.erl:49).  Its who leaves
 * are the next n_who entries of the call's leaf array (rules consume it in order); its topic
 * filters are strings [first_topic, first_topic + n_topics) of the call's string array.
 * {Permission, all} is {Permission, all, all, ["#"]} (:55-56).  n_topics = 0: never matches. */
typedef struct emqx_authz_rule {
  uint8_t permission; /* EMQX_AUTHZ_ALLOW / _DENY                                     */
  uint8_t action;     /* EMQX_AUTHZ_PUBLISH / _SUBSCRIBE / _ALL                       */
  uint8_t who_op;     /* EMQX_AUTHZ_WHO_ALL (n_who 0) / _ONE (n_who 1) / _AND / _OR   */
  uint8_t eq_topics;  /* 1: every filter of the rule is {eq, _} whatever its bytes    */
  uint32_t n_who;
  uint32_t first_topic;
  uint32_t n_topics;
  uint32_t tag;       /* returned for the requests this rule decides                  */
} emqx_authz_rule;

/* One who leaf.  USERNAME / CLIENTID: `operand` = index of the string compared byte for byte;
 * CIDR: strings [operand, operand + count) are IPv4 addresses "a.b.c.d" or "a.b.c.d/len",
 * true if the peer host lies in any ({ipaddr, _}: count 1; {ipaddrs, L}: count = length(L));
 * FLAG: `operand` = bit 0..63 of the client's flag word. */
typedef struct emqx_authz_who {
  uint32_t kind;
  uint32_t operand;
  uint32_t count; /* CIDR only (else 0) */
} emqx_authz_who;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_authz_stats) before the call. */
typedef struct emqx_authz_stats {
  uint64_t size;         /* in: sizeof(emqx_authz_stats) of the caller; out: bytes written  */
  uint64_t n_sources;    /* sources with at least one list (committed snapshot, as below)   */
  uint64_t n_lists;
  uint64_t n_rules;
  uint64_t n_entries;    /* filter entries                                                  */
  uint64_t n_clients;    /* registered clients                                              */
  uint64_t table_bytes;  /* bytes of the snapshot's arrays                                  */
  uint64_t epoch;        /* commits so far                                                  */
  uint64_t last_evals;   /* filter entries the last check call evaluated                    */
  uint64_t last_group;   /* lanes per request of the last device call (1, 4, 16 or 64)      */
  double last_build_ms;  /* host build + upload time of the last commit                     */
  double last_check_ms;  /* time of the last synchronous check call                         */
} emqx_authz_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_AUTHZ_HOST_ONLY: a handle that compiles rules, commits and
 * answers emqx_authz_check_host; its batch entry points return EMQX_EDEVICE (nothing ever
 * falls back to the host silently). */
int emqx_authz_create(int32_t device, emqx_authz** out);
int emqx_authz_destroy(emqx_authz* a);

/* Replaces the rule list (source, scope, key) — key: the client id or username the list belongs
 * to, ignored for SCOPE_ALL.  n_rules = 0 removes it.  A filter string that starts with "eq "
 * is {eq, rest}; a filter with a whole level ${clientid} or ${username} is a pattern.
 * EMQX_EINVAL with a message in err (err_cap bytes, NUL-terminated, may be NULL), nothing
 * changed: an IPv6 or malformed CIDR, permission / action / who_op / leaf kind outside the
 * enumerations, WHO_ALL with leaves or WHO_ONE without exactly one (nesting has no encoding),
 * a flag bit over 63, an index outside the arrays, a string used as filter or principal that
 * is longer than 65535 bytes, source >= EMQX_AUTHZ_MAX_SOURCES. */
int emqx_authz_list_set(emqx_authz* a, uint32_t source, uint32_t scope, const uint8_t* key, uint64_t key_len,
                        const emqx_authz_rule* rules, uint64_t n_rules, const emqx_authz_who* who, uint64_t n_who,
                        const uint8_t* bytes, const uint64_t* offsets, uint64_t n_strings, char* err,
                        uint64_t err_cap);
int emqx_authz_source_clear(emqx_authz* a, uint32_t source);

/* Registers (or replaces) n clients.  ids are the caller's dense client numbers (the tables are
 * indexed by them).  present[i]: EMQX_AUTHZ_HAS_* bits; a field whose bit is clear is
 * `undefined` (its bytes / address are ignored).  ipv4[i]: the peer host, a.b.c.d as
 * (a << 24 | b << 16 | c << 8 | d); a client without the bit (no peer host, or an IPv6 one)
 * fails every CIDR leaf.  flags may be NULL (all 0).  A client id or username over 65535 bytes:
 * EMQX_EINVAL, nothing changed. */
int emqx_authz_clients_set(emqx_authz* a, const uint32_t* ids, uint64_t n, const uint8_t* clientid_bytes,
                           const uint64_t* clientid_offsets, const uint8_t* username_bytes,
                           const uint64_t* username_offsets, const uint32_t* ipv4, const uint8_t* present,
                           const uint64_t* flags);
int emqx_authz_clients_drop(emqx_authz* a, const uint32_t* ids, uint64_t n);

/* Builds the snapshot of every list and client set so far, uploads it and swaps it in.  Checks
 * in flight keep the snapshot they started on; changes after a commit are invisible to checks
 * until the next one. */
int emqx_authz_commit(emqx_authz* a);

/* Checks n requests (clients[i], actions[i], topic i) against the committed snapshot.
 * verdict_out[i]: 0 nomatch, 1 allow, 2 deny, 3 bad request (a client id that is not
 * registered, an action outside 1..2; on the device entry points also a topic whose offsets
 * decrease).  tag_out (may be NULL): the deciding rule's tag or EMQX_AUTHZ_TAG_NONE.  A bad
 * request never fails the batch.  Host buffers; offsets that decrease: EMQX_EINVAL. */
int emqx_authz_check_batch(emqx_authz* a, const uint32_t* clients, const uint8_t* actions,
                           const uint8_t* topic_bytes, const uint64_t* topic_offsets, uint64_t n,
                           uint8_t* verdict_out, uint32_t* tag_out);
/* Same with every buffer in device memory, on `stream` (NULL: the table's own, ordered after
 * the device's null stream).  Synchronizes the stream before returning. */
int emqx_authz_check_batch_device(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                  const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets, uint64_t n,
                                  uint8_t* d_verdict_out, uint32_t* d_tag_out, void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains in front of
 * emqx_match_batch_device_async on the same stream.  `summary` (>= 8 uint64_t, device or
 * host-pinned memory) receives, when the stream reaches it: [0] flags (0 = complete),
 * [1] allow, [2] deny, [3] nomatch, [4] bad requests, [5] entries evaluated.  The snapshot the
 * call reads stays alive until the call has drained. */
int emqx_authz_check_batch_device_async(emqx_authz* a, const uint32_t* d_clients, const uint8_t* d_actions,
                                        const uint8_t* d_topic_bytes, const uint64_t* d_topic_offsets,
                                        uint64_t n, uint8_t* d_verdict_out, uint32_t* d_tag_out,
                                        uint64_t* summary, void* stream);
/* The same outputs computed on the calling thread over the same committed snapshot, with the
 * same predicate code the kernels run: the per-call path (one SUBSCRIBE needs no device round
 * trip) and the checker of the batch path. */
int emqx_authz_check_host(emqx_authz* a, const uint32_t* clients, const uint8_t* actions,
                          const uint8_t* topic_bytes, const uint64_t* topic_offsets, uint64_t n,
                          uint8_t* verdict_out, uint32_t* tag_out);

/* Lanes per request of the device kernel: 0 = chosen per call from the snapshot's longest
 * request and the batch size (default), or 1, 4, 16, 64 (experiments and tests; results never
 * depend on it).  Key "group"; EMQX_ENOTFOUND for unknown keys. */
int emqx_authz_set_tuning(emqx_authz* a, const char* key, int64_t value);
int emqx_authz_stats_get(emqx_authz* a, emqx_authz_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_AUTHZ_H */
