/*
 * emqx_select.h — C ABI of the owner table and the batched select stage (libemqxmatch.so): the
 * 'message.publish' hook fold between the authorization check and emqx_broker:publish/1.
 *
 * Every configured hook consumer asks, per published message, whether the topic matches one of
 * its filters.  Paths are relative to the reference checkout (xiongzhenhai-zh/emqx,
 * EMQX 5.0.0-beta.3):
 *
 *   emqx_rule_events:on_message_publish/2        apps/emqx_rule_engine/src/emqx_rule_events.erl:98-107
 *     -> emqx_rule_engine:get_rules_for_topic/1  apps/emqx_rule_engine/src/emqx_rule_engine.erl:157-160
 *     -> can_topic_match_oneof/2                 apps/emqx_plugin_libs/src/emqx_plugin_libs_rule.erl:265-268
 *        lists:any(emqx_topic:match(Topic, F), From) over every rule; skipped for a sys message
 *        under ignore_sys_message (emqx_rule_events.erl:608-611)
 *   emqx_bridge:on_message_publish/1             apps/emqx_bridge/src/emqx_bridge.erl:84-91
 *     -> get_matched_bridges/1                   emqx_bridge.erl:309-328
 *        one local_topic per bridge; enable = false and direction = ingress never match; sys
 *        messages are skipped
 *   emqx_exhook_server:match_topic_filter/2      apps/emqx_exhook/src/emqx_exhook_server.erl:282-285
 *        lists:any over the hook's topics; AN EMPTY LIST MATCHES EVERY TOPIC
 *
 * The match engine answers {F : emqx_topic:match(T, F)} for a batch as a CSR of filter ids
 * (emqx_match_batch_device*).  This stage turns that CSR into the CSR of consumers ("owners"):
 * each owner at most once per message, however many of its filters matched and however many
 * owners share a filter; restricted to the owner classes that apply to the message; plus the
 * match-everything owners.  The fan-out cannot do this: it emits one delivery per
 * (subscriber, filter) pair on purpose.
 *
 * For one message i the output is exactly the set, no owner twice, in no particular order:
 *
 *   { o : enabled(o) and class(o) in msg_classes[i]
 *         and (MATCH_ALL(o) or some entry e of message i has o in postings(filters[e])) }
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  One writer (set / enable / remove
 * / commit) at a time; any number of concurrent select callers read the committed, immutable
 * snapshot.
 */
#ifndef EMQX_SELECT_H
#define EMQX_SELECT_H

#include <stdint.h>

#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_owntab emqx_owntab;

#define EMQX_SELECT_HOST_ONLY (-2)       /* `device` of a handle without a device               */
#define EMQX_SELECT_MAX_FILTER (1u << 30) /* filter ids are below this (the fan-out's flag bits) */
#define EMQX_SELECT_MAX_OWNER (1u << 30)  /* owner ids are below this: they index a dense array  */
#define EMQX_SELECT_ALL_CLASSES 0xFFFFFFFFu

/* `flags` of emqx_owntab_set. */
#define EMQX_OWNER_ENABLED 0x1u   /* without it the owner is kept but never selected             */
#define EMQX_OWNER_MATCH_ALL 0x2u /* exhook's empty topic list: selected for every message       */

/* summary[8]: [0] flags, [1] CSR entries read, [2] postings examined (the posting lists of the
 * entries with a known filter id, before any test), [3] owners selected, [4] messages with at
 * least one owner, [5] duplicates dropped (postings of enabled owners of an applicable class
 * that an earlier entry of the same message had selected already), [6] entries whose filter id
 * the table does not know (no owner with a filter list holds it), [7] the largest per-message
 * count. */
#define EMQX_SELECT_SUMMARY_WORDS 8
#define EMQX_SELECT_F_OUT_OVERFLOW 0x1u  /* selected > cap_out: out_offsets complete, out_owners untouched */
#define EMQX_SELECT_F_INPUT_REFUSED 0x2u /* offsets[n] > cap_in: nothing read or written but the summary   */

/* One select call.  Every pointer is host memory for emqx_select_batch (the function) and
 * emqx_select_host, device memory for the _device forms.
 *
 * In:  the match CSR exactly as emqx_match_batch_device* writes it: offsets[n+1] with
 *      offsets[0] = 0, filters[] of capacity cap_in (engine ids, or the ext ids of
 *      emqx_insert_filters_ext).  A filter id may occur more than once in a message.  Ids the
 *      table does not know, 0xFFFFFFFF included, select nothing.
 *      msg_classes[n]: bit c set = owners of class c apply to message i; NULL = every class.
 *      The caller clears the rule and bridge bits of a sys message (ignore_sys_message,
 *      emqx_bridge.erl:85).
 * Out: out_offsets[n+1], out_owners[] of capacity cap_out.  A match-all owner is selected for a
 *      message without entries too, so the output is not bounded by the input. */
struct emqx_select_batch {
  const uint64_t* offsets;
  const uint32_t* filters;
  uint64_t n;
  uint64_t cap_in;
  const uint32_t* msg_classes;
  uint64_t* out_offsets;
  uint32_t* out_owners;
  uint64_t cap_out;
};

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_owntab_stats) before the call. */
typedef struct emqx_owntab_stats {
  uint64_t size;        /* in: sizeof(emqx_owntab_stats) of the caller; out: bytes written */
  uint64_t n_owners;    /* owners of the committed snapshot                                 */
  uint64_t n_filters;   /* filter ids with at least one owner                               */
  uint64_t n_postings;  /* (filter, owner) pairs                                            */
  uint64_t n_match_all; /* match-all owners, enabled or not                                 */
  uint64_t max_list;    /* longest posting list                                             */
  uint64_t epoch;       /* commits so far                                                   */
  double last_build_ms; /* host build + upload time of the last commit                      */
  double last_call_ms;  /* time of the last synchronous select call                         */
} emqx_owntab_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_SELECT_HOST_ONLY: a handle that takes
 * changes, commits and answers emqx_select_host; its batch entry points return EMQX_EDEVICE
 * (nothing ever falls back to the host silently). */
int emqx_owntab_create(int32_t device, emqx_owntab** out);
int emqx_owntab_destroy(emqx_owntab* h);

/* Replaces the record of owner `owner`: its class (class_bit 0..31, assigned by the caller:
 * e.g. rules 0, bridges 1, one bit per exhook hook point), its flags (EMQX_OWNER_*) and the n
 * filter ids of its filters.  Duplicate ids within the list are collapsed.  n = 0 without
 * MATCH_ALL: the owner is never selected (lists:any(_, []) is false).  With MATCH_ALL the list
 * is not consulted.  EMQX_EINVAL, nothing changed: class_bit > 31, unknown flag bits, a filter
 * id >= 2^30, an owner id >= 2^30. */
int emqx_owntab_set(emqx_owntab* h, uint32_t owner, uint32_t class_bit, uint32_t flags, const uint32_t* filter_ids,
                    uint64_t n);
/* Sets (on != 0) or clears EMQX_OWNER_ENABLED of n owners; unknown owners are ignored. */
int emqx_owntab_enable(emqx_owntab* h, const uint32_t* owners, uint64_t n, int32_t on);
/* Removes n owners; unknown owners are ignored. */
int emqx_owntab_remove(emqx_owntab* h, const uint32_t* owners, uint64_t n);
/* Builds the posting lists of every owner set so far (ascending and unique per filter), uploads
 * them with one copy and swaps them in.  Calls in flight keep the snapshot they started on;
 * changes are invisible to select calls until a commit. */
int emqx_owntab_commit(emqx_owntab* h);

/* Host buffers, evaluated on the device.  EMQX_EINVAL: offsets[0] != 0, decreasing offsets,
 * offsets[n] > cap_in.  *n_out (may be NULL) = the owners selected; when they exceed cap_out:
 * EMQX_EOVERFLOW, *n_out = the capacity needed, out_offsets complete, out_owners untouched.
 * summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_select_batch(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out, uint64_t* summary_out);
/* Device buffers, on `stream` (NULL: the table's own, ordered after the device's null stream);
 * synchronizes the stream.  The entry count is read on the device.  Returns as above;
 * offsets[n] > cap_in: EMQX_EINVAL with summary flag bit 1.  summary_out: host, may be NULL. */
int emqx_select_batch_device(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out,
                             uint64_t* summary_out, void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains behind
 * emqx_match_batch_device_async on the same stream.  The entry count is read on the device as
 * offsets[n], because that call never tells the host.  `summary` (>= 8 uint64_t, device or
 * host-pinned memory) is written when the stream reaches it.  Whatever the device offsets hold,
 * no access leaves the buffers.  The snapshot the call reads stays alive until the call has
 * drained. */
int emqx_select_batch_device_async(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* summary,
                                   void* stream);
/* The same sets computed on the calling thread over the same committed snapshot, with the same
 * predicate code the kernels run: the per-call path and the checker of the batch path. */
int emqx_select_host(emqx_owntab* h, const struct emqx_select_batch* b, uint64_t* n_out, uint64_t* summary_out);

/* Keys: "max_blocks" (1..16384, default 16384): the grid cap of the by-entry passes; the blocks
 * stride over the tiles beyond it (tests lower it to make them stride); "scan_chunk" (1..1024,
 * default 1024): the tile totals the one-block scans take per carry step (tests lower it to make
 * them carry; the same bytes at every value).  EMQX_ENOTFOUND for unknown keys. */
int emqx_owntab_set_tuning(emqx_owntab* h, const char* key, int64_t value);
int emqx_owntab_stats_get(emqx_owntab* h, emqx_owntab_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_SELECT_H */
