/*
 * emqx_deliver.h — C ABI of the delivery-options table and the batched enrich stage
 * (libemqxmatch.so): the step behind the publish fan-out.
 *
 * emqx_publish_batch / emqx_fanout_batch_device* end at a CSR of deliveries (subscriber id,
 * filter id) per message, what emqx_broker:dispatch/2 sends as {deliver, Topic, Msg}.  In the
 * reference every one of them passes two more steps in the subscriber's channel, both keyed by
 * (subscriber, topic filter) in the session's subscription map.  Paths are relative to the
 * reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_channel:handle_deliver/2                      apps/emqx/src/emqx_channel.erl:788-807
 *     -> emqx_session:ignore_local/3                   apps/emqx/src/emqx_session.erl:280-291
 *          nl = 1 and Subscriber =:= Publisher: dropped ('delivery.dropped.no_local')
 *     -> emqx_session:deliver/2 -> enrich_fun/1        emqx_session.erl:554-557
 *          get_subopts/2                               emqx_session.erl:569-576
 *          enrich_subopts/3                            emqx_session.erl:578-598
 *            nl flag, qos = min(SubQoS, PubQoS) (max under upgrade_qos), retain cleared unless
 *            rap = 1 or headers.retained = true, the 'Subscription-Identifier' property
 *
 * A delivery d of message i has subscriber s = subs[d] and filter
 * f = filters[d] & ~(EMQX_FANOUT_SHARED_BIT | EMQX_FANOUT_RETRY_BIT); its key is the ORDERED pair
 * (f, s).  A $share subscription and a plain one of the same client on the same filter share one
 * key: the session map is keyed by the topic filter without the share prefix, the later set
 * replaces the earlier one.
 *
 * The lists:dropwhile quirk.  ignore_local/3 is a dropwhile: over a list of several delivers
 * drained from one mailbox it drops only the leading run of hits.  How delivers are grouped per
 * drain is runtime timing, not a property of a publish batch, so this stage reports the
 * predicate PER DELIVERY, which is exactly what ignore_local does for a one-element list, and
 * the compacted form drops every hit, as MQTT 5 section 3.8.3.1 requires (a No Local
 * subscription never receives its own publishes).
 *
 * Kept by the caller: inflight, mqueue and packet ids, maybe_ack / maybe_nack, Retain Handling
 * (acts at SUBSCRIBE time), and the MQTT v3 ignore_loop_deliver / is_bridge mapping
 * (emqx_channel.erl:1570), which the caller folds into the options it sets.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  One writer (set / remove /
 * drop_subscribers / commit) at a time; any number of concurrent enrich callers read the
 * committed, immutable snapshot.
 */
#ifndef EMQX_DELIVER_H
#define EMQX_DELIVER_H

#include <stdint.h>

#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_subopts emqx_subopts;

#define EMQX_DELIVER_HOST_ONLY (-2)           /* `device` of a handle without a device */
#define EMQX_DELIVER_NO_SENDER 0xFFFFFFFFu    /* msg_from[i] of a message without a publishing client */
#define EMQX_DELIVER_MAX_FILTER (1u << 30)    /* filter ids are below this (the fan-out's flag bits) */
#define EMQX_DELIVER_MAX_SUBID 268435455u     /* Subscription Identifier: 1..268435455 */

/* Stored options word of a subscription (emqx_types:subopts()). */
#define EMQX_SUBOPT_QOS_MASK 0x03u
#define EMQX_SUBOPT_NL 0x04u          /* nl = 1                                   */
#define EMQX_SUBOPT_RAP 0x08u         /* rap = 1                                  */
#define EMQX_SUBOPT_UPGRADE_QOS 0x10u /* upgrade_qos of the session's zone        */
#define EMQX_SUBOPT_HAS_SUBID 0x20u   /* the subscription carries a subid         */

/* msg_flags[i]. */
#define EMQX_MSG_RETAIN 0x01u   /* the message's retain flag                                 */
#define EMQX_MSG_RETAINED 0x02u /* headers.retained = true (the retainer's dispatch path)    */

/* Output byte of a delivery. */
#define EMQX_DELIVER_QOS_MASK 0x03u
#define EMQX_DELIVER_RETAIN 0x04u
#define EMQX_DELIVER_NL 0x08u            /* the nl flag enrich_subopts sets on the message              */
#define EMQX_DELIVER_DROP_NO_LOCAL 0x10u /* ignore_local's predicate: nl = 1 and the subscriber published */
#define EMQX_DELIVER_NO_SUBOPTS 0x20u    /* key absent: get_subopts -> [], the message is unchanged     */
#define EMQX_DELIVER_BAD_MESSAGE 0x40u   /* msg_qos > 2 or unknown msg_flags bits: exactly this, kept    */

/* summary[8]: [0] flags, [1] deliveries, [2] kept, [3] dropped no_local, [4] no_subopts,
 * [5..7] kept deliveries at qos 0 / 1 / 2 (bad messages count in none of them). */
#define EMQX_DELIVER_SUMMARY_WORDS 8
#define EMQX_DELIVER_F_KEPT_OVERFLOW 0x1u /* kept > cap_kept: kept_offsets complete, kept arrays untouched */
#define EMQX_DELIVER_F_INPUT_REFUSED 0x2u /* offsets[n] > cap_in: nothing read or written but the summary  */

/* One enrich call.  Every pointer is host memory for emqx_deliver_enrich_batch and
 * emqx_deliver_enrich_host, device memory for the _device forms.
 *
 * In:  the delivery CSR exactly as the fan-out writes it, offsets[n+1] with offsets[0] = 0,
 *      subs[] and filters[] of capacity cap_in; per message msg_qos[n] (0..2), msg_flags[n]
 *      (EMQX_MSG_*), msg_from[n] (the publishing client's subscriber id or
 *      EMQX_DELIVER_NO_SENDER; NULL: no message has a sender).
 * Out: out_opts[offsets[n]] (EMQX_DELIVER_* byte per delivery), out_subids[] (optional; 0: none).
 *      - key absent: qos = msg_qos, retain = bit 0 of msg_flags, nl 0, not dropped, NO_SUBOPTS, subid 0
 *      - key present: DROP_NO_LOCAL = nl && msg_from[i] == s; nl flag = nl;
 *        qos = upgrade ? max(sub, pub) : min(sub, pub);
 *        retain = rap ? retain_in : (retained_hdr ? retain_in : 0); subid as stored or 0.
 *        A dropped delivery still gets the other fields, computed the same way.
 *      - bad message: every delivery of it gets exactly EMQX_DELIVER_BAD_MESSAGE and subid 0 and
 *        is kept; a bad message never fails a batch.
 * Compaction, only when kept_offsets != NULL: the CSR without the DROP_NO_LOCAL deliveries,
 *      kept_offsets[n+1], kept_subs, kept_filters, kept_opts (all required), kept_subids
 *      (optional), of capacity cap_kept, distinct from the input buffers.  Order within a message
 *      is preserved; kept_filters carry the SHARED and RETRY bits untouched. */
typedef struct emqx_deliver_batch {
  const uint64_t* offsets;
  const uint32_t* subs;
  const uint32_t* filters;
  uint64_t n;
  uint64_t cap_in;
  const uint8_t* msg_qos;
  const uint8_t* msg_flags;
  const uint32_t* msg_from;
  uint8_t* out_opts;
  uint32_t* out_subids;
  uint64_t* kept_offsets;
  uint32_t* kept_subs;
  uint32_t* kept_filters;
  uint8_t* kept_opts;
  uint32_t* kept_subids;
  uint64_t cap_kept;
} emqx_deliver_batch;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_subopts_stats) before the call. */
typedef struct emqx_subopts_stats {
  uint64_t size;        /* in: sizeof(emqx_subopts_stats) of the caller; out: bytes written */
  uint64_t n_entries;   /* (filter, subscriber) pairs of the committed snapshot             */
  uint64_t n_slots;     /* slots of its hash table                                          */
  uint64_t table_bytes; /* 16 bytes a slot                                                  */
  uint64_t epoch;       /* commits so far                                                   */
  uint64_t max_probe;   /* longest probe run: slots a lookup reads at most                  */
  double last_build_ms; /* host build + upload time of the last commit                      */
  double last_call_ms;  /* time of the last synchronous enrich call                         */
} emqx_subopts_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_DELIVER_HOST_ONLY: a handle that
 * takes changes, commits and answers emqx_deliver_enrich_host; its batch entry points return
 * EMQX_EDEVICE (nothing ever falls back to the host silently). */
int emqx_subopts_create(int32_t device, emqx_subopts** out);
int emqx_subopts_destroy(emqx_subopts* h);

/* Upsert of n subscriptions, as maps:put/3 in emqx_session:subscribe/4: opts[i] is the
 * EMQX_SUBOPT_* word, subids[i] (subids may be NULL when no word has HAS_SUBID) the
 * Subscription Identifier.  EMQX_EINVAL, nothing changed: a filter id >= 2^30, qos 3, bits
 * above EMQX_SUBOPT_HAS_SUBID, HAS_SUBID with a subid outside 1..268435455. */
int emqx_subopts_set(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, const uint8_t* opts,
                     const uint32_t* subids, uint64_t n);
/* Removes n pairs (UNSUBSCRIBE); absent pairs are ignored. */
int emqx_subopts_remove(emqx_subopts* h, const uint32_t* filter_ids, const uint32_t* sub_ids, uint64_t n);
/* Removes every pair of these subscribers (the session ended). */
int emqx_subopts_drop_subscribers(emqx_subopts* h, const uint32_t* sub_ids, uint64_t n);
/* Builds the hash table of every pair set so far, uploads it and swaps it in.  Calls in flight
 * keep the snapshot they started on; changes are invisible to enrich calls until a commit. */
int emqx_subopts_commit(emqx_subopts* h);

/* Host buffers, evaluated on the device.  EMQX_EINVAL: offsets[0] != 0, decreasing offsets,
 * offsets[n] > cap_in.  With compaction, *n_kept (may be NULL) = the kept deliveries; when they
 * exceed cap_kept: EMQX_EOVERFLOW, *n_kept = the capacity needed, kept_offsets and the
 * per-delivery outputs complete, the kept arrays untouched.  summary_out (host, may be NULL)
 * receives the 8 summary words. */
int emqx_deliver_enrich_batch(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out);
/* Device buffers, on `stream` (NULL: the table's own, ordered after the device's null stream);
 * synchronizes the stream.  The delivery count is read on the device.  Returns as above;
 * offsets[n] > cap_in: EMQX_EINVAL with summary flag bit 1.  summary_out: host, may be NULL. */
int emqx_deliver_enrich_batch_device(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept,
                                     uint64_t* summary_out, void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains behind
 * emqx_fanout_batch_device_async on the same stream.  The delivery count is read on the device
 * as offsets[n], because that call never tells the host.  `summary` (>= 8 uint64_t, device or
 * host-pinned memory) is written when the stream reaches it.  Whatever the device offsets hold,
 * no access leaves the buffers.  The snapshot the call reads stays alive until the call has
 * drained. */
int emqx_deliver_enrich_batch_device_async(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* summary,
                                           void* stream);
/* The same outputs computed on the calling thread over the same committed snapshot, with the
 * same predicate code the kernels run: the per-call path and the checker of the batch path. */
int emqx_deliver_enrich_host(emqx_subopts* h, const emqx_deliver_batch* b, uint64_t* n_kept, uint64_t* summary_out);

/* Keys: "max_load_pct" (10..95, default 50): the fill of the hash table the next commit builds
 * (tests raise it to lengthen the probe runs); "max_blocks" (1..16384, default 16384): the grid cap
 * of the by-tile passes (evaluate and scatter), the blocks stride over the tiles beyond it;
 * "scan_chunk" (1..1024, default 1024): the tile totals the one-block scan takes per carry step
 * (tests lower both to make the blocks stride and the scan carry at small shapes; the same bytes
 * at every value).  Both are read when a call is enqueued; a host-only handle accepts and ignores
 * them.  EMQX_EINVAL out of range, EMQX_ENOTFOUND for unknown keys. */
int emqx_subopts_set_tuning(emqx_subopts* h, const char* key, int64_t value);
int emqx_subopts_stats_get(emqx_subopts* h, emqx_subopts_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_DELIVER_H */
