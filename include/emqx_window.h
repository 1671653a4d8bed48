/*
 * emqx_window.h — C ABI of the window stage (libemqxmatch.so): inflight and mqueue admission per
 * inbox, the step behind the inbox stage (emqx_inbox_group_batch_device*).
 *
 * The inbox stage ends at the list emqx_channel:handle_deliver/2 takes.  What the session does
 * with that list is a fold over it.  Paths are relative to the reference checkout
 * (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_channel:handle_deliver/2
 *     disconnected: emqx_session:enqueue/2             apps/emqx/src/emqx_channel.erl:791-801
 *     connected:    emqx_session:deliver/2             apps/emqx/src/emqx_channel.erl:803-814
 *   emqx_session:deliver/2, deliver_msg/2, enqueue/2   apps/emqx/src/emqx_session.erl:483-536
 *   emqx_session:next_pkt_id/1 (65535 -> 1)            apps/emqx/src/emqx_session.erl:739-743
 *   emqx_inflight:is_full/1                            apps/emqx/src/emqx_inflight.erl:84-87
 *   emqx_mqueue:in/2                                   apps/emqx/src/emqx_mqueue.erl:159-179
 *
 * No ack arrives inside one handle_deliver/2 call: within a batch the window only fills and the
 * queue only takes, so the fold is a function of two per-inbox prefix counts and the session's
 * state at entry.  The stage evaluates it for every inbox of a batch at once and hands the
 * caller, per subscriber, what to put on the wire with which packet id, what to queue, what was
 * dropped and why, and the session's counters after the batch.
 *
 * Input: the inbox stage's inbox_subs[m], inbox_offsets[m+1] and box_opts[] (the options byte of
 * emqx_deliver.h, required), and a session table sessions[sub_limit] indexed by subscriber id.
 *
 * Per delivery, in inbox order, with q = box_opts & EMQX_DELIVER_QOS_MASK, a verdict byte and a
 * uint16 packet id (0 unless the verdict is EMQX_W_SEND).  The first of these that applies:
 *   EMQX_W_SKIP_NO_LOCAL   the opts byte has EMQX_DELIVER_DROP_NO_LOCAL (ignore_local runs before
 *                          the session sees the list): no state effect
 *   EMQX_W_BAD_MESSAGE     the opts byte has EMQX_DELIVER_BAD_MESSAGE: no state effect
 *   EMQX_W_NO_SESSION      the record lacks PRESENT, or the inbox's subscriber id is not below
 *                          sub_limit: no state effect
 *   EMQX_W_PASS            the record has PASS: the caller keeps this session on the host
 *                          (takeover in progress, a priority table, shared_dispatch_ack_enabled):
 *                          no state effect
 * Every other delivery is LIVE.  With a = the live deliveries with q > 0 before this one in the
 * inbox:
 *   CONNECTED (emqx_channel.erl:803-814)
 *     q = 0: EMQX_W_SEND_QOS0.
 *     q > 0: the window is full iff inflight_max != 0 && inflight_max <= inflight + a
 *            (is_full/1 on the window as the sends before this one left it).  Not full:
 *            EMQX_W_SEND with id ((next_pkt_id - 1 + a) mod 65535) + 1.  Full: a queue candidate;
 *            once full the window stays full for the rest of the inbox.
 *   not CONNECTED (emqx_channel.erl:791-801, emqx_session:enqueue/2)
 *     q = 0 without STORE_QOS0: EMQX_W_DROP_QOS0 (the first clause of emqx_mqueue:in/2; `dropped`
 *            is not counted).  Every other live delivery is a queue candidate.
 * Queue candidates follow emqx_mqueue:in/2 without a priority table.  With e the candidates of
 * the inbox, c a candidate's 0-based rank among them, L = mq_len, M = mq_max:
 *   M == 0 or L > M: every candidate is EMQX_W_QUEUED, the new length is L + e (the reference
 *     tests PLen =:= MaxLen, so a queue already over a lowered limit never drops).
 *   otherwise: the new length is min(L + e, M); v = max(0, L + e - M) evictions, dropped += v;
 *     evicted_old = min(L, v) of the messages queued before the batch fall out; the first
 *     max(0, e - M) candidates are EMQX_W_QUEUED_DROPPED (queued, then evicted as oldest within
 *     the same call), the rest EMQX_W_QUEUED; a candidate whose enqueue evicted something
 *     (c >= M - L) also carries the bit EMQX_W_EVICTS.
 * q = 3 does not occur behind the enrich stage (it reports EMQX_DELIVER_BAD_MESSAGE); here it
 * counts as q > 0.
 *
 * Per inbox: the 32-byte record after the batch (inflight += sends with id, next_pkt_id advanced
 * by that count with the 65535 -> 1 wrap, mq_len, dropped; the other fields unchanged) and
 * counts[4]: sends with id, sends QoS 0, queued and surviving, evicted_old.  An inbox that is
 * NO_SESSION or PASS gets its record unchanged (all zero for a subscriber id not below sub_limit)
 * and zero counts.  With update_table != 0 the new record of every inbox that is neither is also
 * written to sessions[inbox_subs[k]], so the next batch chains on the stream with no host read.
 * An inbox that hands out more than 65535 ids in one batch reuses ids within the batch (possible
 * only with inflight_max 0 or above 65535; the reference would crash in gb_trees:insert): the
 * verdicts stay as defined and the inbox is counted in summary[7].
 * The uint32 fields saturate at 2^32 - 1; next_pkt_id is read as (next_pkt_id - 1) mod 65535 in
 * 32-bit arithmetic, whatever it holds.
 *
 * Out of scope, kept by the caller: priority tables (p_table; mark such sessions PASS), the
 * shared-subscription ack and nack path (maybe_ack / maybe_nack, off by default), message expiry,
 * active_n slicing of an inbox, which ids are still inflight (only the count is modelled;
 * emqx_ack.h keeps the ids and takes the acks, emqx_retry.h their ages), the id-to-pid lookup and
 * the send.  The queued messages themselves and the ack-driven dequeue/1 are the mqueue stage's
 * (emqx_mqueue.h): its put call runs behind this one and stores what the verdicts queue.  A
 * session with a priority table need not be PASS any more: with mq_max = 0 in its record this call
 * marks its queue candidates EMQX_W_QUEUED and emqx_pmqueue.h applies the table behind it.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  Threading as in emqx_inbox.h: the
 * calls on one handle share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_WINDOW_H
#define EMQX_WINDOW_H

#include <stdint.h>

#include "emqx_deliver.h"
#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_window emqx_window;

#define EMQX_WINDOW_HOST_ONLY (-2) /* `device` of a handle without a device */

/* the verdict byte */
#define EMQX_W_SEND_QOS0 1u      /* send without a packet id                                    */
#define EMQX_W_SEND 2u           /* send with pkt_ids[d]; takes one inflight slot               */
#define EMQX_W_QUEUED 3u         /* in the message queue after the batch                        */
#define EMQX_W_QUEUED_DROPPED 4u /* queued, then evicted as oldest within the same batch        */
#define EMQX_W_DROP_QOS0 5u      /* QoS 0 to a disconnected session that does not store QoS 0   */
#define EMQX_W_SKIP_NO_LOCAL 6u
#define EMQX_W_BAD_MESSAGE 7u
#define EMQX_W_NO_SESSION 8u
#define EMQX_W_PASS 9u
#define EMQX_W_VERDICT_MASK 0x0Fu
#define EMQX_W_EVICTS 0x80u /* on QUEUED / QUEUED_DROPPED: this enqueue evicted the queue's oldest */

/* flags of a session record */
#define EMQX_WINDOW_PRESENT 0x1u
#define EMQX_WINDOW_CONNECTED 0x2u
#define EMQX_WINDOW_STORE_QOS0 0x4u
#define EMQX_WINDOW_PASS 0x8u

/* One session, 32 bytes.  The device forms read and write tables of these 16-byte aligned. */
typedef struct emqx_window_session {
  uint32_t inflight;     /* gb_trees:size of the inflight window at entry */
  uint32_t inflight_max; /* 0 = never full (emqx_inflight:is_full/1)      */
  uint32_t mq_len;       /* mqueue len at entry                           */
  uint32_t mq_max;       /* max_len, 0 = infinity                         */
  uint32_t next_pkt_id;  /* 1..65535                                      */
  uint32_t flags;        /* EMQX_WINDOW_*                                 */
  uint64_t dropped;      /* emqx_mqueue's dropped counter                 */
} emqx_window_session;

/* summary[8]: [0] flags, [1] deliveries (inbox_offsets[m]), [2] inboxes m, [3] sends with id,
 * [4] sends QoS 0, [5] queued and surviving, [6] drops of all kinds: the EMQX_W_DROP_QOS0 and
 * EMQX_W_QUEUED_DROPPED verdicts plus every inbox's evicted_old (the skips are not drops),
 * [7] inboxes that handed out more than 65535 ids. */
#define EMQX_WINDOW_SUMMARY_WORDS 8
#define EMQX_WINDOW_F_INPUT_REFUSED 0x2u /* inbox_offsets[m] > cap_in or >= 2^32, m > cap_boxes or >= 2^32: [1] and */
                                         /* [2] as read, nothing else written but the summary                        */
#define EMQX_WINDOW_F_BAD_SUB 0x4u       /* some inbox_subs[k] >= sub_limit: that inbox is EMQX_W_NO_SESSION, the    */
                                         /* rest are valid                                                           */

/* One call.  Every pointer is host memory for emqx_window_run_batch and emqx_window_run_host,
 * device memory for the _device forms.
 *
 * In:  inbox_subs[m] (distinct, as the inbox stage writes them; of duplicates each is evaluated
 *      against the record at entry), inbox_offsets[m + 1] with inbox_offsets[0] = 0 and no
 *      decrease, box_opts[] of capacity cap_in; sessions[sub_limit].  n_boxes NULL: the inbox
 *      count is `m`.  n_boxes not NULL: it is read from there when the call runs (the inbox
 *      stage's summary word 2) and `m` is ignored; a count above cap_boxes refuses the input.
 * Out: verdicts[] and pkt_ids[] of capacity cap_in, the first inbox_offsets[m] entries written;
 *      out_sessions[cap_boxes] and out_counts[4 * cap_boxes], the first m inboxes written.
 *      sessions[] is written only with update_table != 0.  The outputs are distinct from the
 *      inputs and from each other. */
typedef struct emqx_window_batch {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  uint8_t* verdicts;
  uint16_t* pkt_ids;
  emqx_window_session* out_sessions;
  uint32_t* out_counts;
} emqx_window_batch;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_window_stats) before the call. */
typedef struct emqx_window_stats {
  uint64_t size;          /* in: sizeof(emqx_window_stats) of the caller; out: bytes written */
  uint64_t cap_in;        /* deliveries the reserved scratch takes                           */
  uint64_t cap_boxes;     /* inboxes it takes                                                */
  uint64_t scratch_bytes; /* device memory held                                              */
  uint64_t path;          /* tuning key "path"                                               */
  uint64_t calls;         /* calls so far, all forms                                         */
  double last_call_ms;    /* time of the last synchronous call                               */
} emqx_window_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_WINDOW_HOST_ONLY: a handle that answers
 * emqx_window_run_host alone; its batch entry points return EMQX_EDEVICE (nothing ever falls
 * back to the host silently). */
int emqx_window_create(int32_t device, emqx_window** out);
int emqx_window_destroy(emqx_window* h);

/* Sizes the device scratch for calls of up to cap_in deliveries and cap_boxes inboxes (both
 * < 2^32).  It only grows; it waits for the handle's call in flight first. */
int emqx_window_reserve(emqx_window* h, uint64_t cap_in, uint64_t cap_boxes);

/* Host buffers, evaluated on the device: the m records the inboxes name travel, not the table
 * (n_boxes must be NULL).  EMQX_EINVAL: inbox_offsets[0] != 0, decreasing offsets, a refused
 * input, a subscriber >= sub_limit (the outputs are still complete).  summary_out (host, may be
 * NULL) receives the 8 summary words. */
int emqx_window_run_batch(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out);
/* Device buffers, on `stream` (NULL: the handle's own, ordered after the device's null stream);
 * synchronizes the stream.  The counts are read on the device.  The scratch grows as needed.
 * Returns as above. */
int emqx_window_run_batch_device(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out, void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains behind
 * emqx_inbox_group_batch_device_async on the same stream with no host read.  `summary` (>= 8
 * uint64_t, device or host-pinned memory) is written last, with plain stores.  Whatever the
 * device buffers hold, no access leaves them (offsets that decrease give unspecified verdicts
 * inside the buffers).  EMQX_EOVERFLOW, nothing enqueued: the reserved scratch
 * (emqx_window_reserve) is smaller than cap_in or cap_boxes.  Everything else is reported
 * through the summary alone. */
int emqx_window_run_batch_device_async(emqx_window* h, const emqx_window_batch* b, uint64_t* summary, void* stream);
/* The same bytes computed on the calling thread: the per-call path and the checker of the batch
 * path.  Returns as emqx_window_run_batch. */
int emqx_window_run_host(emqx_window* h, const emqx_window_batch* b, uint64_t* summary_out);

/* Keys: "path": 0 the tile scan (default), 1 one wave per inbox (the yardstick: its time grows with
 * the longest inbox; both produce the same bytes); "max_blocks" (1..2048, default 2048): the grid
 * cap of every pass whose blocks stride (the heads, the verdicts, the write-back and path 1's wave
 * kernel), the blocks stride over the tiles or inboxes beyond it; at 2048 the wave kernel keeps its
 * own cap of 16384; "scan_chunk" (1..1024, default 1024): the tile totals the one-block scan takes
 * per carry step (tests lower both to make the blocks stride and the scan carry at small shapes;
 * the same bytes at every value).  Both are read when a call is enqueued; a host-only handle
 * accepts and ignores them.  EMQX_EINVAL out of range, EMQX_ENOTFOUND for unknown keys. */
int emqx_window_set_tuning(emqx_window* h, const char* key, int64_t value);
int emqx_window_stats_get(emqx_window* h, emqx_window_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_WINDOW_H */
