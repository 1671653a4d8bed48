/*
 * emqx_mqueue.h — C ABI of the mqueue stage (libemqxmatch.so): the queued messages of every session
 * and the two operations of the reference that touch them, emqx_mqueue:in/2 for what the window
 * stage queued and emqx_session:dequeue/1 for what an ack made room for.  The step behind the window
 * stage (emqx_window.h), which decides what is queued but stores nothing, and behind the ack stage
 * (emqx_ack.h), which reopens the window.
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_mqueue:in/2, out/1 without a priority table   apps/emqx/src/emqx_mqueue.erl:159-202
 *   emqx_session:dequeue/1, dequeue/3, acc_cnt/2       apps/emqx/src/emqx_session.erl:453-477
 *   deliver/3, deliver_msg/2, enqueue/2                apps/emqx/src/emqx_session.erl:493-536
 *   batch_n/1, next_pkt_id/1                           apps/emqx/src/emqx_session.erl:783-787, :739-743
 *   replay/1 (its tail)                                apps/emqx/src/emqx_session.erl:692-703
 *   emqx_message:is_expired/1                          apps/emqx/src/emqx_message.erl:239-243
 *   the known answers                                  apps/emqx/test/emqx_mqueue_SUITE.erl,
 *                                                      apps/emqx/test/emqx_session_SUITE.erl
 *
 * State: two tables of the caller's, next to sessions[], slots[] and stamps[].
 *   ring[sub_limit * Q] of emqx_mqueue_entry {ref, opts}: `opts` is the delivery's box_opts byte (its
 *     QoS is opts & EMQX_DELIVER_QOS_MASK), `ref` the caller's name of the message as in emqx_ack.h.
 *     Q is a field of every call: a power of two, 8 <= Q <= 1024, else EMQX_EINVAL.  A row is 16-byte
 *     aligned.
 *   heads[sub_limit] of emqx_mqueue_ring {head, len}: the queue of session `sub`, oldest first, is
 *     ring[sub * Q + (head + i) % Q] for i < len.  A header with head >= Q or len > Q is read as
 *     head % Q and min(len, Q) and sets EMQX_MQ_F_BAD_RING.
 * The caller chooses Q >= mq_max; a session whose queue a row cannot hold (mq_max 0: unbounded, or
 * mq_max > Q) is the caller's to mark EMQX_WINDOW_PASS, the rule emqx_ack.h has for W.  The ring is
 * never cleared: a call writes only the positions it fills, so every form leaves the same bytes in
 * the whole table.
 *
 * Call 1, emqx_mqueue_put_*: emqx_mqueue:in/2 for a batch, behind emqx_window_run_* on the stream,
 * with that call's inbox_subs, inbox_offsets, n_boxes / m, cap_in, cap_boxes and box_opts, its output
 * verdicts[] and optionally refs[] (NULL: the position d names the message).  It reads the verdicts
 * only and neither reads nor writes the window's counters: the window already counted.  Per inbox k
 * with the row (h, L) at entry:
 *     s  = its deliveries with verdict EMQX_W_QUEUED           (verdict & EMQX_W_VERDICT_MASK)
 *     x  = its deliveries that carry EMQX_W_EVICTS
 *     qd = its deliveries with verdict EMQX_W_QUEUED_DROPPED
 *     ev = min(L, x - qd)  (0 when qd > x)                     the old entries evicted
 * the head becomes (h + ev) % Q, the r-th QUEUED delivery of the inbox (by order alone, r from 0) is
 * stored at logical index L - ev + r of the new queue, len becomes L - ev + s.  Survivors that would
 * make len exceed Q are not stored: out_unstored[k] counts them, EMQX_MQ_F_ROW_FULL is set and len
 * stays Q.  out_evicted[cap_in] has one entry per delivery position: the j-th EVICTS delivery of the
 * inbox with j < L gets the old entry at logical index j (the message the reference returns as
 * DroppedMsg; the caller releases it), every other position {EMQX_MQ_NO_REF, 0}.  An inbox whose
 * subscriber id is not below sub_limit stores nothing: all its survivors are unstored and
 * EMQX_MQ_F_BAD_SUB is set.  When sessions is not NULL the call checks one thing: an inbox whose new
 * len differs from sessions[sub].mq_len is counted (summary word 7) and sets
 * EMQX_MQ_F_LEN_MISMATCH.  inbox_subs are distinct.
 *
 * Call 2, emqx_mqueue_take_*: dequeue/1 of the m sessions subs[] names (distinct; NULL: the sessions
 * 0..m-1, m <= sub_limit, a sweep of the whole table, on mass resume for instance) at now_ms.  In
 * practice subs is the ack run call's ack_subs on the same stream, after emqx_ack_run_* with
 * update_table lowered `inflight`.  out_status[k] is EMQX_A_OK, EMQX_A_NO_SESSION (the record lacks
 * PRESENT, or the id is not below sub_limit, which also sets EMQX_MQ_F_BAD_SUB) or EMQX_A_PASS; the
 * latter two touch nothing and have no items.  For an OK session the budget is batch_n/1:
 * n = 1000 when inflight_max is 0, else inflight_max - inflight saturating at 0.  Entry i of the queue
 * (from the head) is EXPIRED iff deadlines != NULL, ref < ref_limit and now_ms > deadlines[ref]
 * (EMQX_RETRY_NO_EXPIRY never passes; a consumed entry with ref >= ref_limit never expires and sets
 * EMQX_MQ_F_BAD_REF), and COUNTING iff it is not expired and its QoS is above 0; c_i is the number
 * of counting entries among 0..i.  The fold of dequeue/3 in closed form:
 *     n == 0            nothing is consumed, whatever the head is (dequeue(0, ..) returns at once)
 *     else              the consumed prefix ends at the first i with c_i == n; QoS-0 entries behind
 *                       it stay queued; when there is no such i the whole queue is consumed.
 * The items are the consumed entries in order, in the layout of the window stage's outputs:
 * out_offsets[m + 1], out_opts[], out_refs[], out_pkt_ids[] and out_verdicts[] with
 *     EMQX_W_SEND_QOS0   a live QoS-0 entry (pkt id 0)
 *     EMQX_W_SEND        a counting entry, id ((next_pkt_id - 1 + a) mod 65535) + 1 with a the
 *                        counting entries before it
 *     EMQX_MQ_EXPIRED    an expired one (pkt id 0), listed so that the caller can release the message
 * deliver/3 never re-queues here: at most `room` counting messages are popped, so every one finds a
 * free inflight slot.  out_counts[4 * k] = sends with id, sends QoS 0, expired, mq_len after.  With
 * update_table != 0, heads[sub] advances (and is normalised), sessions[sub].mq_len becomes the ring's
 * len after the call (a record whose mq_len differed from the ring's len at entry is counted in
 * summary word 7 and sets EMQX_MQ_F_LEN_MISMATCH), inflight grows by the sends with id, next_pkt_id
 * advances with the 65535 -> 1 wrap; `dropped` is unchanged (expiry is a metric, not a queue drop).
 *
 * Overflow: when the items of all sessions exceed cap_out the call sets EMQX_MQ_F_OUTPUT_FULL;
 * out_offsets, out_counts and out_status are complete, the items, heads and the table are UNTOUCHED,
 * and summary word 3 is the cap_out the call needs.
 *
 * The take call's outputs are inputs of the stages that exist: out_offsets serves as inbox_offsets,
 * subs as inbox_subs, out_opts / out_verdicts / out_pkt_ids / out_refs as the record call's box_opts /
 * verdicts / pkt_ids / refs, so emqx_ack_record_batch_device_async and emqx_retry_stamp_* take them
 * unchanged and  run -> stamp -> take -> record -> stamp  runs on one stream with no host read.
 *
 * No thread walks an inbox or a queue: put ranks deliveries by a global prefix count, take is a
 * segmented prefix count over a row's lanes (emqx_amd/csrc/mqueue.h).
 *
 * Out of scope, kept by the caller: priority tables and shift_opts (such sessions are marked PASS),
 * awaiting_rel and the inbound QoS 2 path, log_dropped and the metrics, active_n, a NIF binding.
 * The priority mqueue stage (emqx_pmqueue.h) serves sessions with a priority table in place of this
 * one's two calls, so they need not be PASS.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  Threading as in emqx_ack.h: the calls
 * on one handle share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_MQUEUE_H
#define EMQX_MQUEUE_H

#include <stdint.h>

#include "emqx_ack.h"
#include "emqx_deliver.h"
#include "emqx_match.h"
#include "emqx_retry.h"
#include "emqx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_mqueue emqx_mqueue;

#define EMQX_MQUEUE_HOST_ONLY (-2) /* `device` of a handle without a device */

#define EMQX_MQ_MIN_Q 8u
#define EMQX_MQ_MAX_Q 1024u
#define EMQX_MQ_NO_REF 0xFFFFFFFFu /* out_evicted: this delivery evicted no old entry        */
#define EMQX_MQ_EXPIRED 10u        /* out_verdicts of a take: expired, release the message    */

/* One queued message, 8 bytes. */
typedef struct emqx_mqueue_entry {
  uint32_t ref;
  uint8_t opts;
  uint8_t rsv[3]; /* written 0 */
} emqx_mqueue_entry;

/* The header of a row, 8 bytes. */
typedef struct emqx_mqueue_ring {
  uint32_t head;
  uint32_t len;
} emqx_mqueue_ring;

/* summary[8] of a put call: [0] flags, [1] deliveries inbox_offsets[m], [2] inboxes m, [3] entries
 * stored, [4] old entries evicted, [5] survivors unstored, [6] rows that overflowed Q, [7] inboxes
 * whose new len differs from sessions[].mq_len.
 * summary[8] of a take call: [0] flags, [1] sessions with status EMQX_A_OK, [2] sessions m, [3] items
 * (with EMQX_MQ_F_OUTPUT_FULL: the cap_out the call needs), [4] sends with id, [5] sends QoS 0,
 * [6] expired, [7] sessions whose mq_len differed from the ring's len at entry. */
#define EMQX_MQ_SUMMARY_WORDS 8
#define EMQX_MQ_F_INPUT_REFUSED 0x2u /* inbox_offsets[m] > cap_in or >= 2^32, m > cap_boxes or >= 2^32, or subs NULL */
                                     /* and m > sub_limit: [1], [2] as read, nothing else written but the summary    */
#define EMQX_MQ_F_BAD_SUB 0x4u       /* some subscriber id >= sub_limit: put stores nothing of it, take: NO_SESSION  */
#define EMQX_MQ_F_OUTPUT_FULL 0x8u   /* take: more items than cap_out; see "Overflow"                                */
#define EMQX_MQ_F_BAD_REF 0x10u      /* take: a consumed entry's ref >= ref_limit; it does not expire                */
#define EMQX_MQ_F_BAD_RING 0x20u     /* a header with head >= Q or len > Q was read as head % Q, min(len, Q)         */
#define EMQX_MQ_F_ROW_FULL 0x40u     /* put: survivors beyond Q were not stored (out_unstored)                       */
#define EMQX_MQ_F_LEN_MISMATCH 0x80u /* sessions[].mq_len and the ring's len disagree                                */

/* One put call.  Every pointer is host memory for emqx_mqueue_put_batch and emqx_mqueue_put_host,
 * device memory for the _device forms.
 * In:  the window call's inbox_subs[m], inbox_offsets[m + 1], box_opts[cap_in], verdicts[cap_in];
 *      n_boxes NULL: the inbox count is `m`, else it is read from there when the call runs; refs[cap_in]
 *      or NULL; sessions[sub_limit] or NULL (read only).
 * Out: ring[sub_limit * q] and heads[sub_limit] in place; out_evicted[cap_in] and
 *      out_unstored[cap_boxes], the first inbox_offsets[m] and m written. */
typedef struct emqx_mqueue_put_args {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  const uint8_t* verdicts;
  const uint32_t* refs;
  const emqx_window_session* sessions;
  emqx_mqueue_entry* ring;
  emqx_mqueue_ring* heads;
  uint64_t q;
  uint64_t sub_limit;
  emqx_mqueue_entry* out_evicted;
  uint32_t* out_unstored;
} emqx_mqueue_put_args;

/* One take call.
 * In:  subs[m] (distinct; NULL: 0..m-1), n_boxes, m, cap_boxes as above; sessions[sub_limit]
 *      (required); ring, heads, q; now_ms (< 2^45); deadlines[ref_limit] or NULL; cap_out.
 * Out: out_offsets[cap_boxes + 1], out_opts / out_verdicts / out_pkt_ids / out_refs [cap_out],
 *      out_status[cap_boxes], out_counts[4 * cap_boxes] (16-byte aligned), the first m (m + 1)
 *      written; with update_table != 0 heads[] and sessions[].  The outputs are distinct from the
 *      inputs and from each other. */
typedef struct emqx_mqueue_take_args {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_boxes;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  const emqx_mqueue_entry* ring;
  emqx_mqueue_ring* heads;
  uint64_t q;
  uint64_t now_ms;
  const uint64_t* deadlines;
  uint64_t ref_limit;
  uint64_t cap_out;
  uint64_t* out_offsets;
  uint8_t* out_opts;
  uint8_t* out_verdicts;
  uint16_t* out_pkt_ids;
  uint32_t* out_refs;
  uint8_t* out_status;
  uint32_t* out_counts;
} emqx_mqueue_take_args;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_mqueue_stats) before the call. */
typedef struct emqx_mqueue_stats {
  uint64_t size;          /* in: sizeof(emqx_mqueue_stats) of the caller; out: bytes written */
  uint64_t cap_in;        /* deliveries the reserved scratch takes                            */
  uint64_t cap_boxes;     /* inboxes or sessions it takes                                     */
  uint64_t scratch_bytes; /* device memory held                                               */
  uint64_t calls;         /* calls so far, all forms                                          */
  double last_call_ms;    /* time of the last synchronous call                                */
} emqx_mqueue_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_MQUEUE_HOST_ONLY: a handle that answers
 * the _host calls alone; its batch entry points return EMQX_EDEVICE (nothing ever falls back to
 * the host silently). */
int emqx_mqueue_create(int32_t device, emqx_mqueue** out);
int emqx_mqueue_destroy(emqx_mqueue* h);

/* Sizes the device scratch for calls of up to cap_in deliveries and cap_boxes inboxes or sessions
 * (both < 2^32).  It only grows; it waits for the handle's call in flight first. */
int emqx_mqueue_reserve(emqx_mqueue* h, uint64_t cap_in, uint64_t cap_boxes);

/* The four forms of each call, as in emqx_ack.h.
 *   host buffers, evaluated on the device: the rows, headers and records the call names travel, not
 *     the tables (deadlines[] travels whole; n_boxes must be NULL).
 *   _device: device buffers on `stream` (NULL: the handle's own, ordered after the device's null
 *     stream); synchronizes the stream; the scratch grows as needed.
 *   _device_async: enqueues kernels only and returns at once; every count is read on the device;
 *     `summary` (>= 8 uint64_t, device or host-pinned memory) is written last, with plain stores.
 *     Whatever the device buffers hold, no access leaves them.  EMQX_EOVERFLOW, nothing enqueued:
 *     the reserved scratch is smaller than cap_in or cap_boxes.
 *   _host: the same bytes computed on the calling thread.
 * The synchronous forms return EMQX_EINVAL for a bad argument (q, now_ms >= 2^45, a missing buffer),
 * a refused input or a subscriber >= sub_limit (the outputs are still complete), and EMQX_EOVERFLOW
 * for EMQX_MQ_F_OUTPUT_FULL; the other flags are reported in the summary alone.
 * summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_mqueue_put_batch(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out);
int emqx_mqueue_put_batch_device(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out, void* stream);
int emqx_mqueue_put_batch_device_async(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary, void* stream);
int emqx_mqueue_put_host(emqx_mqueue* h, const emqx_mqueue_put_args* b, uint64_t* summary_out);

int emqx_mqueue_take_batch(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out);
int emqx_mqueue_take_batch_device(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out, void* stream);
int emqx_mqueue_take_batch_device_async(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary, void* stream);
int emqx_mqueue_take_host(emqx_mqueue* h, const emqx_mqueue_take_args* b, uint64_t* summary_out);

/* Keys: "max_blocks" (1..4096, default 4096): the grid cap of every pass, the blocks stride beyond
 * it; "scan_chunk" (1..1024, default 1024): the totals a one-block scan takes per carry step (tests
 * lower both to make the blocks stride and the scans carry at small shapes; the same bytes at every
 * value).  Both are read when a call is enqueued; a host-only handle accepts and ignores them.
 * EMQX_EINVAL out of range, EMQX_ENOTFOUND for unknown keys. */
int emqx_mqueue_set_tuning(emqx_mqueue* h, const char* key, int64_t value);
int emqx_mqueue_stats_get(emqx_mqueue* h, emqx_mqueue_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_MQUEUE_H */
