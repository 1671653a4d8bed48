/*
 * emqx_pmqueue.h — C ABI of the priority mqueue stage (libemqxmatch.so): the queued messages of the
 * sessions whose zone sets mqueue_priorities, and the two operations of the reference that touch
 * them, emqx_mqueue:in/2 and emqx_session:dequeue/1 over emqx_mqueue:out/1, with a p_table and
 * shift_opts.  It stands where emqx_mqueue.h stands for sessions without a priority table: behind the
 * window stage (emqx_window.h) and behind the ack stage (emqx_ack.h).  Window, record, stamp, ack run,
 * retry and rel serve these sessions unchanged; only the two queue calls are this stage's.
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_mqueue:in/2, out/1, get_credits/2, get_shift_opt/1   apps/emqx/src/emqx_mqueue.erl:159-254
 *   emqx_pqueue:plen/2, in/3, out/1, out/2, shift/1, out_p/1  apps/emqx/src/emqx_pqueue.erl:98-211
 *   emqx_session:dequeue/1, dequeue/3, enqueue/2              apps/emqx/src/emqx_session.erl:453-477, :523-536
 *   what a running broker passes as options                   apps/emqx/src/emqx_cm.erl:309-314
 *   the known answers                                         apps/emqx/test/emqx_mqueue_SUITE.erl
 *
 * What the reference does.  The priority of a message is an exact lookup of its topic name in the
 * p_table, else the default priority (0, or `infinity`).  The queue is a LIST of {-P, queue} in list
 * order.  in/2 compares the length of the message's OWN priority with max_len and evicts the oldest
 * message of that priority; the total can reach classes * max_len.  A priority that is not in the list
 * is inserted by a keysort of the whole list, except that the key `infinity` is pushed at the head
 * without a sort and a head element `infinity` is held in place while the rest is sorted; a non-head
 * `infinity` sorts LAST (an atom is above every number).  out/1 takes from the head element and
 * deletes it when it empties:
 *     len == 0                     empty; nothing is reset
 *     last_prio undefined          take from the head class P; last_prio = P,
 *                                  p_credit = (P + base + 1) * mult - 1   (infinity counts as 1 000 000)
 *     p_credit == 0                shift (Rest ++ [Hd]), last_prio = undefined, go round again
 *     else                         take from the head, whatever class that now is; p_credit - 1
 * The credit is signed: a negative priority with base 0 (what a running broker has: get_shift_opt looks
 * for the key p_table, emqx_cm passes `priorities`) gives a negative credit, which never reaches 0, so
 * the list never shifts again.  Every negative value behaves alike; the stage stores -1 for all of them.
 *
 * State: three tables of the caller's, next to sessions[].
 *   tables[n_tables] of emqx_pmqueue_table, one a zone configuration: n_classes (1..8), prio[] strictly
 *     descending (class index ascending is priority descending; EMQX_PMQ_PRIO_INFINITY only as
 *     prio[0]; every other |prio| <= EMQX_PMQ_MAX_PRIO), default_class (< n_classes), max_len, mult
 *     (1..EMQX_PMQ_MAX_MULT), base (0..EMQX_PMQ_MAX_PRIO).  A table is UNFIT when any of that does not
 *     hold, when max_len is 0, 1 or above Qc, or when n_classes is above C: the sessions of an unfit
 *     table (and those whose head names a table not below n_tables) get status EMQX_PMQ_UNFIT, are
 *     left untouched and set EMQX_PMQ_F_UNFIT; they are the caller's, as before this stage.
 *   ring[sub_limit * C * Qc] of emqx_mqueue_entry (emqx_mqueue.h): class c of session `sub` is the ring
 *     at (sub * C + c) * Qc.  C (1..8) and Qc (a power of two, 8..128) are fields of every call.  The
 *     ring is never cleared: a call writes only the positions it fills.
 *   heads[sub_limit] of emqx_pmqueue_head, 64 bytes, 64-byte aligned:
 *     head[c], len[c]   the queue of class c, oldest first, is ring[.. + (head[c] + i) % Qc], i < len[c]
 *     order             the list of the non-empty classes, position p in bits 4p..4p+3, 0xF behind
 *                       the last one
 *     credit            p_credit, signed; flags bit 0 (EMQX_PMQ_H_LAST_DEFINED): last_prio is defined
 *     table             which of tables[] the session belongs to
 *   A malformed head is NORMALISED and sets EMQX_PMQ_F_BAD_HEAD: head[c] is read as head[c] % Qc,
 *   len[c] as min(len[c], Qc) and as 0 for c >= n_classes; when `order` is not exactly a list of the
 *   classes with len > 0, each once, it is read as those classes in ascending index (the sorted
 *   list); a credit below -1 is read as -1.  With update_table the normalised head is what is written.
 *
 * The window record of a session this stage owns carries mq_max = 0: the unchanged window stage then
 * marks every queue candidate EMQX_W_QUEUED and evicts nothing, and the session is NOT marked
 * EMQX_WINDOW_PASS.  THIS STAGE IS THE AUTHORITY for sessions[].mq_len (the sum of the class lengths)
 * and sessions[].dropped (one per eviction), and writes both with update_table, over what the window
 * call left there.  A record with mq_max != 0 sets EMQX_PMQ_F_LIMITED and is served all the same.
 *
 * Call 1, emqx_pmqueue_put_*: in/2 for a batch, behind emqx_window_run_* on the stream, with that
 * call's inbox_subs, inbox_offsets, n_boxes / m, cap_in, cap_boxes, box_opts and verdicts, refs[] or
 * NULL (the position names the message), box_src[] (the message index of each delivery, the inbox
 * stage's output) and msg_class[n_msgs * n_tables] (uint8: the caller resolved topic -> class per
 * table).  The class of delivery d of a session of table t is msg_class[box_src[d] * n_tables + t]; a
 * value not below the table's n_classes means its default_class; box_src[d] >= n_msgs also means the
 * default and sets EMQX_PMQ_F_BAD_SRC.  The candidates are the deliveries with verdict EMQX_W_QUEUED;
 * a QUEUED_DROPPED verdict or an EVICTS bit means the record had a limit: the delivery is ignored
 * and sets EMQX_PMQ_F_BAD_VERDICT.  Per class c of an inbox with e candidates, L = len[c], M = max_len:
 *     L > M    nothing is evicted; the candidates are appended while the ring has room, the others
 *              are counted unstored and set EMQX_PMQ_F_ROW_FULL
 *     else     v = max(0, L + e - M) evictions; the first qd = max(0, e - M) candidates are queued and
 *              then dropped; a candidate of in-class rank r >= M - L evicts; min(L, v) old entries
 *              leave from the class's head
 * out_verdicts[d]: EMQX_W_QUEUED or EMQX_W_QUEUED_DROPPED, with EMQX_W_EVICTS, 0 for a non-candidate;
 * out_class[d]: the class (0xFF for a non-candidate); out_evicted[d]: the old entry the enqueue dropped,
 * else {EMQX_MQ_NO_REF, 0}.  out_counts[8 * k] of inbox k: stored, evicted old, dropped in batch,
 * unstored, mq_len after, dropped after (low, high word), status (EMQX_A_OK, EMQX_A_NO_SESSION,
 * EMQX_A_PASS or EMQX_PMQ_UNFIT; the latter three touch nothing, their deliveries get verdict 0).
 * The order list after the call follows from the activations of the inbox, the first candidate of each
 * class with len 0 at entry, in arrival order: activating the `infinity` class pushes it at the head;
 * any other class: a head `infinity` stays and the rest with the new class is sorted, otherwise the whole
 * list is sorted with `infinity` last.  last_prio and the credit are not touched.  The ring and the
 * outputs are always written; heads[] and sessions[] with update_table != 0.  inbox_subs are distinct.
 *
 * Call 2, emqx_pmqueue_take_*: dequeue/1 of the m sessions subs[] names (distinct; NULL: 0..m-1) at
 * now_ms.  Budget (batch_n/1), expiry (deadlines[ref], ref_limit, EMQX_PMQ_F_BAD_REF), the statuses,
 * the overflow protocol (EMQX_PMQ_F_OUTPUT_FULL: offsets, counts and status complete, items, heads
 * and records untouched, summary word 3 the cap_out the call needs) and the output layout are those
 * of emqx_mqueue_take_* (emqx_mqueue.h), plus EMQX_PMQ_UNFIT and out_class[] per item: the record and
 * stamp calls take the outputs unchanged.  The items are the fold of out/1 above: an expired message is
 * dropped for free, a QoS 0 one is delivered for free, any other costs one unit of the budget; the
 * fold stops at budget 0 or when the queue is empty.  With update_table the call writes heads[] (the
 * class heads and lengths, the order, the credit, last_prio) and sessions[] (inflight, next_pkt_id
 * with the 65535 -> 1 wrap, mq_len).
 *
 * Not here: max_len 0 and 1 and more than 8 classes (unfit), the topic -> priority lookup itself,
 * log_dropped and the metrics, active_n, takeover, a NIF binding.
 *
 * inbox_offsets[0] is 0 and the offsets do not decrease, as the inbox stage writes them; for other
 * offsets no access leaves the buffers, but the forms need not leave the same bytes.
 *
 * Conventions as in emqx_mqueue.h: int status, EMQX_* codes, opaque handles, the calls on one handle
 * share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_PMQUEUE_H
#define EMQX_PMQUEUE_H

#include <stdint.h>

#include "emqx_mqueue.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_pmqueue emqx_pmqueue;

#define EMQX_PMQUEUE_HOST_ONLY (-2) /* `device` of a handle without a device */

#define EMQX_PMQ_MAX_CLASSES 8u
#define EMQX_PMQ_MIN_QC 8u
#define EMQX_PMQ_MAX_QC 128u
#define EMQX_PMQ_PRIO_INFINITY 0x7FFFFFFF /* prio[0] alone: the atom `infinity`                    */
#define EMQX_PMQ_MAX_PRIO 1000000         /* |prio| and base at most; what `infinity` counts as    */
#define EMQX_PMQ_MAX_MULT 1024u
#define EMQX_PMQ_NO_CLASS 0xFFu    /* out_class of a non-candidate; msg_class: the default class  */
#define EMQX_PMQ_UNFIT 7u          /* status: the session's table is unfit; nothing was touched   */
#define EMQX_PMQ_H_LAST_DEFINED 1u /* emqx_pmqueue_head.flags: last_prio is defined               */

/* One zone configuration, 56 bytes. */
typedef struct emqx_pmqueue_table {
  uint32_t n_classes;
  uint32_t default_class;
  uint32_t max_len;
  uint32_t mult;
  uint32_t base;
  uint32_t rsv; /* 0 */
  int32_t prio[8];
} emqx_pmqueue_table;

/* The queue state of one session, 64 bytes. */
typedef struct emqx_pmqueue_head {
  uint16_t head[8];
  uint16_t len[8];
  uint32_t order;
  int32_t credit;
  uint32_t flags;
  uint32_t table;
  uint32_t rsv[4]; /* written as read */
} emqx_pmqueue_head;

/* summary[8] of a put call: [0] flags, [1] deliveries inbox_offsets[m], [2] inboxes m, [3] entries
 * stored, [4] old entries evicted, [5] candidates dropped in batch, [6] candidates unstored, [7] inboxes
 * with status EMQX_A_OK.
 * summary[8] of a take call: [0] flags, [1] sessions with status EMQX_A_OK, [2] sessions m, [3] items
 * (with EMQX_PMQ_F_OUTPUT_FULL: the cap_out the call needs), [4] sends with id, [5] sends QoS 0,
 * [6] expired, [7] sessions with status EMQX_PMQ_UNFIT. */
#define EMQX_PMQ_SUMMARY_WORDS 8
#define EMQX_PMQ_F_INPUT_REFUSED 0x2u  /* as EMQX_MQ_F_INPUT_REFUSED: nothing written but the summary          */
#define EMQX_PMQ_F_BAD_SUB 0x4u        /* some subscriber id >= sub_limit: EMQX_A_NO_SESSION                   */
#define EMQX_PMQ_F_OUTPUT_FULL 0x8u    /* take: more items than cap_out                                        */
#define EMQX_PMQ_F_BAD_REF 0x10u       /* take: a consumed entry's ref >= ref_limit; it does not expire        */
#define EMQX_PMQ_F_BAD_HEAD 0x20u      /* a malformed head was normalised                                      */
#define EMQX_PMQ_F_ROW_FULL 0x40u      /* put: candidates beyond Qc were not stored                            */
#define EMQX_PMQ_F_UNFIT 0x80u         /* some session has status EMQX_PMQ_UNFIT                               */
#define EMQX_PMQ_F_BAD_VERDICT 0x100u  /* put: a QUEUED_DROPPED verdict or an EVICTS bit was ignored           */
#define EMQX_PMQ_F_BAD_SRC 0x200u      /* put: box_src[d] >= n_msgs took the default class                     */
#define EMQX_PMQ_F_LIMITED 0x400u      /* a served record has mq_max != 0                                      */

/* One put call.  Every pointer is host memory for emqx_pmqueue_put_batch and emqx_pmqueue_put_host,
 * device memory for the _device forms.
 * In:  the window call's inbox_subs[m], inbox_offsets[m + 1], box_opts[cap_in], verdicts[cap_in];
 *      n_boxes NULL: the inbox count is `m`, else it is read from there when the call runs; refs[cap_in]
 *      or NULL; box_src[cap_in]; msg_class[n_msgs * n_tables]; tables[n_tables]; sessions[sub_limit].
 * Out: ring and heads in place, sessions[] (mq_len, dropped) with update_table; out_verdicts[cap_in],
 *      out_class[cap_in], out_evicted[cap_in], out_counts[8 * cap_boxes] (16-byte aligned). */
typedef struct emqx_pmqueue_put_args {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  const uint8_t* verdicts;
  const uint32_t* refs;
  const uint32_t* box_src;
  const uint8_t* msg_class;
  uint64_t n_msgs;
  const emqx_pmqueue_table* tables;
  uint64_t n_tables;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  emqx_mqueue_entry* ring;
  emqx_pmqueue_head* heads;
  uint64_t c;
  uint64_t qc;
  uint8_t* out_verdicts;
  uint8_t* out_class;
  emqx_mqueue_entry* out_evicted;
  uint32_t* out_counts;
} emqx_pmqueue_put_args;

/* One take call: emqx_mqueue_take_args with the tables, C, Qc and out_class[cap_out]. */
typedef struct emqx_pmqueue_take_args {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_boxes;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  const emqx_pmqueue_table* tables;
  uint64_t n_tables;
  const emqx_mqueue_entry* ring;
  emqx_pmqueue_head* heads;
  uint64_t c;
  uint64_t qc;
  uint64_t now_ms;
  const uint64_t* deadlines;
  uint64_t ref_limit;
  uint64_t cap_out;
  uint64_t* out_offsets;
  uint8_t* out_opts;
  uint8_t* out_verdicts;
  uint16_t* out_pkt_ids;
  uint32_t* out_refs;
  uint8_t* out_class;
  uint8_t* out_status;
  uint32_t* out_counts;
} emqx_pmqueue_take_args;

/* Versioned by size, as emqx_mqueue_stats. */
typedef struct emqx_pmqueue_stats {
  uint64_t size;          /* in: sizeof(emqx_pmqueue_stats) of the caller; out: bytes written */
  uint64_t cap_in;        /* as reserved; kept for parity with emqx_mqueue_stats: no scratch depends on it */
  uint64_t cap_boxes;     /* inboxes or sessions it takes                                     */
  uint64_t scratch_bytes; /* device memory held                                               */
  uint64_t group;         /* tuning key "group"                                               */
  uint64_t calls;         /* calls so far, all forms                                          */
  double last_call_ms;    /* time of the last synchronous call                                */
} emqx_pmqueue_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_PMQUEUE_HOST_ONLY: a handle that answers
 * the _host calls alone; its device entry points return EMQX_EDEVICE (nothing ever falls back to
 * the host silently). */
int emqx_pmqueue_create(int32_t device, emqx_pmqueue** out);
int emqx_pmqueue_destroy(emqx_pmqueue* h);
int emqx_pmqueue_reserve(emqx_pmqueue* h, uint64_t cap_in, uint64_t cap_boxes);

/* The four forms of each call, as in emqx_mqueue.h:
 *   host buffers, evaluated on the device (emqx_pmqueue_put_batch, _take_batch): the rings, heads
 *     and records of the sessions the call names travel, not the tables (tables[], msg_class[] and
 *     deadlines[] travel whole; n_boxes must be NULL).
 *   _device: device buffers on `stream` (NULL: the handle's own, ordered after the device's null
 *     stream); synchronizes the stream; the scratch grows as needed.
 *   _device_async: enqueues kernels only and returns at once; every count is read on the device;
 *     `summary` (>= 8 uint64_t, device or host-pinned memory) is written last, with plain stores.
 *     Whatever the device buffers hold, no access leaves them.  EMQX_EOVERFLOW, nothing enqueued:
 *     the reserved scratch is smaller than cap_boxes.
 *   _host: the same bytes computed on the calling thread.
 * The synchronous forms return EMQX_EINVAL for a bad argument (c, qc, now_ms >= 2^45, a missing
 * buffer), a refused input or a subscriber >= sub_limit (the outputs are still complete), and
 * EMQX_EOVERFLOW for EMQX_PMQ_F_OUTPUT_FULL; the other flags are reported in the summary alone. */
int emqx_pmqueue_put_batch(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out);
int emqx_pmqueue_put_batch_device(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out, void* stream);
int emqx_pmqueue_put_batch_device_async(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary, void* stream);
int emqx_pmqueue_put_host(emqx_pmqueue* h, const emqx_pmqueue_put_args* b, uint64_t* summary_out);

int emqx_pmqueue_take_batch(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out);
int emqx_pmqueue_take_batch_device(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out, void* stream);
int emqx_pmqueue_take_batch_device_async(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary, void* stream);
int emqx_pmqueue_take_host(emqx_pmqueue* h, const emqx_pmqueue_take_args* b, uint64_t* summary_out);

/* Keys: "max_blocks" (1..4096, default 4096) and "scan_chunk" (1..1024, default 1024) as in
 * emqx_mqueue.h; "group" (4, 8, 16, 32 or 64): the lanes that own an inbox (put) or a session (take); the
 * same bytes at every value.  The default, 4, is tuned for small inboxes: it is the fastest measured
 * at 2 deliveries and 2 items a session, and a wider group pays on long inboxes.  All are read when
 * a call is enqueued; a host-only handle accepts and ignores them.  EMQX_EINVAL out of range,
 * EMQX_ENOTFOUND for unknown keys. */
int emqx_pmqueue_set_tuning(emqx_pmqueue* h, const char* key, int64_t value);
int emqx_pmqueue_stats_get(emqx_pmqueue* h, emqx_pmqueue_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_PMQUEUE_H */
