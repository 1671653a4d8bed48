/*
 * emqx_retry.h — C ABI of the retry stage (libemqxmatch.so): when each inflight entry of a session
 * went in, and the two operations of the reference that need it: the timer-driven redelivery
 * (retry/1) and the replay on resume (replay/1).  The step behind the ack stage (emqx_ack.h), which
 * keeps the inflight entries in slots[] but not their age.
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_session:await/3, with_ts/1                    apps/emqx/src/emqx_session.erl:604-606, :789-790
 *   emqx_session:pubrec/2 (the new stamp)              apps/emqx/src/emqx_session.erl:404-414
 *   emqx_session:retry/1, retry_delivery/4,5           apps/emqx/src/emqx_session.erl:612-651
 *   emqx_session:sort_fun/0, age/2                     apps/emqx/src/emqx_session.erl:780-781, :792
 *   emqx_session:replay/1                              apps/emqx/src/emqx_session.erl:692-703
 *   emqx_message:is_expired/1, elapsed/1               apps/emqx/src/emqx_message.erl:239-243, :342-343
 *   emqx_inflight:to_list/1                            apps/emqx/src/emqx_inflight.erl:109-111
 *   the known answers                                  apps/emqx/test/emqx_session_SUITE.erl:313-322, :338-346
 *
 * State: the stamp table.  It is the caller's and lies next to the ack stage's slots[]:
 * stamps[sub_limit * W] of uint64_t, stamps[sub * W + j] belonging to slots[sub * W + j]; W is one
 * of 8, 16, 32, 64 and a row is 16-byte aligned.  A stamp is
 *     ts_ms << 19 | dup << 18 | phase << 16 | pkt_id          (ts_ms < 2^45; 0: no entry)
 * and BELONGS to its slot iff the slot's phase is not EMQX_ACK_EMPTY and the stamp's phase and
 * pkt_id equal the slot's (a phase above 3 has no stamp form: such a slot never owns one).  The
 * identity rides in the stamp so that the stage can tell a fresh entry from one it has seen without
 * any change to emqx_ack_record_* or emqx_ack_run_*.
 *
 * Call 1, emqx_retry_stamp_*: behind EVERY emqx_ack_record_* and EVERY emqx_ack_run_* on the
 * stream, with that call's inbox_subs or ack_subs as subs[] (distinct; NULL: the rows 0..m-1), its
 * n_boxes / m / cap_boxes, and now_ms.  For every slot of every named row below sub_limit:
 *     the slot is EMPTY                      the stamp becomes 0
 *     the stamp belongs to the slot          unchanged (timestamp and dup are kept)
 *     otherwise                              ts now_ms, dup 0, the slot's phase and pkt_id
 * That stamps what record inserted (await/3), restamps what a PUBREC turned into PUBREL_AWAIT
 * (pubrec/2 stores a new Ts) and clears what an ack freed.  The call compares identities, not
 * histories: a slot freed and refilled with the same pkt_id and phase between two stamp calls keeps
 * the old stamp.  A caller that stamps after each record and each run call never sees that, since
 * between two stamp calls a slot is then either filled or freed, not both.  Rows named with an id
 * at or above sub_limit are skipped and set EMQX_RETRY_F_BAD_SUB.
 *
 * Call 2, emqx_retry_sweep_*, mode EMQX_RETRY_MODE_RETRY: retry/1 of the m sessions subs[] names
 * (distinct; NULL: the sessions 0..m-1, m <= sub_limit, a sweep of the whole table) at now_ms.  A
 * session's interval is intervals[sub] when intervals is not NULL, else interval_ms (both at most
 * 2^31; an intervals[] entry above it counts as 2^31).  out_status[k] is EMQX_A_OK,
 * EMQX_A_NO_SESSION (the record lacks PRESENT, or the id is not below sub_limit, which also sets
 * EMQX_RETRY_F_BAD_SUB) or EMQX_A_PASS; the latter two leave row, stamps and record untouched and
 * have no items, counts 0 and no timer.  For an OK session, each non-empty slot has the timestamp
 * of its stamp, or now_ms if the stamp does not belong to it (counted in summary word 7, sets
 * EMQX_RETRY_F_UNSTAMPED, and the slot is stamped now_ms, dup 0).  Ages are signed: a slot is OLD
 * iff now_ms - ts >= interval, so a stamp in the future is young.  The reference sorts the window
 * by Ts (stable over packet-id order) and visits it while the entries are old; with one now_ms that
 * is every old slot, ordered by (ts, pkt_id, slot index).  Those are the session's items, 8 bytes
 * each, of kind
 *     EMQX_RETRY_PUBREL        the slot is PUBREL_AWAIT; never checked for expiry
 *     EMQX_RETRY_EXPIRED       any other slot with deadlines != NULL, ref < ref_limit and
 *                              now_ms > deadlines[ref] (deadlines[ref] = CreatedAt + Interval * 1000
 *                              of the message, EMQX_RETRY_NO_EXPIRY: never).  A ref not below
 *                              ref_limit never expires and sets EMQX_RETRY_F_BAD_REF
 *     EMQX_RETRY_PUBLISH_DUP   any other slot that is not expired
 * The reference's reply list is the items other than EXPIRED in order; the EXPIRED ones are listed
 * so that the caller can release the message ('delivery.dropped.expired').  Effects: an EXPIRED
 * slot and its stamp are zeroed; every other old slot's stamp becomes now_ms with dup 1 for a
 * message and dup 0 for a PUBREL; young slots are untouched.  Outputs: out_offsets[m + 1] and
 * out_items[] (session k's items at out_offsets[k] .. out_offsets[k + 1]); out_counts[4 * k] =
 * publishes, pubrels, expired and inflight_after = sessions[sub].inflight - expired saturating at
 * 0; out_timers[k] = EMQX_RETRY_NO_TIMER when the row had no entry at entry (or the session is not
 * OK), else interval when no young entry is left (also when every entry was deleted), else
 * interval - max(0, now_ms - the smallest young ts).  With update_table != 0,
 * sessions[sub].inflight becomes inflight_after.
 *
 * Overflow: when the items of all sessions exceed cap_out the call sets EMQX_RETRY_F_OUTPUT_FULL;
 * out_offsets, out_counts, out_timers and out_status are complete, out_items, the rows, the stamps
 * and the table are UNTOUCHED, so the call can be repeated with a larger buffer (summary word 3 is
 * the count it needs).
 *
 * Mode EMQX_RETRY_MODE_REPLAY: replay/1.  Every non-empty slot of an OK session is an item, in
 * (pkt_id, slot index) order, EMQX_RETRY_PUBREL for PUBREL_AWAIT and EMQX_RETRY_PUBLISH_DUP for
 * anything else; no expiry check, every timer EMQX_RETRY_NO_TIMER, nothing written but the outputs.
 * stamps, intervals and deadlines are not read and may be NULL.  replay/1's trailing dequeue/1 is
 * emqx_mqueue_take_* (emqx_mqueue.h) on the same stream.
 *
 * No thread walks a list: per slot the fold is a predicate, per item a rank among at most W keys,
 * per session one minimum (emqx_amd/csrc/retry.h).
 *
 * Out of scope, kept by the caller: check_expire_latency and the latency stats, timer wheels (the
 * caller decides which sessions are due, or sweeps them all), a NIF binding.  awaiting_rel and the
 * inbound QoS 2 path (publish/3, pubrel/2, expire(awaiting_rel, _)) are the rel stage's
 * (emqx_rel.h).
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  Threading as in emqx_ack.h: the calls
 * on one handle share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_RETRY_H
#define EMQX_RETRY_H

#include <stdint.h>

#include "emqx_ack.h"
#include "emqx_match.h"
#include "emqx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_retry emqx_retry;

#define EMQX_RETRY_HOST_ONLY (-2) /* `device` of a handle without a device */

#define EMQX_RETRY_MODE_RETRY 0u
#define EMQX_RETRY_MODE_REPLAY 1u

/* kind of an item */
#define EMQX_RETRY_PUBLISH_DUP 1u /* the message again, with dup set  */
#define EMQX_RETRY_PUBREL 2u      /* {pubrel, PacketId}               */
#define EMQX_RETRY_EXPIRED 3u     /* deleted: release the message     */

#define EMQX_RETRY_NO_TIMER 0xFFFFFFFFu
#define EMQX_RETRY_NO_EXPIRY 0xFFFFFFFFFFFFFFFFull /* a deadline that never passes */
#define EMQX_RETRY_MAX_INTERVAL (1ull << 31)       /* interval_ms is at most this  */
#define EMQX_RETRY_MAX_NOW (1ull << 45)            /* now_ms is below this         */

/* the fields of a stamp */
#define EMQX_RETRY_STAMP_TS_SHIFT 19
#define EMQX_RETRY_STAMP_DUP (1ull << 18)
#define EMQX_RETRY_STAMP_PHASE_SHIFT 16

/* One item, 8 bytes. */
typedef struct emqx_retry_item {
  uint16_t pkt_id;
  uint8_t kind; /* EMQX_RETRY_PUBLISH_DUP / PUBREL / EXPIRED */
  uint8_t qos;
  uint32_t ref;
} emqx_retry_item;

/* summary[8] of a stamp call: [0] flags, [1] rows stamped over (named and below sub_limit),
 * [2] rows named m, [3] slots stamped, [4] stamps cleared, [5..7] 0.
 * summary[8] of a sweep call: [0] flags, [1] sessions with status EMQX_A_OK, [2] sessions m,
 * [3] items (with EMQX_RETRY_F_OUTPUT_FULL: the cap_out the call needs), [4] PUBLISH_DUP,
 * [5] PUBREL, [6] EXPIRED, [7] slots found unstamped. */
#define EMQX_RETRY_SUMMARY_WORDS 8
#define EMQX_RETRY_F_INPUT_REFUSED 0x2u /* as EMQX_ACK_F_INPUT_REFUSED: m > cap_boxes or >= 2^32, or subs NULL and   */
                                        /* m > sub_limit: [2] as read, nothing else written but the summary          */
#define EMQX_RETRY_F_BAD_SUB 0x4u       /* some subscriber id >= sub_limit: the row is skipped (sweep: NO_SESSION)   */
#define EMQX_RETRY_F_OUTPUT_FULL 0x8u   /* sweep: more items than cap_out; see "Overflow"                            */
#define EMQX_RETRY_F_BAD_REF 0x10u      /* sweep: an old message slot's ref >= ref_limit; it does not expire         */
#define EMQX_RETRY_F_UNSTAMPED 0x20u    /* sweep: a non-empty slot whose stamp does not belong to it                 */

/* One stamp call.  Every pointer is host memory for emqx_retry_stamp_batch and
 * emqx_retry_stamp_host, device memory for the _device forms.
 * In:  subs[m] (distinct; NULL: 0..m-1); n_boxes NULL: the row count is `m`, else it is read from
 *      there when the call runs; slots[sub_limit * W].
 * Out: stamps[sub_limit * W], the named rows updated in place. */
typedef struct emqx_retry_stamp_args {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_boxes;
  const emqx_ack_slot* slots;
  uint64_t* stamps;
  uint64_t w;
  uint64_t sub_limit;
  uint64_t now_ms;
} emqx_retry_stamp_args;

/* One sweep call.
 * In:  subs[m], n_boxes, m, cap_boxes as above; sessions[sub_limit] (required); slots and stamps
 *      (stamps NULL only in replay mode); now_ms, interval_ms, intervals[sub_limit] or NULL;
 *      deadlines[ref_limit] or NULL; mode; cap_out.
 * Out: out_offsets[cap_boxes + 1], out_items[cap_out], out_status[cap_boxes],
 *      out_counts[4 * cap_boxes] (16-byte aligned), out_timers[cap_boxes], the first m (m + 1)
 *      written; the rows, the stamps and, with update_table != 0, sessions[].inflight.  The outputs
 *      are distinct from the inputs and from each other. */
typedef struct emqx_retry_sweep_args {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_boxes;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  emqx_ack_slot* slots;
  uint64_t* stamps;
  uint64_t w;
  uint64_t now_ms;
  uint64_t interval_ms;
  const uint32_t* intervals;
  const uint64_t* deadlines;
  uint64_t ref_limit;
  uint64_t mode;
  uint64_t cap_out;
  uint64_t* out_offsets;
  emqx_retry_item* out_items;
  uint8_t* out_status;
  uint32_t* out_counts;
  uint32_t* out_timers;
} emqx_retry_sweep_args;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_retry_stats) before the call. */
typedef struct emqx_retry_stats {
  uint64_t size;          /* in: sizeof(emqx_retry_stats) of the caller; out: bytes written */
  uint64_t cap_boxes;     /* rows or sessions the reserved scratch takes                    */
  uint64_t w;             /* the largest W it takes                                         */
  uint64_t scratch_bytes; /* device memory held: 8 bytes per 256 lanes of rows, the counters */
  uint64_t calls;         /* calls so far, all forms                                        */
  double last_call_ms;    /* time of the last synchronous call                              */
} emqx_retry_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_RETRY_HOST_ONLY: a handle that answers
 * the _host calls alone; its batch entry points return EMQX_EDEVICE (nothing ever falls back to
 * the host silently). */
int emqx_retry_create(int32_t device, emqx_retry** out);
int emqx_retry_destroy(emqx_retry* h);

/* Sizes the device scratch for calls of up to cap_boxes rows (< 2^32) of w slots.  It only grows;
 * it waits for the handle's call in flight first. */
int emqx_retry_reserve(emqx_retry* h, uint64_t cap_boxes, uint64_t w);

/* The four forms of each call, as in emqx_ack.h.
 *   host buffers, evaluated on the device: the m rows, stamp rows, records and intervals the call
 *     names travel, not the tables (deadlines[] travels whole; n_boxes must be NULL).
 *   _device: device buffers on `stream` (NULL: the handle's own, ordered after the device's null
 *     stream); synchronizes the stream; the scratch grows as needed.
 *   _device_async: enqueues kernels only and returns at once; every count is read on the device;
 *     `summary` (>= 8 uint64_t, device or host-pinned memory) is written last, with plain stores.
 *     Whatever the device buffers hold, no access leaves them.  EMQX_EOVERFLOW, nothing enqueued:
 *     the reserved scratch is smaller than cap_boxes or w.
 *   _host: the same bytes computed on the calling thread.
 * The synchronous forms return EMQX_EINVAL for a bad argument (w, now_ms >= 2^45, interval_ms >
 * 2^31, an unknown mode, a missing buffer), a refused input or a subscriber >= sub_limit (the
 * outputs are still complete), and EMQX_EOVERFLOW for EMQX_RETRY_F_OUTPUT_FULL.
 * summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_retry_stamp_batch(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out);
int emqx_retry_stamp_batch_device(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out, void* stream);
int emqx_retry_stamp_batch_device_async(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary, void* stream);
int emqx_retry_stamp_host(emqx_retry* h, const emqx_retry_stamp_args* b, uint64_t* summary_out);

int emqx_retry_sweep_batch(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out);
int emqx_retry_sweep_batch_device(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out, void* stream);
int emqx_retry_sweep_batch_device_async(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary, void* stream);
int emqx_retry_sweep_host(emqx_retry* h, const emqx_retry_sweep_args* b, uint64_t* summary_out);

/* Keys: "max_blocks" (1..4096, default 4096): the grid cap of every pass over the rows, the blocks
 * stride over the groups of rows beyond it; "scan_chunk" (1..1024, default 1024): the totals the
 * sweep's one-block scan takes per carry step (tests lower both to make the blocks stride and the
 * scan carry at small shapes; the same bytes at every value).  Both are read when a call is
 * enqueued; a host-only handle accepts and ignores them.  EMQX_EINVAL out of range, EMQX_ENOTFOUND
 * for unknown keys. */
int emqx_retry_set_tuning(emqx_retry* h, const char* key, int64_t value);
int emqx_retry_stats_get(emqx_retry* h, emqx_retry_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_RETRY_H */
