/*
 * emqx_ack.h — C ABI of the ack stage (libemqxmatch.so): which packet ids are inflight per
 * session, and a batch of PUBACK / PUBREC / PUBCOMP evaluated against them.  The step behind the
 * window stage (emqx_window.h), which only ever fills the window; this stage reopens it.
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_session:puback/2                              apps/emqx/src/emqx_session.erl:379-389
 *   emqx_session:pubrec/2                              apps/emqx/src/emqx_session.erl:404-414
 *   emqx_session:pubcomp/2                             apps/emqx/src/emqx_session.erl:437-447
 *   emqx_session:dequeue/1, dequeue/3, acc_cnt/2       apps/emqx/src/emqx_session.erl:453-477
 *   emqx_session:batch_n/1 (?DEFAULT_BATCH_N = 1000)   apps/emqx/src/emqx_session.erl:783-787
 *   emqx_inflight:lookup/2, update/3, delete/2         apps/emqx/src/emqx_inflight.erl
 *   the known answers                                  apps/emqx/test/emqx_session_SUITE.erl:168-230
 *
 * State: the slot table.  It is the caller's, like the window stage's sessions[]:
 * slots[sub_limit * W] of 8-byte emqx_ack_slot, row `sub` holding the inflight entries of session
 * `sub`.  W (slots per session) is a field of each call and is one of 8, 16, 32, 64 (anything
 * else: EMQX_EINVAL); a row is 16-byte aligned.  The caller chooses W >= inflight_max; sessions a
 * row cannot hold (inflight_max 0 or above W) are the caller's to mark EMQX_WINDOW_PASS.  `ref` is
 * the caller's 32-bit name of the message (the inbox stage's box_src, a ring index).
 *
 * Call 1, emqx_ack_record_*: behind the window stage, with that call's inbox_subs, inbox_offsets,
 * n_boxes / m, cap_in, cap_boxes and box_opts, and its outputs verdicts[] and pkt_ids[].  In inbox
 * k the r-th delivery (inbox order, r from 0) whose verdict & EMQX_W_VERDICT_MASK is EMQX_W_SEND
 * goes into the r-th EMPTY slot, ascending slot index, of row inbox_subs[k] AS THE ROW WAS AT
 * ENTRY, stored as {pkt_ids[d], EMQX_ACK_MSG, box_opts[d] & EMQX_DELIVER_QOS_MASK, refs[d]}
 * (refs NULL: the delivery's position d).  Sends beyond the row's empty slots are not recorded:
 * they are counted in out_unrecorded[k] and the summary and set EMQX_ACK_F_ROW_FULL.  No
 * duplicate check is made: an id the row already holds is stored a second time (the reference
 * would crash in gb_trees:insert).  An inbox whose subscriber is not below sub_limit records
 * nothing, has all its sends in out_unrecorded[k], and sets EMQX_ACK_F_BAD_SUB.  The rank r is by
 * order alone, for any verdicts[] and pkt_ids[] a caller passes; no thread walks an inbox.  The
 * window's session table is neither read nor written: the window already counted these sends.
 *
 * Call 2, emqx_ack_run_*: a batch of acks grouped by session exactly as the inbox stage groups:
 * ack_subs[m] (distinct), ack_offsets[m+1], and acks[], each kind << 16 | pkt_id with kind
 * EMQX_ACK_PUBACK / PUBREC / PUBCOMP, in arrival order within a session.  A caller gets this
 * layout from emqx_inbox_group_batch_device_async by passing one "message" per ack
 * (offsets = 0..n), the session of each ack as subs[] and the packed ack as filters[]: that call's
 * box_filters, inbox_subs, inbox_offsets and summary word 2 (as n_boxes) are this call's inputs on
 * the same stream.
 *
 * The result is the reference's sequential fold per session.  For each ack in list order: the
 * verdict is the first of
 *   EMQX_A_NO_SESSION   the record lacks PRESENT, or the subscriber id is not below sub_limit
 *   EMQX_A_PASS         the record has PASS: row and record untouched
 *   EMQX_A_BAD_KIND     kind not 1..3: no effect
 * and otherwise follows from the slot the id names and that slot's phase AT THAT MOMENT:
 *                slot is MSG                slot is PUBREL_AWAIT     no such slot
 *   PUBACK       OK, slot becomes EMPTY     IN_USE                   NOT_FOUND
 *   PUBREC       OK, becomes PUBREL_AWAIT   IN_USE                   NOT_FOUND
 *   PUBCOMP      IN_USE                     OK, slot becomes EMPTY   NOT_FOUND
 * (EMQX_A_IN_USE is MQTT 0x91, EMQX_A_NOT_FOUND 0x92).  The slot an id names is the lowest slot
 * index of the row at entry with phase != EMPTY and that pkt_id; in a malformed row that holds an
 * id twice the higher slot is shadowed for the whole call and stays as it is.  "No such slot"
 * includes a slot this call has already emptied.
 *
 * Outputs: verdicts[d]; out_refs[d] = the slot's ref for every OK (the reference returns the
 * message on puback and pubrec), EMQX_ACK_NO_REF otherwise; out_counts[4 * k] = released (slots
 * that became EMPTY), to_pubrel (PUBREC OKs), errors (IN_USE + NOT_FOUND + BAD_KIND) and room =
 * batch_n/1 on the window after the batch: 1000 if inflight_max == 0, else inflight_max -
 * inflight_after saturating at 0 (all four 0 for a NO_SESSION or PASS session).  The row is
 * rewritten in place: freed slots are zeroed, the others keep their position.  With
 * update_table != 0, sessions[sub].inflight becomes inflight - released (saturating at 0) and
 * nothing else in the record changes: the next emqx_window_run_batch_device_async on the stream
 * sees the reopened window with no host read.
 *
 * No thread walks a session's ack list: a slot's phase only moves MSG -> PUBREL_AWAIT -> EMPTY or
 * MSG -> EMPTY within a call and nothing is inserted, so the fold has a closed form in two
 * per-slot minima (emqx_amd/csrc/ack.h), and the time of a call does not depend on how the acks
 * are spread over the sessions.
 *
 * Out of scope, kept by the caller: latency stats, a NIF binding.  awaiting_rel and the inbound
 * QoS 2 path (publish/3, pubrel/2, expire(awaiting_rel, _)) are the rel stage's (emqx_rel.h), which
 * keeps a table of its own next to slots[] and runs in front of the match.  The dequeue/1 that follows an ack is the mqueue stage's
 * (emqx_mqueue.h): its take call runs behind the run call on the stream, reads the lowered
 * `inflight` and pops what `room` allows; its outputs are inputs of the record call, which needs no
 * change for it.  The timestamps of the entries, retry/1 with
 * message expiry and replay/1 are the retry stage's (emqx_retry.h): it keeps a stamp per slot next
 * to slots[] and is called behind every record and run call.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  Threading as in emqx_inbox.h: the
 * calls on one handle share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_ACK_H
#define EMQX_ACK_H

#include <stdint.h>

#include "emqx_deliver.h"
#include "emqx_match.h"
#include "emqx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_ack emqx_ack;

#define EMQX_ACK_HOST_ONLY (-2) /* `device` of a handle without a device */

/* phase of a slot */
#define EMQX_ACK_EMPTY 0u
#define EMQX_ACK_MSG 1u          /* a #message{} is inflight                 */
#define EMQX_ACK_PUBREL_AWAIT 2u /* PUBREC seen, {pubrel, Ts} is inflight    */

/* kind of an ack: acks[d] = kind << 16 | pkt_id */
#define EMQX_ACK_PUBACK 1u
#define EMQX_ACK_PUBREC 2u
#define EMQX_ACK_PUBCOMP 3u

/* the verdict byte */
#define EMQX_A_OK 1u
#define EMQX_A_IN_USE 2u    /* MQTT 0x91 */
#define EMQX_A_NOT_FOUND 3u /* MQTT 0x92 */
#define EMQX_A_NO_SESSION 4u
#define EMQX_A_PASS 5u
#define EMQX_A_BAD_KIND 6u

#define EMQX_ACK_NO_REF 0xFFFFFFFFu
#define EMQX_ACK_DEFAULT_BATCH_N 1000u  /* ?DEFAULT_BATCH_N */
#define EMQX_ACK_MAX_ACKS (1ull << 31)  /* a call takes fewer acks than this */

/* One inflight entry, 8 bytes. */
typedef struct emqx_ack_slot {
  uint16_t pkt_id;
  uint8_t phase; /* EMQX_ACK_EMPTY / MSG / PUBREL_AWAIT */
  uint8_t qos;
  uint32_t ref;
} emqx_ack_slot;

/* summary[8] of a record call: [0] flags, [1] deliveries (inbox_offsets[m]), [2] inboxes m,
 * [3] EMQX_W_SEND verdicts, [4] recorded, [5] not recorded ([3] - [4]), [6] inboxes whose row was
 * too full, [7] 0.
 * summary[8] of a run call: [0] flags, [1] acks (ack_offsets[m]), [2] sessions m, [3] OK,
 * [4] released slots, [5] IN_USE, [6] NOT_FOUND, [7] the rest (NO_SESSION, PASS, BAD_KIND). */
#define EMQX_ACK_SUMMARY_WORDS 8
#define EMQX_ACK_F_INPUT_REFUSED 0x2u /* offsets[m] > cap_in or >= 2^32 (run: >= 2^31), m > cap_boxes or >= 2^32:  */
                                      /* [1] and [2] as read, nothing else written but the summary                 */
#define EMQX_ACK_F_BAD_SUB 0x4u       /* some subscriber id >= sub_limit: record: nothing recorded for that inbox; */
                                      /* run: its acks are EMQX_A_NO_SESSION; the rest is valid                    */
#define EMQX_ACK_F_ROW_FULL 0x8u      /* record: some inbox had more sends than its row had empty slots            */

/* One record call.  Every pointer is host memory for emqx_ack_record_batch and
 * emqx_ack_record_host, device memory for the _device forms.
 * In:  inbox_subs[m] (distinct), inbox_offsets[m + 1] with inbox_offsets[0] = 0 and no decrease,
 *      box_opts[], verdicts[], pkt_ids[] and optionally refs[] of capacity cap_in; n_boxes as in
 *      emqx_window_batch.
 * Out: slots[sub_limit * W], the rows of the inboxes' sessions updated in place;
 *      out_unrecorded[cap_boxes], the first m written. */
typedef struct emqx_ack_record_args {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  const uint8_t* verdicts;
  const uint16_t* pkt_ids;
  const uint32_t* refs;
  emqx_ack_slot* slots;
  uint64_t w;
  uint64_t sub_limit;
  uint32_t* out_unrecorded;
} emqx_ack_record_args;

/* One run call.
 * In:  ack_subs[m] (distinct), ack_offsets[m + 1] with ack_offsets[0] = 0 and no decrease,
 *      acks[] of capacity cap_in; n_boxes NULL: the session count is `m`, else it is read from
 *      there when the call runs; sessions[sub_limit] (required) for PRESENT, PASS, inflight and
 *      inflight_max; slots[sub_limit * W].
 * Out: verdicts[] and out_refs[] of capacity cap_in, the first ack_offsets[m] written;
 *      out_counts[4 * cap_boxes], the first m sessions written; the rows; sessions[].inflight with
 *      update_table != 0.  The outputs are distinct from the inputs and from each other. */
typedef struct emqx_ack_run_args {
  const uint32_t* ack_subs;
  const uint64_t* ack_offsets;
  const uint32_t* acks;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  emqx_ack_slot* slots;
  uint64_t w;
  uint8_t* verdicts;
  uint32_t* out_refs;
  uint32_t* out_counts;
} emqx_ack_run_args;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_ack_stats) before the call. */
typedef struct emqx_ack_stats {
  uint64_t size;          /* in: sizeof(emqx_ack_stats) of the caller; out: bytes written       */
  uint64_t cap_in;        /* deliveries or acks the reserved scratch takes                      */
  uint64_t cap_boxes;     /* inboxes or sessions it takes                                       */
  uint64_t w;             /* the largest W it takes                                             */
  uint64_t scratch_bytes; /* device memory held: 8 * cap_boxes * (w + 2) and the tile totals    */
  uint64_t rematch;       /* tuning key "rematch"                                               */
  uint64_t calls;         /* calls so far, all forms                                            */
  double last_call_ms;    /* time of the last synchronous call                                  */
} emqx_ack_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_ACK_HOST_ONLY: a handle that answers the
 * _host calls alone; its batch entry points return EMQX_EDEVICE (nothing ever falls back to the
 * host silently). */
int emqx_ack_create(int32_t device, emqx_ack** out);
int emqx_ack_destroy(emqx_ack* h);

/* Sizes the device scratch for calls of up to cap_in deliveries or acks, cap_boxes inboxes or
 * sessions (both < 2^32) and rows of w slots.  It only grows; it waits for the handle's call in
 * flight first. */
int emqx_ack_reserve(emqx_ack* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w);

/* The four forms of each call, as in emqx_window.h.
 *   host buffers, evaluated on the device: the m rows (and records) the call names travel, not the
 *     tables (n_boxes must be NULL).  EMQX_EINVAL: offsets[0] != 0, decreasing offsets, a refused
 *     input, a subscriber >= sub_limit (the outputs are still complete).
 *   _device: device buffers on `stream` (NULL: the handle's own, ordered after the device's null
 *     stream); synchronizes the stream; the scratch grows as needed.
 *   _device_async: enqueues kernels only and returns at once; every count is read on the device;
 *     `summary` (>= 8 uint64_t, device or host-pinned memory) is written last, with plain stores.
 *     Whatever the device buffers hold, no access leaves them.  EMQX_EOVERFLOW, nothing enqueued:
 *     the reserved scratch is smaller than cap_in, cap_boxes or w.
 *   _host: the same bytes computed on the calling thread.
 * summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_ack_record_batch(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out);
int emqx_ack_record_batch_device(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out, void* stream);
int emqx_ack_record_batch_device_async(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary, void* stream);
int emqx_ack_record_host(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out);

int emqx_ack_run_batch(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out);
int emqx_ack_run_batch_device(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out, void* stream);
int emqx_ack_run_batch_device_async(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary, void* stream);
int emqx_ack_run_host(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out);

/* Keys: "rematch": 0 (default) the verdict buffer carries an ack's matched slot between the passes
 * of a run call; 1 every pass matches the ack against its row again (the same bytes, more row
 * reads); "max_blocks" (1..4096, default 4096): the grid cap of every pass whose blocks stride
 * (the tile passes of record and run, run's init pass and both rows kernels), the blocks stride
 * over the tiles or rows beyond it; "scan_chunk" (1..1024, default 1024): the tile totals record's
 * one-block scan takes per carry step (tests lower both to make the blocks stride and the scan
 * carry at small shapes; the same bytes at every value).  Both are read when a call is enqueued;
 * a host-only handle accepts and ignores them.  EMQX_EINVAL out of range, EMQX_ENOTFOUND for
 * unknown keys. */
int emqx_ack_set_tuning(emqx_ack* h, const char* key, int64_t value);
int emqx_ack_stats_get(emqx_ack* h, emqx_ack_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_ACK_H */
