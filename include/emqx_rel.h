/*
 * emqx_rel.h — C ABI of the rel stage (libemqxmatch.so): the inbound half of emqx_session.  Which
 * QoS 2 packet ids a session has received and not yet seen released (awaiting_rel), a batch of
 * inbound PUBLISH / PUBREL evaluated against them, and the expiry of stale ids.  The stage stands
 * in FRONT of the match: it decides which messages of an inbound batch are routed at all, and its
 * out_route[] is the list the match call takes.
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_session:publish/3, is_awaiting_full/1         apps/emqx/src/emqx_session.erl:342-369
 *   emqx_session:pubrel/2                              apps/emqx/src/emqx_session.erl:420-428
 *   expire(awaiting_rel, _), expire_awaiting_rel/2     apps/emqx/src/emqx_session.erl:657-674
 *   age/2                                              apps/emqx/src/emqx_session.erl:792
 *   the defaults (max_awaiting_rel 100,
 *   await_rel_timeout 300000)                          apps/emqx/src/emqx_session.erl:208-210
 *   what the channel does with the answers             apps/emqx/src/emqx_channel.erl:402-410, :618-640
 *   a disconnected channel ignores the timer           apps/emqx/src/emqx_channel.erl:1123-1133
 *   reason codes 0x91, 0x92, 0x93                      apps/emqx/include/emqx_mqtt.hrl:143-145
 *   the known answers                                  apps/emqx/test/emqx_session_SUITE.erl:138-166,
 *                                                      :209-215, :348-358
 *
 * State: the awaiting table.  It is the caller's and lies next to the ack stage's slots[]:
 * rel[sub_limit * W] of uint64_t, row `sub` holding the awaiting_rel map of session `sub`.  W
 * (entries per session) is a field of each call and is one of 8, 16, 32, 64, 128 (anything else:
 * EMQX_EINVAL; 128 covers the default limit of 100); a row is 16-byte aligned.  An entry is
 *   ts_ms << 17 | 1 << 16 | pkt_id        with ts_ms < 2^45;  0 is an empty entry,
 * and every non-zero word counts as an entry whose id is its low 16 bits.  A session's
 * awaiting_rel_cnt is the number of non-zero entries of its row; the 32-byte emqx_window_session
 * is not changed and the stage never writes sessions[]: it reads a record's flags for
 * EMQX_WINDOW_PRESENT, EMQX_WINDOW_PASS and EMQX_WINDOW_CONNECTED only.
 *
 * Limits, a scalar and an optional array as the retry stage's intervals: max_awaiting (0 =
 * infinity) is every session's max_awaiting_rel unless maxes[sub_limit] is given; timeout_ms
 * (EMQX_REL_NO_TIMEOUT = infinity) is every session's await_rel_timeout unless
 * timeouts[sub_limit] is given.
 *
 * Call 1, emqx_rel_run_*: one inbound batch grouped by session exactly as emqx_ack_run_* takes its
 * acks: ev_subs[m] (distinct), ev_offsets[m + 1], and events[], each kind << 16 | pkt_id with kind
 *   EMQX_REL_PUBLISH   a QoS 2 PUBLISH (the first clause of publish/3)
 *   EMQX_REL_PUBREL    a PUBREL (pubrel/2)
 *   EMQX_REL_DIRECT    a QoS 0 / 1 PUBLISH (the second clause of publish/3): always routed, no state
 * in arrival order within a session.  Optional ts[] (uint64 per event) is the message's timestamp,
 * which is what the reference stores (maps:put(PacketId, Ts, _)); NULL: the call's now_ms.  A stamp
 * not below 2^45 is stored as 2^45 - 1 and, when it is stored, sets EMQX_REL_F_BAD_TS.  Optional
 * src[] (uint32 per event) is the caller's message index, for example the inbox stage's box_src.
 * A caller gets this layout from emqx_inbox_group_batch_device_async as emqx_ack.h describes for
 * acks: one "message" per event, the session of each event as subs[] and the packed event as
 * filters[]; that call's box_filters, inbox_subs, inbox_offsets, box_src and summary word 2 (as
 * n_boxes) are this call's inputs on the same stream.
 *
 * The result is the reference's sequential fold per session, in list order.  With `limit` the
 * session's max_awaiting_rel, the verdict byte of an event is the first of
 *   EMQX_REL_NO_SESSION  the record lacks PRESENT, or the subscriber id is not below sub_limit (the
 *                        second also sets EMQX_REL_F_BAD_SUB)
 *   EMQX_REL_PASS        the record has PASS: the row is untouched
 *   EMQX_REL_ROW_SMALL   limit is 0 (infinity) or above W: the row cannot hold what the reference
 *                        could, the session is treated as PASS and EMQX_REL_F_ROW_SMALL is set;
 *                        nothing ever silently differs from the reference
 *   EMQX_REL_BAD_KIND    kind not 1..3: no effect
 * and otherwise, with c the number of non-empty entries of the row AT THAT MOMENT:
 *   DIRECT     EMQX_REL_OK, routed
 *   PUBLISH    c >= limit: EMQX_REL_EXCEEDED (0x93), even when the id is present: the full check
 *              comes first (:347); else the id is present: EMQX_REL_IN_USE (0x91); else EMQX_REL_OK:
 *              the entry goes into the lowest empty slot of the row at that moment and the event is
 *              routed
 *   PUBREL     the id is present: EMQX_REL_OK, and the lowest-index non-empty slot that holds the id
 *              at that moment is zeroed (a malformed row that holds an id twice gives it up in two
 *              PUBRELs); else EMQX_REL_NOT_FOUND (0x92)
 * Because the slot choice is defined, rows compare byte for byte.
 *
 * Outputs: verdicts[d]; out_route[] (capacity cap_in) = src[d], or d with src NULL, of every routed
 * event (the OK PUBLISHes and DIRECTs) in grouped position order, their number in summary word 3:
 * it is bounded by the event count, so there is no overflow protocol; out_counts[4 * k] = routed,
 * released (the PUBREL OKs), errors (IN_USE + NOT_FOUND + EXCEEDED + BAD_KIND) and cnt_after (the
 * row's entries behind the batch), all four 0 for a NO_SESSION, PASS or ROW_SMALL session, whose
 * events are not routed either: such sessions stay the caller's; out_arm[k] = 1 iff the session had
 * an OK QoS 2 PUBLISH, which is where the channel calls ensure_timer(await_timer, _), else 0.  The
 * rows are updated in place; a row that did not change is not stored.
 * ev_subs distinct is a precondition: with duplicates those sessions' results are unspecified, but
 * no access leaves the buffers.
 *
 * Whether a PUBLISH lands depends on every earlier verdict of its session (an insert under a size
 * limit, a removal that makes room), so there is no closed form in per-slot minima as the ack
 * stage has one: a group of lanes steps through a session's events (emqx_amd/csrc/rel_kernels.hip),
 * and a session of n events costs n dependent steps of one group.
 *
 * Call 2, emqx_rel_expire_*: expire(awaiting_rel, _) at now_ms for the m sessions subs[] names
 * (distinct); subs NULL: the sessions 0 .. m - 1, a sweep of the table.  An entry is expired iff
 * (int64)(now_ms - ts_ms) >= timeout, so a stamp in the future is young (age/2 is a plain
 * difference), and never with timeout infinity; expired entries are zeroed.  out_status[k] is the
 * first of EMQX_REL_NO_SESSION (as above), EMQX_REL_PASS, EMQX_REL_IDLE (channel_rule != 0 and the
 * record lacks CONNECTED: the session is left untouched, emqx_channel.erl:1123-1125) and
 * EMQX_REL_OK.  out_counts[4 * k] = expired, remaining, timer_armed, 0 with timer_armed = 1 iff
 * remaining > 0: the reference re-arms with the full timeout, not the remainder (:673); all 0
 * unless the status is OK.  Only changed 16-byte pairs of a row are stored.
 *
 * Out of scope, kept by the caller: priority tables and takeover, the PUBREC / PUBCOMP replies
 * themselves (the verdict byte is their reason code), the metrics of inc_expired_cnt, a NIF
 * binding.
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.  Threading as in emqx_inbox.h: the
 * calls on one handle share its device scratch and are ordered by the handle.
 */
#ifndef EMQX_REL_H
#define EMQX_REL_H

#include <stdint.h>

#include "emqx_match.h"
#include "emqx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_rel emqx_rel;

#define EMQX_REL_HOST_ONLY (-2) /* `device` of a handle without a device */

/* kind of an event: events[d] = kind << 16 | pkt_id */
#define EMQX_REL_PUBLISH 1u
#define EMQX_REL_PUBREL 2u
#define EMQX_REL_DIRECT 3u

/* the verdict byte of an event, the status byte of an expire call's session */
#define EMQX_REL_OK 1u
#define EMQX_REL_IN_USE 2u    /* MQTT 0x91 */
#define EMQX_REL_NOT_FOUND 3u /* MQTT 0x92 */
#define EMQX_REL_EXCEEDED 4u  /* MQTT 0x93 */
#define EMQX_REL_NO_SESSION 5u
#define EMQX_REL_PASS 6u
#define EMQX_REL_ROW_SMALL 7u
#define EMQX_REL_BAD_KIND 8u
#define EMQX_REL_IDLE 9u /* expire alone */

#define EMQX_REL_DEFAULT_MAX_AWAITING 100u /* max_awaiting_rel  */
#define EMQX_REL_DEFAULT_TIMEOUT 300000u   /* await_rel_timeout */
#define EMQX_REL_NO_TIMEOUT 0xFFFFFFFFu    /* timeout infinity  */
#define EMQX_REL_MAX_W 128u
#define EMQX_REL_TS_LIMIT (1ull << 45)     /* a stored stamp is below this */
#define EMQX_REL_MAX_EVENTS (1ull << 31)   /* a call takes fewer events than this */

/* An entry of the awaiting table. */
#define EMQX_REL_ENTRY(ts_ms, pkt_id) (((uint64_t)(ts_ms) << 17) | (1ull << 16) | ((uint64_t)(pkt_id) & 0xFFFFu))
#define EMQX_REL_ENTRY_ID(e) ((uint32_t)((e) & 0xFFFFu))
#define EMQX_REL_ENTRY_TS(e) ((uint64_t)(e) >> 17)

/* summary[8] of a run call: [0] flags, [1] events (ev_offsets[m]), [2] sessions m, [3] routed (the
 * length of out_route), [4] released, [5] IN_USE, [6] NOT_FOUND, [7] EXCEEDED.
 * summary[8] of an expire call: [0] flags, [1] sessions with status OK, [2] m, [3] expired,
 * [4] remaining, [5] sessions armed, [6] 0, [7] 0. */
#define EMQX_REL_SUMMARY_WORDS 8
#define EMQX_REL_F_INPUT_REFUSED 0x2u /* run: ev_offsets[m] > cap_in or >= 2^31; both: m > cap_boxes or >= 2^32:  */
                                      /* [1] (run) and [2] as read, nothing else written but the summary         */
#define EMQX_REL_F_BAD_SUB 0x4u       /* some subscriber id >= sub_limit: NO_SESSION; the rest is valid           */
#define EMQX_REL_F_ROW_SMALL 0x8u     /* run: some session's limit is 0 or above W                               */
#define EMQX_REL_F_BAD_TS 0x10u       /* run: a stamp >= 2^45 was stored as 2^45 - 1                              */

/* One run call.  Every pointer is host memory for emqx_rel_run_batch and emqx_rel_run_host, device
 * memory for the _device forms.
 * In:  ev_subs[m] (distinct), ev_offsets[m + 1] with ev_offsets[0] = 0 and no decrease, events[] and
 *      optionally ts[] and src[] of capacity cap_in; n_boxes NULL: the session count is `m`, else it
 *      is read from there when the call runs; sessions[sub_limit] (required); rel[sub_limit * W];
 *      maxes NULL or [sub_limit].
 * Out: verdicts[] and out_route[] of capacity cap_in, the first ev_offsets[m] and summary[3]
 *      written; out_counts[4 * cap_boxes] and out_arm[cap_boxes], the first m sessions written; the
 *      rows.  The outputs are distinct from the inputs and from each other. */
typedef struct emqx_rel_run_args {
  const uint32_t* ev_subs;
  const uint64_t* ev_offsets;
  const uint32_t* events;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_in;
  uint64_t cap_boxes;
  const uint64_t* ts;
  const uint32_t* src;
  const emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t* rel;
  uint64_t w;
  uint64_t now_ms;
  uint32_t max_awaiting; /* 0 = infinity */
  uint32_t reserved;     /* 0 */
  const uint32_t* maxes;
  uint8_t* verdicts;
  uint32_t* out_route;
  uint32_t* out_counts;
  uint8_t* out_arm;
} emqx_rel_run_args;

/* One expire call.
 * In:  subs NULL or [m] (distinct); n_boxes as above; sessions[sub_limit] (required);
 *      rel[sub_limit * W]; timeouts NULL or [sub_limit].
 * Out: out_status[cap_boxes] and out_counts[4 * cap_boxes], the first m sessions written; the rows. */
typedef struct emqx_rel_expire_args {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m;
  uint64_t cap_boxes;
  const emqx_window_session* sessions;
  uint64_t sub_limit;
  uint64_t* rel;
  uint64_t w;
  uint64_t now_ms;
  uint32_t timeout_ms; /* EMQX_REL_NO_TIMEOUT = infinity */
  uint32_t reserved;   /* 0 */
  const uint32_t* timeouts;
  uint64_t channel_rule;
  uint8_t* out_status;
  uint32_t* out_counts;
} emqx_rel_expire_args;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_rel_stats) before the call. */
typedef struct emqx_rel_stats {
  uint64_t size;          /* in: sizeof(emqx_rel_stats) of the caller; out: bytes written */
  uint64_t cap_in;        /* events the reserved scratch takes                            */
  uint64_t cap_boxes;     /* sessions it takes                                            */
  uint64_t w;             /* the largest W it takes                                       */
  uint64_t scratch_bytes; /* device memory held: the tile totals and the counters         */
  uint64_t lanes;         /* tuning key "lanes"                                           */
  uint64_t calls;         /* calls so far, all forms                                      */
  double last_call_ms;    /* time of the last synchronous call                            */
} emqx_rel_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_REL_HOST_ONLY: a handle that answers the
 * _host calls alone; its batch entry points return EMQX_EDEVICE (nothing ever falls back to the
 * host silently). */
int emqx_rel_create(int32_t device, emqx_rel** out);
int emqx_rel_destroy(emqx_rel* h);

/* Sizes the device scratch for calls of up to cap_in events, cap_boxes sessions (both < 2^32) and
 * rows of w entries.  It only grows; it waits for the handle's call in flight first. */
int emqx_rel_reserve(emqx_rel* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w);

/* The four forms of each call, as in emqx_ack.h.
 *   host buffers, evaluated on the device: the m rows and records the call names travel, not the
 *     tables (n_boxes must be NULL).  EMQX_EINVAL: offsets[0] != 0, decreasing offsets, a refused
 *     input, a subscriber >= sub_limit (the outputs are still complete).
 *   _device: device buffers on `stream` (NULL: the handle's own, ordered after the device's null
 *     stream); synchronizes the stream; the scratch grows as needed.
 *   _device_async: enqueues kernels only and returns at once; every count is read on the device;
 *     `summary` (>= 8 uint64_t, device or host-pinned memory) is written last, with plain stores.
 *     Whatever the device buffers hold, no access leaves them and no loop runs past cap_in steps.
 *     EMQX_EOVERFLOW, nothing enqueued: the reserved scratch is smaller than cap_in, cap_boxes or w.
 *   _host: the same bytes computed on the calling thread.
 * summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_rel_run_batch(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out);
int emqx_rel_run_batch_device(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out, void* stream);
int emqx_rel_run_batch_device_async(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary, void* stream);
int emqx_rel_run_host(emqx_rel* h, const emqx_rel_run_args* b, uint64_t* summary_out);

int emqx_rel_expire_batch(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out);
int emqx_rel_expire_batch_device(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out, void* stream);
int emqx_rel_expire_batch_device_async(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary, void* stream);
int emqx_rel_expire_host(emqx_rel* h, const emqx_rel_expire_args* b, uint64_t* summary_out);

/* Keys: "lanes": the lanes of a wave that own one session in the run fold: 0 (default) max(4, W / 16),
 * chosen by measurement, or 4, 8, 16, 32, 64; a value above W / 2 of a call is lowered to W / 2 (the
 * same bytes at every value).  "max_blocks" (1..4096, default 4096) and "scan_chunk" (1..1024, default 1024) as
 * in emqx_ack.h: the grid cap of every pass whose blocks stride, and the tile totals the route
 * list's one-block scan takes per carry step.  All are read when a call is enqueued; a host-only
 * handle accepts and ignores them.  EMQX_EINVAL out of range, EMQX_ENOTFOUND for unknown keys. */
int emqx_rel_set_tuning(emqx_rel* h, const char* key, int64_t value);
int emqx_rel_stats_get(emqx_rel* h, emqx_rel_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_REL_H */
