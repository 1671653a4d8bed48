/*
 * emqx_inbox.h — C ABI of the inbox stage (libemqxmatch.so): a batch's deliveries grouped by
 * subscriber, the step behind the fan-out (emqx_fanout_batch_device*) or behind the enrich
 * stage's compacted form (emqx_deliver_enrich_batch_device*).
 *
 * Every stage in front ends at a CSR of deliveries keyed by MESSAGE.  The consumer of a delivery
 * is a subscriber's connection process.  Paths are relative to the reference checkout
 * (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   emqx_broker:do_dispatch/2                          apps/emqx/src/emqx_broker.erl:500-524
 *     one `SubPid ! {deliver, Topic, Msg}` per delivery
 *   emqx_connection:handle_msg({deliver, ...})         apps/emqx/src/emqx_connection.erl:505-509
 *   emqx_ws_connection                                 apps/emqx/src/emqx_ws_connection.erl:402-403
 *     -> emqx_misc:drain_deliver/1                     apps/emqx/src/emqx_misc.erl:158-172
 *          up to active_n more delivers are taken from the mailbox: the connection regroups
 *   emqx_channel:handle_deliver/2                      apps/emqx/src/emqx_channel.erl:776-807
 *     works on that list per subscriber
 *
 * This stage is the transpose: the message-major CSR becomes a subscriber-major one, one inbox
 * per subscriber that received anything, its deliveries in batch order.  The caller does one
 * id-to-pid lookup and one send per inbox; the list it sends is the list handle_deliver/2 takes.
 *
 * Let perm be the STABLE sort of the delivery positions d = 0..total-1 by subs[d] (ascending
 * subscriber id, ties in ascending d).  Then box_msgs[k] is the message of perm[k] (the largest
 * i with offsets[i] <= perm[k]), box_filters[k] = filters[perm[k]] (SHARED and RETRY bits
 * untouched), box_opts / box_subids likewise, box_src[k] = perm[k]; inbox_subs[m] are the
 * distinct subscriber ids, ascending, and inbox_offsets[m+1] their extents in the box_* arrays.
 * Inside an inbox the deliveries are in message order, within a message in fan-out order: the
 * order in which one publisher's sends would have reached the mailbox.  The result is a pure
 * function of the input: two runs are byte-identical.
 *
 * Kept by the caller: the pid lookup and the send, active_n slicing of an inbox.  Inflight and
 * mqueue admission of every inbox is the next stage (emqx_window.h).
 *
 * Conventions as in emqx_match.h: int status, EMQX_* codes.
 *
 * Threading: the calls on one handle share its device scratch and are ordered by the handle
 * (each call starts after the handle's previous call has finished on the device, whichever
 * streams they use).  Concurrent callers take one handle each.
 */
#ifndef EMQX_INBOX_H
#define EMQX_INBOX_H

#include <stdint.h>

#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_inbox emqx_inbox;

#define EMQX_INBOX_HOST_ONLY (-2)              /* `device` of a handle without a device      */
#define EMQX_INBOX_MAX_SUB_LIMIT (1ull << 32)  /* sub_limit lies in 1..2^32                  */

/* summary[8]: [0] flags, [1] deliveries (offsets[n]), [2] inboxes m, [3] the longest inbox,
 * [4] messages with at least one delivery, [5..7] 0. */
#define EMQX_INBOX_SUMMARY_WORDS 8
#define EMQX_INBOX_F_BOX_OVERFLOW 0x1u  /* m > cap_boxes: [2] = the capacity needed, the box_* arrays complete,  */
                                        /* inbox_subs / inbox_offsets hold the first cap_boxes inboxes           */
                                        /* (cap_boxes + 1 offsets)                                               */
#define EMQX_INBOX_F_INPUT_REFUSED 0x2u /* offsets[n] > cap_in, offsets[n] >= 2^32 or n >= 2^32: nothing read    */
                                        /* or written but the summary                                            */
#define EMQX_INBOX_F_BAD_SUB 0x4u       /* some subs[d] >= sub_limit: [2] = [3] = 0, the outputs unspecified     */

/* One group call.  Every pointer is host memory for emqx_inbox_group_batch and
 * emqx_inbox_group_host, device memory for the _device forms.
 *
 * In:  the delivery CSR as the fan-out or the enrich stage's compacted form writes it:
 *      offsets[n+1] with offsets[0] = 0, subs[] and filters[] of capacity cap_in, optionally
 *      opts[] (one byte a delivery) and subids[]; sub_limit (1..2^32): every subscriber id is
 *      below it (it sets the number of sort passes).
 * Out: box_msgs[], box_filters[] (required when cap_in > 0), box_opts[], box_subids[], box_src[]
 *      (each optional: NULL skips it; box_opts needs opts, box_subids needs subids), all of
 *      capacity cap_in, the first offsets[n] entries written; inbox_subs[cap_boxes],
 *      inbox_offsets[cap_boxes + 1].  A caller that sizes cap_boxes = min(cap_in, sub_limit)
 *      never sees BOX_OVERFLOW.  The outputs are distinct from the inputs and from each other. */
typedef struct emqx_inbox_batch {
  const uint64_t* offsets;
  const uint32_t* subs;
  const uint32_t* filters;
  const uint8_t* opts;
  const uint32_t* subids;
  uint64_t n;
  uint64_t cap_in;
  uint64_t sub_limit;
  uint32_t* box_msgs;
  uint32_t* box_filters;
  uint8_t* box_opts;
  uint32_t* box_subids;
  uint32_t* box_src;
  uint32_t* inbox_subs;
  uint64_t* inbox_offsets;
  uint64_t cap_boxes;
} emqx_inbox_batch;

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_inbox_stats) before the call. */
typedef struct emqx_inbox_stats {
  uint64_t size;          /* in: sizeof(emqx_inbox_stats) of the caller; out: bytes written */
  uint64_t cap_in;        /* deliveries the reserved scratch takes                          */
  uint64_t sub_limit;     /* the largest sub_limit it takes                                 */
  uint64_t scratch_bytes; /* device memory held                                             */
  uint64_t path;          /* tuning key "path"                                              */
  uint64_t calls;         /* group calls so far, all forms                                  */
  uint64_t last_passes;   /* sort passes of the last call (8-bit digits of sub_limit)       */
  double last_call_ms;    /* time of the last synchronous call                              */
} emqx_inbox_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_INBOX_HOST_ONLY: a handle that answers
 * emqx_inbox_group_host alone; its batch entry points return EMQX_EDEVICE (nothing ever falls
 * back to the host silently). */
int emqx_inbox_create(int32_t device, emqx_inbox** out);
int emqx_inbox_destroy(emqx_inbox* h);

/* Sizes the device scratch for calls of up to cap_in deliveries (< 2^32) and subscriber ids
 * below sub_limit.  It only grows; it waits for the handle's call in flight first.  EMQX_EINVAL:
 * cap_in >= 2^32, sub_limit outside 1..2^32. */
int emqx_inbox_reserve(emqx_inbox* h, uint64_t cap_in, uint64_t sub_limit);

/* Host buffers, evaluated on the device (the scratch grows as needed).  EMQX_EINVAL:
 * offsets[0] != 0, decreasing offsets, a refused input, a subscriber >= sub_limit.  *n_boxes
 * (may be NULL) = m; m > cap_boxes: EMQX_EOVERFLOW, *n_boxes = the capacity needed, outputs as
 * the flag says.  summary_out (host, may be NULL) receives the 8 summary words. */
int emqx_inbox_group_batch(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out);
/* Device buffers, on `stream` (NULL: the handle's own, ordered after the device's null stream);
 * synchronizes the stream.  The delivery count is read on the device.  The scratch grows as
 * needed.  Returns as above; a refused input or a bad subscriber: EMQX_EINVAL with the summary
 * flag. */
int emqx_inbox_group_batch_device(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out,
                                  void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains behind
 * emqx_fanout_batch_device_async or emqx_deliver_enrich_batch_device_async on the same stream
 * with no host read.  The delivery count is read on the device as offsets[n].  `summary` (>= 8
 * uint64_t, device or host-pinned memory) is written last, with plain stores.  Whatever the
 * device buffers hold, no access leaves them.  EMQX_EOVERFLOW, nothing enqueued: the reserved
 * scratch (emqx_inbox_reserve) is smaller than cap_in or sub_limit.  Everything else is
 * reported through the summary alone. */
int emqx_inbox_group_batch_device_async(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* summary, void* stream);
/* The same outputs computed on the calling thread: the per-call path and the checker of the
 * batch path.  Returns as emqx_inbox_group_batch. */
int emqx_inbox_group_host(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out);

/* Keys: "path": 0 the stage's own radix passes (default), 1 the library radix sort followed by one
 * gather kernel (the yardstick; both produce the same bytes); "max_blocks" (1..16384, default
 * 16384): the grid cap of every pass whose blocks stride (the histogram and scatter of every radix
 * pass, the heads, the starts, path 1's prep and gather, and the longest pass, which never takes
 * more than 1024), the blocks stride over the tiles or rows beyond it; "scan_chunk" (1..1024,
 * default 1024): the tile totals the one-block scans take per carry step (tests lower both to make
 * the blocks stride and the scans carry at small shapes; the same bytes at every value).  Both are
 * read when a call is enqueued; a host-only handle accepts and ignores them.  EMQX_EINVAL out of
 * range, EMQX_ENOTFOUND for unknown keys. */
int emqx_inbox_set_tuning(emqx_inbox* h, const char* key, int64_t value);
int emqx_inbox_stats_get(emqx_inbox* h, emqx_inbox_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_INBOX_H */
