// Shared pieces of the mqueue stage (include/emqx_mqueue.h): the ring of queued
// messages a session owns and the closed forms of emqx_mqueue:in/2 over an inbox and of
// emqx_session:dequeue/1 over a row.
//
// Put.  The window stage (window.h) folds in/2 over the e queue candidates of an inbox whose queue
// holds L of at most M entries (0 < M, L <= M): the first M - L candidates find room, every later
// one finds the queue full and evicts its oldest entry, v = max(0, L + e - M) evictions in all, and
// marks each of those candidates EMQX_W_EVICTS: #EVICTS = v.  The oldest entry is an old one for the
// first L evictions and a candidate of this very batch after that, and those candidates, the first
// qd = max(0, e - M), are the ones marked QUEUED_DROPPED: #QUEUED_DROPPED = qd.  So
//     evicted_old = min(L, v) = v - qd = #EVICTS - #QUEUED_DROPPED
// (e >= M: v - qd = L <= v; e < M: qd = 0 and v < L).  With M = 0 or L > M nothing is ever evicted
// and both counts are 0.  The stage takes the two counts from the verdicts and bounds the result by
// L, so that whatever the verdicts hold the new queue is the old one without a prefix, then the
// QUEUED deliveries in order (mq_put_plan).  The j-th evicting delivery with j < L dropped the old
// entry of logical index j.
//
// Take.  dequeue/3 pops one message a step: an expired one is dropped and costs nothing, a QoS-0
// one is delivered and costs nothing, any other is delivered and costs one of the Cnt = batch_n/1
// steps; it stops when Cnt reaches 0 or the queue is empty.  With c_i the inclusive prefix count of
// the counting entries, entry i is consumed iff the count BEFORE it is below n (mq_consumed): a
// predicate per entry over one prefix count, no walk.  A consumed entry's place among the session's
// items is its logical index, its packet id follows from the count before it.
// Everything here is __host__ __device__: the kernels (mqueue_kernels.hip) and the host evaluator
// (mqueue.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "ack.h"
#include "window.h"

namespace emqx {

constexpr uint32_t MQ_F_INPUT_REFUSED = 2u, MQ_F_BAD_SUB = 4u, MQ_F_OUTPUT_FULL = 8u, MQ_F_BAD_REF = 0x10u, MQ_F_BAD_RING = 0x20u,
                   MQ_F_ROW_FULL = 0x40u, MQ_F_LEN_MISMATCH = 0x80u;
// words of the summaries
enum {
  MQ_S_FLAGS = 0, MQ_S_TOTAL = 1, MQ_S_BOXES = 2,
  MQ_P_STORED = 3, MQ_P_EVICTED = 4, MQ_P_UNSTORED = 5, MQ_P_FULL_ROWS = 6, MQ_P_MISMATCH = 7,  // put
  MQ_T_OKS = 1, MQ_T_ITEMS = 3, MQ_T_SENDS = 4, MQ_T_SENDS0 = 5, MQ_T_EXPIRED = 6, MQ_T_MISMATCH = 7,  // take
  MQ_S_WORDS = 8,
  // behind the counters in the scratch: the take scan's total and its overflow decision
  MQ_C_TOTAL = 8, MQ_C_FULL = 9, MQ_C_WORDS = 10
};

constexpr uint32_t MQ_MIN_Q = 8, MQ_MAX_Q = 1024;
constexpr uint32_t MQ_NO_REF = 0xFFFFFFFFu;
constexpr uint8_t MQ_EXPIRED = 10;
constexpr uint64_t MQ_NO_EXPIRY = ~0ull;
constexpr uint64_t MQ_MAX_NOW = 1ull << 45;
constexpr uint32_t MQ_ROWS = 4;                   // consecutive deliveries per thread (put)
constexpr uint32_t MQ_TILE = AK_BLOCK * MQ_ROWS;  // deliveries per tile (1024)
constexpr uint32_t MQ_MAX_GROUP = 8;              // lanes a session at most (take): 16 entries a trip
// the session record as eight words (emqx_window_session)
constexpr uint32_t MQ_REC_MQ_LEN = 2, MQ_REC_NEXT_PKT = 4;

AK_HD inline bool mq_q_ok(uint64_t q) { return q >= MQ_MIN_Q && q <= MQ_MAX_Q && (q & (q - 1)) == 0; }

// An entry as two words: ref, then opts in the low byte (the three bytes above it are written 0).
AK_HD inline uint32_t mq_word1(uint8_t opts) { return opts; }

// A header as the stage reads it; *bad: it was malformed.
AK_HD inline void mq_header(uint32_t head, uint32_t len, uint32_t q, uint32_t* h, uint32_t* L, bool* bad) {
  *bad = head >= q || len > q;
  *h = head & (q - 1);
  *L = len < q ? len : q;
}

// What a verdict byte adds to an inbox's three counts.
AK_HD inline bool mq_is_queued(uint8_t v) { return (v & AK_W_MASK) == WN_QUEUED; }
AK_HD inline bool mq_is_qdropped(uint8_t v) { return (v & AK_W_MASK) == WN_QUEUED_DROPPED; }
AK_HD inline bool mq_evicts(uint8_t v) { return (v & WN_EVICTS) != 0; }

// The plan of an inbox: where its r-th QUEUED delivery goes and what its row becomes.
struct MqPlan {
  uint32_t start;     // physical index of the first survivor, (h + L) % q
  uint32_t room;      // survivors the row takes, q - (L - ev); 0 for a subscriber the table lacks
  uint32_t head, len; // the header after the call
  uint32_t ev, stored, unstored;
};
AK_HD inline MqPlan mq_put_plan(bool ok, uint32_t h, uint32_t L, uint32_t q, uint32_t s, uint32_t x, uint32_t qd) {
  MqPlan p{0, 0, 0, 0, 0, 0, s};
  if (!ok) return p;
  const uint32_t cand = x > qd ? x - qd : 0u;
  p.ev = cand < L ? cand : L;
  const uint32_t kept = L - p.ev;
  p.room = q - kept;
  p.start = (h + L) & (q - 1);
  p.stored = s < p.room ? s : p.room;
  p.unstored = s - p.stored;
  p.head = (h + p.ev) & (q - 1);
  p.len = kept + p.stored;
  return p;
}

// batch_n/1.
AK_HD inline uint32_t mq_budget(uint32_t inflight_max, uint32_t inflight) { return ak_room(inflight_max, inflight); }

// Whether the entry is expired; *bad_ref: deadlines are given and the ref is not below ref_limit.
AK_HD inline bool mq_expired(uint32_t ref, uint64_t now, const uint64_t* deadlines, uint64_t ref_limit, bool* bad_ref) {
  *bad_ref = false;
  if (!deadlines) return false;
  if (ref >= ref_limit) {
    *bad_ref = true;
    return false;
  }
  return now > deadlines[ref];
}
// Whether a live entry costs one step of the budget.
AK_HD inline bool mq_counting(uint8_t opts, bool expired) { return !expired && (opts & AK_O_QOS) != 0; }
// Entry i is consumed iff the counting entries before it are fewer than n.
AK_HD inline bool mq_consumed(uint32_t before, uint32_t n) { return before < n; }
// The verdict and the packet id of a consumed entry.
AK_HD inline uint8_t mq_item(uint8_t opts, bool expired, uint32_t next_pkt_id, uint32_t before, uint16_t* id) {
  *id = 0;
  if (expired) return MQ_EXPIRED;
  if ((opts & AK_O_QOS) == 0) return WN_SEND_QOS0;
  const uint32_t pkt0 = (next_pkt_id - 1u) % WN_PKT_MOD;
  *id = static_cast<uint16_t>((pkt0 + before % WN_PKT_MOD) % WN_PKT_MOD + 1u);
  return WN_SEND;
}
// next_pkt_id after `sends` ids were given out.
AK_HD inline uint32_t mq_next_pkt(uint32_t next_pkt_id, uint32_t sends) {
  if (!sends) return next_pkt_id;
  const uint32_t pkt0 = (next_pkt_id - 1u) % WN_PKT_MOD;
  return static_cast<uint32_t>((pkt0 + static_cast<uint64_t>(sends)) % WN_PKT_MOD) + 1u;
}

AK_HD inline uint64_t mq_tiles(uint64_t total) { return (total + MQ_TILE - 1) / MQ_TILE; }
// Lanes a session, sessions a block and trip, and the trips ("tiles") of m sessions (take).
AK_HD inline uint32_t mq_group(uint32_t q) { return q / 2 < MQ_MAX_GROUP ? q / 2 : MQ_MAX_GROUP; }
AK_HD inline uint32_t mq_rows_per_block(uint32_t q) { return AK_BLOCK / mq_group(q); }
AK_HD inline uint64_t mq_take_tiles(uint64_t m, uint32_t q) { return (m + mq_rows_per_block(q) - 1) / mq_rows_per_block(q); }

#if defined(__HIPCC__)
// Arguments of the device passes of a put call; the first block is emqx_mqueue_put_args'.
struct MqPutArgs {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  const uint8_t* verdicts;
  const uint32_t* refs;
  const uint32_t* sessions;  // AK_REC_WORDS words a record, or NULL
  uint2* ring;
  uint2* heads;
  uint32_t q;
  uint64_t sub_limit;
  uint2* out_evicted;
  uint32_t* out_unstored;
  // scratch of the handle, sized for cap_in deliveries and cap_boxes inboxes
  uint64_t* tile_sx;        // [tiles] QUEUED (low) and EVICTS (high) counts of a tile, then their exclusive scan
  uint32_t* tile_qd;        // [tiles] QUEUED_DROPPED of a tile, then their exclusive scan
  uint64_t* head_pre;       // [cap_boxes + 1] the three counts between the tile's start and the inbox's head (16 bits each)
  uint2* plans;             // [cap_boxes] MqPlan's start and room
  unsigned long long* ctr;  // [MQ_C_WORDS] counters, zeroed by the scan kernel
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks;      // grid cap of every pass whose blocks stride
  uint32_t scan_chunk;      // tile totals per carry step of the scan, 1..AK_SCAN_BLOCK
};
// Of a take call.
struct MqTakeArgs {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes;
  uint32_t* sessions;
  uint64_t sub_limit, update_table;
  const uint2* ring;
  uint2* heads;
  uint32_t q;
  uint64_t now_ms;
  const uint64_t* deadlines;
  uint64_t ref_limit, cap_out;
  uint64_t* out_offsets;
  uint8_t* out_opts;
  uint8_t* out_verdicts;
  uint16_t* out_pkt_ids;
  uint32_t* out_refs;
  uint8_t* out_status;
  uint32_t* out_counts;
  // scratch of the handle
  uint64_t* tile_tot;       // [mq_take_tiles(cap_boxes, MQ_MAX_Q)] items of a tile, then their exclusive scan
  unsigned long long* ctr;  // [MQ_C_WORDS] counters, zeroed by the scan kernel; total and full
  uint64_t* summary;
  uint32_t max_blocks, scan_chunk;
};
int mq_launch_put(const MqPutArgs& a, void* stream);
int mq_launch_take(const MqTakeArgs& a, void* stream);
#endif

}  // namespace emqx
