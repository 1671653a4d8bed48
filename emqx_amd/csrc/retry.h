// Shared pieces of the retry stage (include/emqx_retry.h): the stamp of an
// inflight slot and the closed form of emqx_session:retry/1 and replay/1 over one row.  The
// reference sorts the window by timestamp and visits it while the entries are old; with one `now`
// that is "every slot with now - ts >= interval", so per slot the fold is a predicate (rt_eval),
// per item a rank among the row's keys (rt_key, ties by slot index) and per session one maximum
// (the largest age among the young slots gives the timer).
// Everything here is __host__ __device__: the kernels (retry_kernels.hip) and the host evaluator
// (retry.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "ack.h"

namespace emqx {

constexpr uint32_t RT_F_INPUT_REFUSED = 2u, RT_F_BAD_SUB = 4u, RT_F_OUTPUT_FULL = 8u, RT_F_BAD_REF = 0x10u, RT_F_UNSTAMPED = 0x20u;
// words of the summaries
enum {
  RT_S_FLAGS = 0, RT_S_ROWS = 1, RT_S_BOXES = 2,
  RT_T_STAMPED = 3, RT_T_CLEARED = 4,                                                        // stamp
  RT_W_ITEMS = 3, RT_W_PUBLISHES = 4, RT_W_PUBRELS = 5, RT_W_EXPIRED = 6, RT_W_UNSTAMPED = 7,  // sweep
  RT_S_WORDS = 8,
  // behind the counters in the scratch: the scan's total and its overflow decision
  RT_C_TOTAL = 8, RT_C_FULL = 9, RT_C_WORDS = 10
};

constexpr uint32_t RT_MODE_RETRY = 0, RT_MODE_REPLAY = 1;
constexpr uint32_t RT_PUBLISH_DUP = 1, RT_PUBREL = 2, RT_EXPIRED = 3;
constexpr uint32_t RT_NO_TIMER = 0xFFFFFFFFu;
constexpr uint64_t RT_NO_EXPIRY = ~0ull;
constexpr uint64_t RT_MAX_INTERVAL = 1ull << 31, RT_MAX_NOW = 1ull << 45;
constexpr uint32_t RT_TS_SHIFT = 19, RT_PHASE_SHIFT = 16;
constexpr uint64_t RT_DUP = 1ull << 18;
constexpr uint64_t RT_NO_KEY = ~0ull;  // the key of a slot that is no item: above every key

// A stamp: ts_ms << 19 | dup << 18 | phase << 16 | pkt_id.
AK_HD inline uint64_t rt_stamp(uint64_t ts, bool dup, uint32_t word0) {
  return (ts << RT_TS_SHIFT) | (dup ? RT_DUP : 0ull) | (static_cast<uint64_t>(ak_phase(word0) & 3u) << RT_PHASE_SHIFT) | (word0 & 0xFFFFu);
}
AK_HD inline uint64_t rt_ts(uint64_t stamp) { return stamp >> RT_TS_SHIFT; }
// Whether the stamp is the slot's: the slot is not EMPTY and phase and pkt_id agree.  The slot's
// phase is compared in full, so a phase above 3 owns no stamp.
AK_HD inline bool rt_belongs(uint64_t stamp, uint32_t word0) {
  return ak_phase(word0) != AK_EMPTY && static_cast<uint32_t>(stamp & 0x3FFFFull) == (word0 & 0x00FFFFFFu);
}

// The stamp call: what the slot's stamp becomes.
AK_HD inline uint64_t rt_stamp_next(uint32_t word0, uint64_t stamp, uint64_t now) {
  if (ak_phase(word0) == AK_EMPTY) return 0;
  return rt_belongs(stamp, word0) ? stamp : rt_stamp(now, false, word0);
}

// The interval of a session: intervals[sub] or the call's, at most 2^31.
AK_HD inline uint32_t rt_interval(const uint32_t* intervals, uint64_t sub, uint64_t interval_ms) {
  const uint64_t v = intervals ? intervals[sub] : interval_ms;
  return static_cast<uint32_t>(v < RT_MAX_INTERVAL ? v : RT_MAX_INTERVAL);
}

// Whether the slot is an item of its session's sweep; the count pass and the emit pass agree
// because both ask this.
AK_HD inline bool rt_is_item(uint32_t mode, uint32_t word0, uint64_t stamp, uint64_t now, uint32_t interval) {
  if (ak_phase(word0) == AK_EMPTY) return false;
  if (mode == RT_MODE_REPLAY) return true;
  const uint64_t ts = rt_belongs(stamp, word0) ? rt_ts(stamp) : now;
  return static_cast<int64_t>(now) - static_cast<int64_t>(ts) >= static_cast<int64_t>(interval);
}

// One slot of an OK session under a sweep.
struct RtSlot {
  uint32_t kind;        // 0: no item, else RT_PUBLISH_DUP / RT_PUBREL / RT_EXPIRED
  uint32_t young_age;   // max(0, now - ts) of a young slot, else 0 (below the interval)
  uint64_t key;         // the item's place in the row's order, RT_NO_KEY when it is none
  uint64_t stamp_after; // what the stamp becomes (retry mode, when the call is not full)
  bool nonempty, unstamped, bad_ref;
};

AK_HD inline RtSlot rt_eval(uint32_t mode, uint32_t word0, uint32_t ref, uint64_t stamp, uint64_t now, uint32_t interval,
                            const uint64_t* deadlines, uint64_t ref_limit) {
  RtSlot e{0, 0, RT_NO_KEY, stamp, false, false, false};
  const uint32_t phase = ak_phase(word0);
  if (phase == AK_EMPTY) return e;
  e.nonempty = true;
  const uint32_t plain = phase == AK_AWAIT ? RT_PUBREL : RT_PUBLISH_DUP;
  if (mode == RT_MODE_REPLAY) {
    e.kind = plain;
    e.key = word0 & 0xFFFFu;
    return e;
  }
  e.unstamped = !rt_belongs(stamp, word0);
  const uint64_t ts = e.unstamped ? now : rt_ts(stamp);
  const int64_t age = static_cast<int64_t>(now) - static_cast<int64_t>(ts);
  if (age < static_cast<int64_t>(interval)) {  // young
    e.young_age = age > 0 ? static_cast<uint32_t>(age) : 0u;
    if (e.unstamped) e.stamp_after = rt_stamp(now, false, word0);
    return e;
  }
  e.kind = plain;
  e.key = (ts << 16) | (word0 & 0xFFFFu);
  if (plain == RT_PUBLISH_DUP && deadlines) {
    if (ref >= ref_limit) e.bad_ref = true;
    else if (now > deadlines[ref]) e.kind = RT_EXPIRED;
  }
  e.stamp_after = e.kind == RT_EXPIRED ? 0ull : rt_stamp(now, plain == RT_PUBLISH_DUP, word0);
  return e;
}

// The first word of an item: pkt_id | kind << 16 | qos << 24 (the second is the slot's ref).
AK_HD inline uint32_t rt_item_word0(uint32_t word0, uint32_t kind) { return (word0 & 0xFF00FFFFu) | (kind << 16); }

// The timer of an OK session: `any` whether the row had an entry at entry, `young_age` the largest
// rt_eval().young_age of the row.
AK_HD inline uint32_t rt_timer(uint32_t mode, bool any, uint32_t interval, uint32_t young_age) {
  return (mode == RT_MODE_REPLAY || !any) ? RT_NO_TIMER : interval - young_age;
}

// Rows a block takes per trip, and the trips ("tiles") of m rows.
AK_HD inline uint32_t rt_rows_per_block(uint32_t w) { return AK_BLOCK / (w / 2); }
AK_HD inline uint64_t rt_tiles(uint64_t m, uint32_t w) { return (m + rt_rows_per_block(w) - 1) / rt_rows_per_block(w); }

#if defined(__HIPCC__)
// Arguments of the device passes of a stamp call; the first block is emqx_retry_stamp_args'.
struct RtStampArgs {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes;
  const uint2* slots;
  uint64_t* stamps;
  uint32_t w;
  uint64_t sub_limit, now_ms;
  // scratch of the handle
  unsigned long long* ctr;  // [RT_C_WORDS] counters, zeroed by the init kernel
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks;      // grid cap of the pass over the rows
};
// Of a sweep call.
struct RtSweepArgs {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes;
  uint32_t* sessions;  // AK_REC_WORDS words a record
  uint64_t sub_limit, update_table;
  uint2* slots;
  uint64_t* stamps;
  uint32_t w;
  uint64_t now_ms, interval_ms;
  const uint32_t* intervals;
  const uint64_t* deadlines;
  uint64_t ref_limit;
  uint32_t mode;
  uint64_t cap_out;
  uint64_t* out_offsets;
  uint2* out_items;
  uint8_t* out_status;
  uint32_t* out_counts;
  uint32_t* out_timers;
  // scratch of the handle
  uint64_t* tile_tot;       // [rt_tiles(cap_boxes, w)] items of a tile, then their exclusive scan
  unsigned long long* ctr;  // [RT_C_WORDS] counters, zeroed by the scan kernel; total and full
  uint64_t* summary;
  uint32_t max_blocks;  // grid cap of the count and the emit pass
  uint32_t scan_chunk;  // tile totals per carry step of the scan, 1..AK_SCAN_BLOCK
};
int rt_launch_stamp(const RtStampArgs& a, void* stream);
int rt_launch_sweep(const RtSweepArgs& a, void* stream);
#endif

}  // namespace emqx
