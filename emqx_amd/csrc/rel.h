// Shared pieces of the rel stage (include/emqx_rel.h): the packing of an entry of
// the awaiting table, the classification of a session, the verdict of one step of the fold and the
// expiry predicate.  Everything here is __host__ __device__: the kernels (rel_kernels.hip) and the
// host evaluator (rel.cpp) run the same functions.  Unlike the ack fold this one has no closed
// form: a PUBLISH lands or not by the row's count at that moment, which every earlier verdict of
// the session moves, so both sides step through a session's events in order.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RL_HD __host__ __device__
#else
#define RL_HD
#endif

namespace emqx {

constexpr uint32_t RL_F_INPUT_REFUSED = 2u, RL_F_BAD_SUB = 4u, RL_F_ROW_SMALL = 8u, RL_F_BAD_TS = 0x10u;
// words of the summaries
enum {
  RL_S_FLAGS = 0, RL_S_TOTAL = 1, RL_S_BOXES = 2,
  RL_R_ROUTED = 3, RL_R_RELEASED = 4, RL_R_IN_USE = 5, RL_R_NOT_FOUND = 6, RL_R_EXCEEDED = 7,  // run
  RL_X_OK = 1, RL_X_EXPIRED = 3, RL_X_REMAINING = 4, RL_X_ARMED = 5,                           // expire
  RL_S_WORDS = 8
};

constexpr uint32_t RL_BLOCK = 256;                   // threads per block
constexpr uint32_t RL_ROWS = 4;                      // consecutive events per thread of the route passes
constexpr uint32_t RL_TILE = RL_BLOCK * RL_ROWS;     // events per tile of the route passes (1024)
constexpr uint64_t RL_MAX_TOTAL = (1ull << 32) - 1;  // session indices are 32-bit
constexpr uint64_t RL_MAX_EVENTS = (1ull << 31) - 1;
constexpr uint32_t RL_MAX_BLOCKS = 4096;
constexpr uint32_t RL_SCAN_BLOCK = 1024;
constexpr uint32_t RL_MAX_W = 128;
constexpr uint32_t RL_MIN_LANES = 4, RL_MAX_LANES = 64;

// kind of an event, the verdict byte (EMQX_REL_*)
constexpr uint32_t RL_PUBLISH = 1, RL_PUBREL = 2, RL_DIRECT = 3;
constexpr uint8_t RL_OK = 1, RL_IN_USE = 2, RL_NOT_FOUND = 3, RL_EXCEEDED = 4, RL_NO_SESSION = 5, RL_PASS = 6, RL_ROW_SMALL = 7,
                  RL_BAD_KIND = 8, RL_IDLE = 9;
constexpr uint32_t RL_NO_TIMEOUT = 0xFFFFFFFFu;
constexpr uint64_t RL_TS_LIMIT = 1ull << 45;
// what the stage reads of the window stage's 32-byte record: its flags word
constexpr uint32_t RL_PRESENT = 1u, RL_CONNECTED = 2u, RL_PASSF = 8u;
constexpr uint32_t RL_REC_WORDS = 8, RL_REC_FLAGS = 5;

// An entry: ts_ms << 17 | 1 << 16 | pkt_id; 0 is empty, every other word is an entry.
RL_HD constexpr uint64_t rl_entry(uint64_t ts_ms, uint32_t pkt_id) { return (ts_ms << 17) | (1ull << 16) | (pkt_id & 0xFFFFu); }
RL_HD inline bool rl_hit(uint64_t e, uint32_t pkt_id) { return e != 0 && (static_cast<uint32_t>(e) & 0xFFFFu) == pkt_id; }
RL_HD inline uint64_t rl_entry_ts(uint64_t e) { return e >> 17; }
// The stamp an entry stores for `ts`; *bad: it was clamped.
RL_HD inline uint64_t rl_stamp(uint64_t ts, bool* bad) {
  *bad = ts >= RL_TS_LIMIT;
  return *bad ? RL_TS_LIMIT - 1 : ts;
}

RL_HD inline bool rl_w_ok(uint64_t w) { return w == 8 || w == 16 || w == 32 || w == 64 || w == 128; }

// The lanes that own one session in the run fold: max(4, W / 16) by measurement (DESIGN.md §3.17:
// with a few events a session, fewer lanes a session put more sessions into a wave), or the
// override lowered to W / 2 capped at 64 (every lane holds at least one 16-byte pair of the row).
RL_HD inline uint32_t rl_lanes(uint32_t w, uint32_t override_lanes) {
  const uint32_t most = w / 2 < RL_MAX_LANES ? w / 2 : RL_MAX_LANES;
  if (override_lanes) return override_lanes < most ? override_lanes : most;
  return w / 16 > RL_MIN_LANES ? w / 16 : RL_MIN_LANES;
}
RL_HD inline bool rl_lanes_ok(int64_t v) { return v == 0 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64; }

// 0: the session takes events; else the verdict of every one of its events.  `limit`: the
// session's max_awaiting_rel, 0 = infinity.
RL_HD inline uint8_t rl_session(bool sub_ok, uint32_t flags, uint32_t limit, uint32_t w) {
  if (!sub_ok || !(flags & RL_PRESENT)) return RL_NO_SESSION;
  if (flags & RL_PASSF) return RL_PASS;
  return (limit == 0 || limit > w) ? RL_ROW_SMALL : 0;
}
// The status of a session in an expire call, RL_OK: it is swept.
RL_HD inline uint8_t rl_expire_session(bool sub_ok, uint32_t flags, bool channel_rule) {
  if (!sub_ok || !(flags & RL_PRESENT)) return RL_NO_SESSION;
  if (flags & RL_PASSF) return RL_PASS;
  return (channel_rule && !(flags & RL_CONNECTED)) ? RL_IDLE : RL_OK;
}

// One step of the fold (the table of include/emqx_rel.h): `cnt` the non-empty entries of the row
// and `present` whether it holds the id, both at that moment.
RL_HD inline uint8_t rl_verdict(uint32_t kind, uint32_t cnt, uint32_t limit, bool present) {
  if (kind == RL_DIRECT) return RL_OK;
  if (kind == RL_PUBLISH) return cnt >= limit ? RL_EXCEEDED : present ? RL_IN_USE : RL_OK;
  if (kind == RL_PUBREL) return present ? RL_OK : RL_NOT_FOUND;
  return RL_BAD_KIND;
}
RL_HD inline bool rl_routed(uint32_t kind, uint8_t verdict) { return verdict == RL_OK && (kind == RL_PUBLISH || kind == RL_DIRECT); }

// expire_awaiting_rel/2: age(Now, Ts) >= Timeout, a plain signed difference.
RL_HD inline bool rl_expired(uint64_t e, uint64_t now_ms, uint32_t timeout) {
  if (e == 0 || timeout == RL_NO_TIMEOUT) return false;
  return static_cast<int64_t>(now_ms - rl_entry_ts(e)) >= static_cast<int64_t>(timeout);
}

RL_HD inline uint64_t rl_tiles(uint64_t total) { return (total + RL_TILE - 1) / RL_TILE; }

#if defined(__HIPCC__)
// Arguments of the device passes of a run call; the first block is emqx_rel_run_args'.
struct RlRunArgs {
  const uint32_t* ev_subs;
  const uint64_t* ev_offsets;
  const uint32_t* events;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  const uint64_t* ts;
  const uint32_t* src;
  const uint32_t* sessions;  // RL_REC_WORDS words a record
  uint64_t sub_limit;
  uint64_t* rel;
  uint32_t w;
  uint64_t now_ms;
  uint32_t max_awaiting;
  const uint32_t* maxes;
  uint8_t* verdicts;
  uint32_t* out_route;
  uint32_t* out_counts;
  uint8_t* out_arm;
  // scratch of the handle
  uint32_t* tile_tot;       // [tiles] routed events of a tile, then their exclusive scan
  unsigned long long* ctr;  // [RL_S_WORDS] counters, zeroed by the init kernel
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t lanes;           // lanes a session of the fold, already resolved for w
  uint32_t max_blocks;      // grid cap of every pass whose blocks stride
  uint32_t scan_chunk;      // tile totals per carry step of the scan, 1..RL_SCAN_BLOCK
};
// Of an expire call.
struct RlExpArgs {
  const uint32_t* subs;
  const uint64_t* n_boxes;
  uint64_t m, cap_boxes;
  const uint32_t* sessions;
  uint64_t sub_limit;
  uint64_t* rel;
  uint32_t w;
  uint64_t now_ms;
  uint32_t timeout_ms;
  const uint32_t* timeouts;
  uint64_t channel_rule;
  uint8_t* out_status;
  uint32_t* out_counts;
  unsigned long long* ctr;
  uint64_t* summary;
  uint32_t max_blocks;
};
int rl_launch_run(const RlRunArgs& a, void* stream);
int rl_launch_expire(const RlExpArgs& a, void* stream);
#endif

}  // namespace emqx
