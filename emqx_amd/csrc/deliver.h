// Snapshot layout and the per-delivery predicate of the delivery-options table
// (include/emqx_deliver.h).  Everything here is __host__ __device__: the kernels
// (deliver_kernels.hip) and the host evaluator (deliver.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DV_HD __host__ __device__
#else
#define DV_HD
#endif

namespace emqx {

// The constants of emqx_deliver.h / emqx_match.h, restated for code that includes neither.
constexpr uint32_t DV_KEY_MASK = 0x3FFFFFFFu;  // ~(EMQX_FANOUT_SHARED_BIT | EMQX_FANOUT_RETRY_BIT)
constexpr uint32_t DV_EMPTY = 0xFFFFFFFFu;     // filter of an empty slot: cannot be a filter id
constexpr uint32_t DV_NO_SENDER = 0xFFFFFFFFu;
constexpr uint32_t DV_SUB_QOS = 0x03u, DV_SUB_NL = 0x04u, DV_SUB_RAP = 0x08u, DV_SUB_UPGRADE = 0x10u, DV_SUB_SUBID = 0x20u;
constexpr uint32_t DV_MSG_RETAIN = 0x01u, DV_MSG_RETAINED = 0x02u;
constexpr uint32_t DV_OUT_RETAIN = 0x04u, DV_OUT_NL = 0x08u, DV_OUT_DROP = 0x10u, DV_OUT_NO_SUBOPTS = 0x20u, DV_OUT_BAD = 0x40u;
constexpr uint32_t DV_F_KEPT_OVERFLOW = 1u, DV_F_INPUT_REFUSED = 2u;
// Tuning (emqx_subopts_set_tuning): the largest grid of the by-tile passes, beyond which the
// blocks stride over the tiles, and the tile totals the one-block scan takes per carry step.
constexpr uint32_t DV_MAX_BLOCKS = 16384;
constexpr uint32_t DV_SCAN_BLOCK = 1024;
// words of the device counters / the summary
enum { DV_S_FLAGS = 0, DV_S_TOTAL = 1, DV_S_KEPT = 2, DV_S_DROPPED = 3, DV_S_NO_SUBOPTS = 4, DV_S_QOS0 = 5, DV_S_WORDS = 8 };

// One slot of the open-addressing table: read with one 16-byte load.
struct alignas(16) DvSlot {
  uint32_t filter;  // DV_EMPTY: empty
  uint32_t sub;
  uint32_t opts;    // DV_SUB_*
  uint32_t subid;   // 0 without DV_SUB_SUBID
};

struct DvView {
  const DvSlot* slots;  // [n_slots], at least one of them empty
  uint32_t n_slots;     // >= 1, any number (the home slot is a multiply-shift, not a mask)
  uint32_t max_probe;   // longest probe run of the build: a lookup reads at most this many slots
};

// Home slot of (filter, sub): a 32-bit mix, then Lemire's multiply-shift onto [0, n_slots).
DV_HD inline uint32_t dv_home(uint32_t filter, uint32_t sub, uint32_t n_slots) {
  uint32_t h = filter * 0x9E3779B1u ^ (sub + 0x7F4A7C15u) * 0x85EBCA6Bu;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return static_cast<uint32_t>((static_cast<uint64_t>(h) * n_slots) >> 32);
}

// One slot with one 16-byte load.  On the device the four words are pinned live right behind
// the load: left alone, the compiler loads `filter`, waits, tests it and fetches the other 12
// bytes in a second, dependent round trip (the narrowing match_kernels.hip's load3_masked
// describes).
DV_HD inline DvSlot dv_load(const DvSlot* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4 v = *reinterpret_cast<const uint4*>(p);
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
  return DvSlot{v.x, v.y, v.z, v.w};
#else
  return *p;
#endif
}

// Linear probing, bounded by the longest run of the build: true and the slot when the key is
// present.  The slot index stays below n_slots whatever the key.
DV_HD inline bool dv_lookup(const DvView& v, uint32_t filter, uint32_t sub, DvSlot* out) {
  uint32_t i = dv_home(filter, sub, v.n_slots);
  for (uint32_t k = 0; k < v.max_probe; ++k) {
    const DvSlot s = dv_load(v.slots + i);
    if (s.filter == DV_EMPTY) return false;
    if (s.filter == filter && s.sub == sub) {
      *out = s;
      return true;
    }
    if (++i >= v.n_slots) i = 0;
  }
  return false;
}

// emqx_session:ignore_local/3's predicate (emqx_session.erl:282-290) and enrich_subopts/3
// (:578-598) over get_subopts/2 (:569-576) for one delivery: the EMQX_DELIVER_* byte, *subid.
DV_HD inline uint32_t dv_enrich(const DvView& v, uint32_t sub, uint32_t filter_word, uint32_t qos, uint32_t flags,
                                uint32_t from, uint32_t* subid) {
  *subid = 0;
  if (qos > 2u || (flags & ~(DV_MSG_RETAIN | DV_MSG_RETAINED))) return DV_OUT_BAD;
  const uint32_t retain_in = flags & DV_MSG_RETAIN;
  DvSlot s;
  if (!dv_lookup(v, filter_word & DV_KEY_MASK, sub, &s))  // :575 error -> [], :578 the message as it is
    return qos | (retain_in ? DV_OUT_RETAIN : 0u) | DV_OUT_NO_SUBOPTS;
  uint32_t out = 0;
  if (s.opts & DV_SUB_NL) {  // :579-580 {nl, 1}: set_flag(nl); :284 the drop needs Subscriber =:= Publisher
    out |= DV_OUT_NL;
    if (from == sub && from != DV_NO_SENDER) out |= DV_OUT_DROP;
  }
  const uint32_t sq = s.opts & DV_SUB_QOS;
  out |= (s.opts & DV_SUB_UPGRADE) ? (sq > qos ? sq : qos) : (sq < qos ? sq : qos);  // :583-588
  // :589-594 {rap, 1} keeps the flag; {rap, 0} keeps it only under headers.retained = true
  if (retain_in && ((s.opts & DV_SUB_RAP) || (flags & DV_MSG_RETAINED))) out |= DV_OUT_RETAIN;
  if (s.opts & DV_SUB_SUBID) *subid = s.subid;  // :595-598
  return out;
}

#if defined(__HIPCC__)
// Arguments of the device passes (deliver_kernels.hip); the pointers are emqx_deliver_batch's.
struct DvArgs {
  DvView v;
  const uint64_t* offsets;
  const uint32_t* subs;
  const uint32_t* filters;
  uint64_t n, cap_in;
  const uint8_t* msg_qos;
  const uint8_t* msg_flags;
  const uint32_t* msg_from;
  uint8_t* out_opts;
  uint32_t* out_subids;
  uint64_t* kept_offsets;  // NULL: annotate only
  uint32_t* kept_subs;
  uint32_t* kept_filters;
  uint8_t* kept_opts;
  uint32_t* kept_subids;
  uint64_t cap_kept;
  unsigned long long* ctr;  // [DV_S_WORDS] device counters, zero when the first pass starts
  uint32_t* tile_kept;      // [ceil(cap_in / DV_TILE)] kept deliveries per tile
  uint64_t* tile_base;      // [same] exclusive scan of tile_kept
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks;      // grid cap of the by-tile passes
  uint32_t scan_chunk;      // tile totals per carry step of the scan, 1..DV_SCAN_BLOCK
};
constexpr uint32_t DV_TILE = 256;  // deliveries per tile = threads per block
int dv_launch(const DvArgs& a, void* stream);
#endif

}  // namespace emqx
