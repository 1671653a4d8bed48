// Device record and the per-record functions of the route table (include/emqx_route.h,
// DESIGN.md §3.13).  Everything here is __host__ __device__: the kernels (route_kernels.hip) and
// the host evaluator (route.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace emqx {

constexpr uint32_t RT_NODES = 64;
constexpr uint32_t RT_LOCAL = 1u, RT_SHARE = 2u, RT_REMOTE = 4u;
constexpr uint32_t RT_F_FWD_OVERFLOW = 1u, RT_F_INPUT_REFUSED = 2u;
// words of the summary; the device counters continue behind them
enum { RT_S_FLAGS = 0, RT_S_ENTRIES = 1, RT_S_FWD = 2, RT_S_DROPPED = 3, RT_S_FWD_MSGS = 4, RT_S_KEPT = 5,
       RT_S_UNKNOWN = 6, RT_S_FWD_NODES = 7, RT_S_WORDS = 8, RT_C_WORDS = 16 };

// One filter id's dests, 16 bytes, dense by filter id.
struct RtRec {
  uint64_t node_mask;  // bit v: the plain route #route{dest = v}
  uint32_t n_groups;   // distinct groups among the grouped dests {Group, _Node}
  uint32_t spare;
};
static_assert(sizeof(RtRec) == 16, "one 16-byte load");

// do_route/2's three clauses as bits (emqx_broker.erl:254-259).
RT_HD inline uint32_t rt_flags(const RtRec& r, uint32_t local) {
  const uint64_t me = 1ull << local;
  return ((r.node_mask & me) ? RT_LOCAL : 0u) | (r.n_groups ? RT_SHARE : 0u) | ((r.node_mask & ~me) ? RT_REMOTE : 0u);
}

RT_HD inline uint32_t rt_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<uint32_t>(__popcll(x));
#else
  return static_cast<uint32_t>(__builtin_popcountll(x));
#endif
}

// |aggre(lookup_routes(To))|: the plain routes plus the distinct groups (emqx_broker.erl:261-272).
RT_HD inline uint64_t rt_routes(const RtRec& r) { return static_cast<uint64_t>(rt_popc(r.node_mask)) + r.n_groups; }

// The nodes one entry forwards to.
RT_HD inline uint64_t rt_fwd_mask(const RtRec& r, uint32_t local) { return r.node_mask & ~(1ull << local); }

// The record of filter id f; an id the snapshot has no slot for has no dest.
RT_HD inline RtRec rt_record(const RtRec* recs, uint64_t n_slots, uint32_t f) {
  if (f < n_slots) return recs[f];
  return RtRec{0, 0, 0};
}

// Tuning key "scan_chunk": the elements the one-block scans take per carry step, at most this.
constexpr uint32_t RT_SCAN_BLOCK = 1024;

#if defined(__HIPCC__)
constexpr uint32_t RT_BLOCK = 256, RT_ROWS = 8, RT_TILE = RT_BLOCK * RT_ROWS;  // 2 048 entries a tile
constexpr uint32_t RT_PAD_KEY = RT_NODES;  // path 1: sorts behind every node under 7 key bits
constexpr uint32_t RT_SORT_BITS = 7;

RT_HD inline uint64_t rt_tiles(uint64_t total) { return total ? (total + RT_TILE - 1) / RT_TILE : 1; }

// Arguments of the device passes (route_kernels.hip); the pointers are emqx_route_batch's.
struct RtArgs {
  const RtRec* recs;
  uint64_t n_slots;
  uint32_t local;
  uint64_t fwd_nodes;  // the union of every record's forward mask: the node bits worth a ballot
  const uint64_t* offsets;
  const uint32_t* filters;
  uint64_t n, cap_in;
  uint8_t* entry_flags;  // may be NULL
  uint32_t* msg_routes;
  uint64_t* node_offsets;
  uint32_t* fwd_msgs;
  uint32_t* fwd_filters;
  uint64_t cap_fwd;
  uint64_t* local_offsets;  // may be NULL, with local_filters
  uint32_t* local_filters;
  unsigned long long* ctr;  // [RT_C_WORDS] device counters, zero when the first pass starts
  uint64_t* tile_hist;      // [RT_NODES * tiles] node-major forwards of a tile, then their exclusive scan
  uint64_t* tile_routes;    // [tiles] routes of a tile, then the exclusive scan
  uint64_t* tile_kept;      // [tiles] kept entries
  uint64_t* tile_hasfwd;    // [tiles] entries with at least one forward
  uint64_t* tile_fwd;       // [tiles] forwards of a tile over every node (path 1's reservation)
  uint64_t* entry_mask;     // [cap_in] or NULL: pass 1 stores forward mask | kept << local, pass 4 reads it
  uint64_t* head_routes;    // [n + 1] routes of the tile's entries before the head of message i
  uint32_t* head_kf;        // [n + 1] the same for kept (low half) and has-forward (high half)
  uint32_t* sort_key[2];    // path 1: [cap_fwd] node of each forward, unsorted / sorted
  uint64_t* sort_val[2];    // path 1: [cap_fwd] message << 32 | filter
  void* sort_temp;
  uint64_t sort_temp_bytes;
  uint64_t* summary;    // device or host-pinned, written last with plain stores
  uint32_t max_blocks;  // grid cap of the by-tile passes
  uint32_t scan_chunk;  // elements per carry step of the scans, 1..RT_SCAN_BLOCK
};
uint64_t rt_sort_temp_bytes(uint64_t cap_fwd);
int rt_launch(const RtArgs& a, int path, void* stream);
#endif

}  // namespace emqx
