// Shared pieces of the inbox stage (include/emqx_inbox.h): the digit and pass
// arithmetic from sub_limit and the constants; the message lookup is stage_common.h's csr_find.
// Everything here is __host__ __device__: the kernels (inbox_kernels.hip) and the host side
// (inbox.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IB_HD __host__ __device__
#else
#define IB_HD
#endif

namespace emqx {

constexpr uint32_t IB_F_BOX_OVERFLOW = 1u, IB_F_INPUT_REFUSED = 2u, IB_F_BAD_SUB = 4u;
// words of the summary
enum { IB_S_FLAGS = 0, IB_S_TOTAL = 1, IB_S_BOXES = 2, IB_S_LONGEST = 3, IB_S_MSGS = 4, IB_S_WORDS = 8 };

constexpr uint32_t IB_DIGIT_BITS = 8;                    // one pass sorts by one 8-bit digit
constexpr uint32_t IB_RADIX = 1u << IB_DIGIT_BITS;       // 256 buckets a pass
constexpr uint32_t IB_MAX_PASSES = 4;                    // 32 key bits
constexpr uint32_t IB_BLOCK = 256;                       // threads per block = deliveries per row of a tile
constexpr uint32_t IB_ROWS = 8;                          // rows per tile
constexpr uint32_t IB_TILE = IB_BLOCK * IB_ROWS;         // deliveries per tile of every pass (2048)
constexpr uint64_t IB_MAX_TOTAL = (1ull << 32) - 1;      // positions and message indices are 32-bit
constexpr uint64_t IB_MAX_SUB_LIMIT = 1ull << 32;
// Tuning (emqx_inbox_set_tuning): the largest grid of the by-tile and by-row passes, beyond which
// the blocks stride, and the tile totals a one-block scan takes per carry step.
constexpr uint32_t IB_MAX_BLOCKS = 16384;
constexpr uint32_t IB_LONGEST_BLOCKS = 1024;             // the longest pass never takes more
constexpr uint32_t IB_SCAN_BLOCK = 1024;

// Key bits that can differ below sub_limit (1..2^32): ceil(log2(sub_limit)).
IB_HD inline uint32_t ib_key_bits(uint64_t sub_limit) {
  uint32_t b = 0;
  while (b < 32 && (1ull << b) < sub_limit) ++b;
  return b;
}

// LSD passes over 8-bit digits, lowest first: 1..4 (a limit of 1 or 2 still takes one pass,
// which is what moves the payloads).
IB_HD inline uint32_t ib_passes(uint64_t sub_limit) {
  const uint32_t b = ib_key_bits(sub_limit);
  return b == 0 ? 1u : (b + IB_DIGIT_BITS - 1) / IB_DIGIT_BITS;
}

IB_HD inline uint32_t ib_digit(uint32_t key, uint32_t pass) { return (key >> (pass * IB_DIGIT_BITS)) & (IB_RADIX - 1); }

IB_HD inline uint64_t ib_tiles(uint64_t total) { return (total + IB_TILE - 1) / IB_TILE; }

#if defined(__HIPCC__)
// Arguments of the device passes; the first block of pointers is emqx_inbox_batch's.
struct IbArgs {
  const uint64_t* offsets;
  const uint32_t* subs;
  const uint32_t* filters;
  const uint8_t* opts;
  const uint32_t* subids;
  uint64_t n, cap_in, sub_limit;
  uint32_t* box_msgs;
  uint32_t* box_filters;
  uint8_t* box_opts;
  uint32_t* box_subids;
  uint32_t* box_src;
  uint32_t* inbox_subs;
  uint64_t* inbox_offsets;
  uint64_t cap_boxes;
  // scratch of the handle, sized for cap_in deliveries
  uint32_t* key[2];      // [cap_in] ping-pong of the keys; key[(passes - 1) & 1] ends sorted
  uint32_t* idx[2];      // [cap_in] ping-pong of the delivery positions; idx[(passes - 1) & 1] ends as the inbox starts
  uint32_t* msg_of;      // [cap_in] message index of delivery d
  uint32_t* tile_hist;   // [IB_RADIX * tiles] digit-major counts of a pass, then their exclusive scan
  uint32_t* tile_heads;  // [tiles] inbox heads per tile of the sorted keys
  uint32_t* tile_hbase;  // [tiles] exclusive scan of tile_heads
  uint32_t* digit_tot;   // [IB_MAX_PASSES * IB_RADIX] digit totals per pass, zero when the call starts
  unsigned long long* ctr;  // [IB_S_WORDS] counters, zero when the call starts
  void* sort_temp;       // path 1: the library sort's temporary storage
  uint64_t sort_temp_bytes;
  uint64_t* summary;     // device or host-pinned, written last with plain stores
  uint32_t max_blocks;   // grid cap of every pass whose blocks stride
  uint32_t scan_chunk;   // tile totals per carry step of the scans, 1..IB_SCAN_BLOCK
};
int ib_launch(const IbArgs& a, int path, void* stream);
// Temporary storage of path 1's sort over cap_in pairs on the key bits of sub_limit.
uint64_t ib_sort_temp_bytes(uint64_t cap_in, uint64_t sub_limit);
#endif

}  // namespace emqx
