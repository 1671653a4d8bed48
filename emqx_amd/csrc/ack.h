// Shared pieces of the ack stage (include/emqx_ack.h): the closed form of the
// per-session fold over a list of PUBACK / PUBREC / PUBCOMP.  Within one call a slot's phase only
// moves MSG -> PUBREL_AWAIT -> EMPTY or MSG -> EMPTY and nothing is inserted, so what an ack of
// rank p sees in the slot it names follows from the slot's phase at entry and two minima over the
// acks that name the slot:
//   first = min over its PUBACKs and PUBRECs of p * 2 + (kind == PUBREC)   (t1 and k1 in one word)
//   comp  = min over its PUBCOMPs that can complete (ak_comp_counts) of p  (t2)
// Everything here is __host__ __device__: the kernels (ack_kernels.hip) and the host evaluator
// (ack.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AK_HD __host__ __device__
#else
#define AK_HD
#endif

namespace emqx {

constexpr uint32_t AK_F_INPUT_REFUSED = 2u, AK_F_BAD_SUB = 4u, AK_F_ROW_FULL = 8u;
// words of the summaries
enum {
  AK_S_FLAGS = 0, AK_S_TOTAL = 1, AK_S_BOXES = 2,
  AK_R_SENDS = 3, AK_R_RECORDED = 4, AK_R_UNRECORDED = 5, AK_R_FULL_ROWS = 6,                // record
  AK_A_OKS = 3, AK_A_RELEASED = 4, AK_A_IN_USE = 5, AK_A_NOT_FOUND = 6, AK_A_REST = 7,        // run
  AK_S_WORDS = 8
};

constexpr uint32_t AK_BLOCK = 256;                    // threads per block
constexpr uint32_t AK_ROWS = 4;                       // consecutive acks or deliveries per thread
constexpr uint32_t AK_TILE = AK_BLOCK * AK_ROWS;      // per tile (1024)
constexpr uint64_t AK_MAX_TOTAL = (1ull << 32) - 1;   // positions and inbox indices are 32-bit
constexpr uint64_t AK_MAX_ACKS = (1ull << 31) - 1;    // a rank and one bit share 32 bits
// Tuning (emqx_ack_set_tuning): the largest grid of the by-tile and by-row passes, beyond which
// the blocks stride, and the tile totals record's one-block scan takes per carry step.
constexpr uint32_t AK_MAX_BLOCKS = 4096;
constexpr uint32_t AK_SCAN_BLOCK = 1024;
constexpr uint32_t AK_NONE = 0xFFFFFFFFu;

// phase of a slot (EMQX_ACK_*), kind of an ack, the verdict byte (EMQX_A_*)
constexpr uint32_t AK_EMPTY = 0, AK_MSG = 1, AK_AWAIT = 2;
constexpr uint32_t AK_PUBACK = 1, AK_PUBREC = 2, AK_PUBCOMP = 3;
constexpr uint8_t AK_OK = 1, AK_IN_USE = 2, AK_NOT_FOUND = 3, AK_NO_SESSION = 4, AK_PASS = 5, AK_BAD_KIND = 6;
constexpr uint32_t AK_BATCH_N = 1000;
// what the stage reads of the window stage: its SEND verdict, the QoS bits, the record's flags
constexpr uint8_t AK_W_SEND = 2, AK_W_MASK = 0x0F, AK_O_QOS = 0x03;
constexpr uint32_t AK_PRESENT = 1u, AK_PASSF = 8u;
// a 32-byte session record as eight words
constexpr uint32_t AK_REC_WORDS = 8, AK_REC_INFLIGHT = 0, AK_REC_INFLIGHT_MAX = 1, AK_REC_FLAGS = 5;

// A slot as two words: pkt_id | phase << 16 | qos << 24, and ref.
AK_HD inline uint32_t ak_word0(uint32_t pkt_id, uint32_t phase, uint32_t qos) {
  return (pkt_id & 0xFFFFu) | ((phase & 0xFFu) << 16) | ((qos & 0xFFu) << 24);
}
AK_HD inline uint32_t ak_phase(uint32_t word0) { return (word0 >> 16) & 0xFFu; }
AK_HD inline bool ak_hit(uint32_t word0, uint32_t pkt_id) { return ak_phase(word0) != AK_EMPTY && (word0 & 0xFFFFu) == pkt_id; }
AK_HD inline uint32_t ak_with_phase(uint32_t word0, uint32_t phase) { return (word0 & ~0x00FF0000u) | (phase << 16); }

AK_HD inline bool ak_w_ok(uint64_t w) { return w == 8 || w == 16 || w == 32 || w == 64; }

// 0: the session takes acks; else the verdict of every one of its acks.
AK_HD inline uint8_t ak_session(bool sub_ok, uint32_t flags) {
  if (!sub_ok || !(flags & AK_PRESENT)) return AK_NO_SESSION;
  return (flags & AK_PASSF) ? AK_PASS : 0;
}

// What an ack of rank p sees in its slot.  A phase that is none of the three never changes.
AK_HD inline uint32_t ak_phase_at(uint32_t s0, uint32_t first, uint32_t comp, uint32_t p) {
  if (s0 == AK_MSG) {
    if (first == AK_NONE || p <= (first >> 1)) return AK_MSG;
    if (!(first & 1u)) return AK_EMPTY;  // a PUBACK took it
  } else if (s0 != AK_AWAIT) {
    return s0;
  }
  return (comp == AK_NONE || p <= comp) ? AK_AWAIT : AK_EMPTY;
}
constexpr uint32_t AK_AT_END = AK_NONE;  // the rank behind every ack: the phase after the call

// Whether a PUBCOMP of rank p on the slot can be the one that completes it: the slot awaits the
// PUBREL from the start, or from the PUBREC of rank t1 < p on.
AK_HD inline bool ak_comp_counts(uint32_t s0, uint32_t first, uint32_t p) {
  if (s0 == AK_AWAIT) return true;
  return s0 == AK_MSG && first != AK_NONE && (first & 1u) && p > (first >> 1);
}

// The table of include/emqx_ack.h; `seen`: the phase of the ack's slot at its moment.
AK_HD inline uint8_t ak_verdict(uint32_t kind, uint32_t seen) {
  if (seen == AK_EMPTY) return AK_NOT_FOUND;
  return (kind == AK_PUBCOMP ? seen == AK_AWAIT : seen == AK_MSG) ? AK_OK : AK_IN_USE;
}

// batch_n/1 on the window after `released` slots were freed.
AK_HD inline uint32_t ak_inflight_after(uint32_t inflight, uint32_t released) {
  return inflight > released ? inflight - released : 0u;
}
AK_HD inline uint32_t ak_room(uint32_t inflight_max, uint32_t inflight_after) {
  if (inflight_max == 0) return AK_BATCH_N;
  return inflight_max > inflight_after ? inflight_max - inflight_after : 0u;
}

// The index of the r-th set bit of mask (r from 0, r < popcount(mask)).
AK_HD inline uint32_t ak_nth_set(uint64_t mask, uint32_t r) {
  uint32_t pos = 0;
  for (uint32_t width = 32; width; width >>= 1) {
    const uint64_t low = (mask >> pos) & ((1ull << width) - 1ull);
    const uint32_t c = static_cast<uint32_t>(__builtin_popcountll(low));
    if (r >= c) {
      r -= c;
      pos += width;
    }
  }
  return pos;
}

AK_HD inline uint64_t ak_tiles(uint64_t total) { return (total + AK_TILE - 1) / AK_TILE; }

#if defined(__HIPCC__)
// Arguments of the device passes of a record call; the first block is emqx_ack_record_args'.
struct AkRecArgs {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  const uint8_t* verdicts;
  const uint16_t* pkt_ids;
  const uint32_t* refs;
  uint2* slots;
  uint32_t w;
  uint64_t sub_limit;
  uint32_t* out_unrecorded;
  // scratch of the handle
  uint32_t* tile_tot;       // [tiles] SEND verdicts of a tile, then their exclusive scan
  uint32_t* head_pre;       // [cap_boxes + 1] SEND verdicts between the tile's start and the inbox's head
  uint64_t* masks;          // [cap_boxes] the EMPTY slots of the inbox's row at entry
  unsigned long long* ctr;  // [AK_S_WORDS] counters, zeroed by the scan kernel
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks;      // grid cap of every pass whose blocks stride
  uint32_t scan_chunk;      // tile totals per carry step of the scan, 1..AK_SCAN_BLOCK
};
// Of a run call.
struct AkRunArgs {
  const uint32_t* ack_subs;
  const uint64_t* ack_offsets;
  const uint32_t* acks;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  uint32_t* sessions;  // AK_REC_WORDS words a record
  uint64_t sub_limit;
  uint64_t update_table;
  uint2* slots;
  uint32_t w;
  uint8_t* verdicts;
  uint32_t* out_refs;
  uint32_t* out_counts;
  uint32_t rematch;
  // scratch of the handle
  uint32_t* first;          // [cap_boxes * w]
  uint32_t* comp;           // [cap_boxes * w]
  unsigned long long* ctr;  // [AK_S_WORDS] counters, zeroed by the init kernel
  uint64_t* summary;
  uint32_t max_blocks;  // grid cap of every pass whose blocks stride
};
int ak_launch_record(const AkRecArgs& a, void* stream);
int ak_launch_run(const AkRunArgs& a, void* stream);
#endif

}  // namespace emqx
