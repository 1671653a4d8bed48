// Shared pieces of the window stage (include/emqx_window.h): the closed form of
// the session fold.  An inbox's plan follows from its record at entry and its two live counts;
// a delivery's verdict from the plan and its two ranks.  Everything here is __host__ __device__:
// the kernels (window_kernels.hip) and the host evaluator (window.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WN_HD __host__ __device__
#else
#define WN_HD
#endif

namespace emqx {

constexpr uint32_t WN_F_INPUT_REFUSED = 2u, WN_F_BAD_SUB = 4u;
// words of the summary
enum {
  WN_S_FLAGS = 0, WN_S_TOTAL = 1, WN_S_BOXES = 2, WN_S_SENDS = 3, WN_S_SENDS0 = 4, WN_S_QUEUED = 5, WN_S_DROPS = 6,
  WN_S_WRAPPED = 7, WN_S_WORDS = 8
};

constexpr uint32_t WN_BLOCK = 256;                   // threads per block
constexpr uint32_t WN_ROWS = 8;                      // consecutive deliveries per thread
constexpr uint32_t WN_TILE = WN_BLOCK * WN_ROWS;     // deliveries per tile (2048)
constexpr uint64_t WN_MAX_TOTAL = (1ull << 32) - 1;  // positions, ranks and inbox indices are 32-bit
// Tuning (emqx_window_set_tuning): the largest grid of the by-tile and by-row passes, beyond which
// the blocks stride, and the tile totals the one-block scan takes per carry step.
constexpr uint32_t WN_MAX_BLOCKS = 2048;
constexpr uint32_t WN_WAVE_BLOCKS = 16384;  // path 1's wave kernel while max_blocks is at its maximum
constexpr uint32_t WN_SCAN_BLOCK = 1024;

// the verdict byte (EMQX_W_*)
constexpr uint8_t WN_SEND_QOS0 = 1, WN_SEND = 2, WN_QUEUED = 3, WN_QUEUED_DROPPED = 4, WN_DROP_QOS0 = 5,
                  WN_SKIP_NO_LOCAL = 6, WN_BAD_MESSAGE = 7, WN_NO_SESSION = 8, WN_PASS = 9, WN_EVICTS = 0x80;
// the opts byte (EMQX_DELIVER_*)
constexpr uint8_t WN_O_QOS = 0x03, WN_O_NO_LOCAL = 0x10, WN_O_BAD = 0x40;
// flags of a record (EMQX_WINDOW_*)
constexpr uint32_t WN_PRESENT = 1u, WN_CONNECTED = 2u, WN_STORE_QOS0 = 4u, WN_PASSF = 8u;
constexpr uint32_t WN_PKT_MOD = 65535;

// emqx_window_session
struct alignas(8) WnRec {
  uint32_t inflight, inflight_max, mq_len, mq_max, next_pkt_id, flags;
  uint64_t dropped;
};
static_assert(sizeof(WnRec) == 32, "two 16-byte halves");

// What an opts byte says on its own: 0 not live, 1 live with q = 0, 2 live with q > 0.
WN_HD inline uint32_t wn_live(uint8_t o) {
  if (o & (WN_O_NO_LOCAL | WN_O_BAD)) return 0;
  return (o & WN_O_QOS) ? 2u : 1u;
}

enum : uint32_t { WN_M_NONE = 0, WN_M_PASS = 1, WN_M_CONN = 2, WN_M_DISC = 3, WN_M_DISC_STORE = 4 };

// What a delivery needs of its inbox.
struct WnPlan {
  uint32_t mode;   // WN_M_*
  uint32_t sends;  // the first `sends` live q > 0 deliveries get an id (connected)
  uint32_t pkt0;   // (next_pkt_id - 1) mod 65535
  uint32_t qd;     // the first qd candidates are QUEUED_DROPPED
  uint32_t ev;     // candidates of rank >= ev evict (~0: none does)
};

// What the inbox's own outputs add.
struct WnTotals {
  uint32_t sends, sends0, queued, evicted_old;
  uint64_t drops;
  uint32_t wrapped;
};

WN_HD inline uint32_t wn_sat32(uint64_t x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(x); }

// The plan of an inbox with A live q > 0 and Z live q = 0 deliveries; `ok`: its subscriber id is
// below sub_limit and *rec is its record.  *rec becomes the record after the batch.
WN_HD inline WnPlan wn_plan(bool ok, WnRec* rec, uint32_t A, uint32_t Z, WnTotals* t) {
  WnPlan p{WN_M_NONE, 0, 0, 0, ~0u};
  *t = WnTotals{0, 0, 0, 0, 0, 0};
  if (!ok || !(rec->flags & WN_PRESENT)) return p;
  if (rec->flags & WN_PASSF) {
    p.mode = WN_M_PASS;
    return p;
  }
  uint64_t e;  // queue candidates
  if (rec->flags & WN_CONNECTED) {
    p.mode = WN_M_CONN;
    uint32_t room = A;  // inflight_max 0: never full
    if (rec->inflight_max) room = rec->inflight_max > rec->inflight ? rec->inflight_max - rec->inflight : 0u;
    p.sends = A < room ? A : room;
    e = A - p.sends;
    t->sends0 = Z;
  } else if (rec->flags & WN_STORE_QOS0) {
    p.mode = WN_M_DISC_STORE;
    e = static_cast<uint64_t>(A) + Z;
  } else {
    p.mode = WN_M_DISC;
    e = A;
    t->drops = Z;
  }
  p.pkt0 = (rec->next_pkt_id - 1u) % WN_PKT_MOD;
  t->sends = p.sends;
  t->wrapped = p.sends > WN_PKT_MOD ? 1u : 0u;
  const uint64_t L = rec->mq_len, M = rec->mq_max;
  if (M == 0 || L > M) {
    rec->mq_len = wn_sat32(L + e);
    t->queued = wn_sat32(e);
  } else {
    const uint64_t v = L + e > M ? L + e - M : 0;
    p.qd = static_cast<uint32_t>(e > M ? e - M : 0);
    p.ev = static_cast<uint32_t>(M - L);
    rec->mq_len = static_cast<uint32_t>(L + e < M ? L + e : M);
    rec->dropped += v;
    t->evicted_old = static_cast<uint32_t>(L < v ? L : v);
    t->queued = static_cast<uint32_t>(e - p.qd);
    t->drops += v;
  }
  rec->inflight = wn_sat32(static_cast<uint64_t>(rec->inflight) + p.sends);
  if (p.sends) rec->next_pkt_id = static_cast<uint32_t>((p.pkt0 + static_cast<uint64_t>(p.sends)) % WN_PKT_MOD) + 1u;
  return p;
}

// The verdict of a delivery with opts byte o; a and z: the live q > 0 and live q = 0 deliveries
// before it in its inbox.
WN_HD inline uint8_t wn_verdict(const WnPlan& p, uint8_t o, uint32_t a, uint32_t z, uint16_t* id) {
  *id = 0;
  if (o & WN_O_NO_LOCAL) return WN_SKIP_NO_LOCAL;
  if (o & WN_O_BAD) return WN_BAD_MESSAGE;
  if (p.mode == WN_M_NONE) return WN_NO_SESSION;
  if (p.mode == WN_M_PASS) return WN_PASS;
  const bool q0 = (o & WN_O_QOS) == 0;
  uint32_t c;
  if (p.mode == WN_M_CONN) {
    if (q0) return WN_SEND_QOS0;
    if (a < p.sends) {
      *id = static_cast<uint16_t>((p.pkt0 + a % WN_PKT_MOD) % WN_PKT_MOD + 1u);
      return WN_SEND;
    }
    c = a - p.sends;
  } else if (p.mode == WN_M_DISC_STORE) {
    c = a + z;
  } else {
    if (q0) return WN_DROP_QOS0;
    c = a;
  }
  return static_cast<uint8_t>((c < p.qd ? WN_QUEUED_DROPPED : WN_QUEUED) | (c >= p.ev ? WN_EVICTS : 0));
}

WN_HD inline uint64_t wn_tiles(uint64_t total) { return (total + WN_TILE - 1) / WN_TILE; }

#if defined(__HIPCC__)
// Arguments of the device passes; the first block is emqx_window_batch's.
struct WnArgs {
  const uint32_t* inbox_subs;
  const uint64_t* inbox_offsets;
  const uint8_t* box_opts;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes;
  WnRec* sessions;
  uint64_t sub_limit;
  uint64_t update_table;
  uint8_t* verdicts;
  uint16_t* pkt_ids;
  WnRec* out_sessions;
  uint32_t* out_counts;
  // scratch of the handle, sized for cap_in deliveries and cap_boxes inboxes
  uint64_t* tile_tot;   // [tiles] live counts of a tile (q > 0 low, q = 0 high), then their exclusive scan
  uint64_t* head_pre;   // [cap_boxes + 1] live counts between the tile's start and the inbox's head
  unsigned long long* ctr;  // [WN_S_WORDS] counters, zeroed by the scan kernel
  uint64_t* summary;    // device or host-pinned, written last with plain stores
  uint32_t max_blocks;  // grid cap of every pass whose blocks stride
  uint32_t scan_chunk;  // tile totals per carry step of the scan, 1..WN_SCAN_BLOCK
};
int wn_launch(const WnArgs& a, int path, void* stream);
#endif

}  // namespace emqx
