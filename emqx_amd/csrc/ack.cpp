// C ABI of the ack stage (include/emqx_ack.h): the handle and its device scratch, the device entry
// points of both calls and the host evaluators.  The closed form of the fold lives in ack.h and is
// the same code on both sides.  With EMQX_ACK_NO_DEVICE this file compiles with a plain C++
// compiler into the host-only part (tests/c/test_ack_host.cpp): handles of device
// EMQX_ACK_HOST_ONLY alone.
// The handle's shared fields, create and destroy, the ordering of its calls, the device call forms and
// the staging are stage_host.h's; this file gives them its policy.
#ifdef EMQX_ACK_NO_DEVICE
#define EMQX_STAGE_NO_DEVICE
#endif

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/emqx_ack.h"
#include "ack.h"
#include "stage_host.h"

using namespace emqx;

static_assert(AK_F_INPUT_REFUSED == EMQX_ACK_F_INPUT_REFUSED && AK_F_BAD_SUB == EMQX_ACK_F_BAD_SUB &&
                  AK_F_ROW_FULL == EMQX_ACK_F_ROW_FULL && AK_S_WORDS == EMQX_ACK_SUMMARY_WORDS,
              "flags");
static_assert(AK_EMPTY == EMQX_ACK_EMPTY && AK_MSG == EMQX_ACK_MSG && AK_AWAIT == EMQX_ACK_PUBREL_AWAIT &&
                  AK_PUBACK == EMQX_ACK_PUBACK && AK_PUBREC == EMQX_ACK_PUBREC && AK_PUBCOMP == EMQX_ACK_PUBCOMP,
              "phases and kinds");
static_assert(AK_OK == EMQX_A_OK && AK_IN_USE == EMQX_A_IN_USE && AK_NOT_FOUND == EMQX_A_NOT_FOUND &&
                  AK_NO_SESSION == EMQX_A_NO_SESSION && AK_PASS == EMQX_A_PASS && AK_BAD_KIND == EMQX_A_BAD_KIND,
              "verdicts");
static_assert(AK_NONE == EMQX_ACK_NO_REF && AK_BATCH_N == EMQX_ACK_DEFAULT_BATCH_N && AK_MAX_ACKS + 1 == EMQX_ACK_MAX_ACKS,
              "constants");
static_assert(AK_W_SEND == EMQX_W_SEND && AK_W_MASK == EMQX_W_VERDICT_MASK && AK_O_QOS == EMQX_DELIVER_QOS_MASK &&
                  AK_PRESENT == EMQX_WINDOW_PRESENT && AK_PASSF == EMQX_WINDOW_PASS,
              "what the stage reads of the window stage");
static_assert(sizeof(emqx_ack_slot) == 8 && sizeof(emqx_window_session) == 4 * AK_REC_WORDS &&
                  offsetof(emqx_window_session, inflight) == 4 * AK_REC_INFLIGHT &&
                  offsetof(emqx_window_session, inflight_max) == 4 * AK_REC_INFLIGHT_MAX &&
                  offsetof(emqx_window_session, flags) == 4 * AK_REC_FLAGS,
              "layout");

static_assert(EMQX_ACK_HOST_ONLY == STAGE_HOST_ONLY, "host-only handles");

struct emqx_ack : StageHandle {  // (stage_host.h)
  int64_t rematch = 0;
  int64_t max_blocks = AK_MAX_BLOCKS, scan_chunk = AK_SCAN_BLOCK;
  uint64_t cap_in = 0, cap_boxes = 0, w = 0;  // what the scratch takes
};

namespace {

struct Policy;  // what the call forms of stage_host.h ask of this stage; with the device code below

constexpr uint64_t MAX_SUB_LIMIT = 1ull << 32;

// What both calls share of their argument blocks.
struct Common {
  const uint32_t* subs;
  const uint64_t* offsets;
  const uint64_t* n_boxes;
  uint64_t m, cap_in, cap_boxes, sub_limit, w, max_total;
};
Common common_of(const emqx_ack_record_args* b) {
  return {b->inbox_subs, b->inbox_offsets, b->n_boxes, b->m, b->cap_in, b->cap_boxes, b->sub_limit, b->w, AK_MAX_TOTAL};
}
Common common_of(const emqx_ack_run_args* b) {
  return {b->ack_subs, b->ack_offsets, b->n_boxes, b->m, b->cap_in, b->cap_boxes, b->sub_limit, b->w, AK_MAX_ACKS};
}

// What every form requires of its argument block, whichever memory it points into.
bool common_ok(const Common& c) {
  if (!c.offsets || !ak_w_ok(c.w)) return false;
  if (c.cap_in > AK_MAX_TOTAL || c.cap_boxes > AK_MAX_TOTAL || c.sub_limit > MAX_SUB_LIMIT) return false;
  if (c.cap_boxes && !c.subs) return false;
  if (!c.n_boxes && c.m > c.cap_boxes) return false;
  return true;
}
bool batch_ok(const emqx_ack_record_args* b) {
  if (!b || !common_ok(common_of(b))) return false;
  if (b->cap_in && (!b->box_opts || !b->verdicts || !b->pkt_ids)) return false;
  if (b->cap_boxes && !b->out_unrecorded) return false;
  if (b->sub_limit && !b->slots) return false;
  return true;
}
bool batch_ok(const emqx_ack_run_args* b) {
  if (!b || !common_ok(common_of(b))) return false;
  if (b->cap_in && (!b->acks || !b->verdicts || !b->out_refs)) return false;
  if (b->cap_boxes && !b->out_counts) return false;
  if (b->sub_limit && (!b->slots || !b->sessions)) return false;
  return true;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* summary_out) {
  if (summary_out) std::memcpy(summary_out, sum, AK_S_WORDS * sizeof(uint64_t));
  return (sum[AK_S_FLAGS] & (AK_F_INPUT_REFUSED | AK_F_BAD_SUB)) ? EMQX_EINVAL : EMQX_OK;
}

// Host buffers: the summary of an input the call refuses, or false.
bool refused(const Common& c, uint64_t m, uint64_t* sum) {
  const bool boxes_ok = m <= c.cap_boxes && m <= AK_MAX_TOTAL;
  if (boxes_ok && c.offsets[m] <= c.cap_in && c.offsets[m] <= c.max_total) return false;
  sum[AK_S_FLAGS] = AK_F_INPUT_REFUSED;
  sum[AK_S_BOXES] = m;
  sum[AK_S_TOTAL] = boxes_ok ? c.offsets[m] : 0;
  return true;
}

// ---- the host evaluators -----------------------------------------------------------------------

int record_host(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(c.offsets, m)) return EMQX_EINVAL;
  sum[AK_S_TOTAL] = b->inbox_offsets[m];
  sum[AK_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w);
  for (uint64_t k = 0; k < m; ++k) {
    const uint32_t sub = b->inbox_subs[k];
    const bool ok = sub < b->sub_limit;
    emqx_ack_slot* row = ok ? b->slots + static_cast<uint64_t>(sub) * W : nullptr;
    uint64_t mask = 0;  // the row's EMPTY slots at entry
    for (uint32_t w = 0; ok && w < W; ++w)
      if (row[w].phase == AK_EMPTY) mask |= 1ull << w;
    const uint32_t nfree = static_cast<uint32_t>(__builtin_popcountll(mask));
    uint32_t sends = 0;
    for (uint64_t d = b->inbox_offsets[k]; d < b->inbox_offsets[k + 1]; ++d) {
      if ((b->verdicts[d] & AK_W_MASK) != AK_W_SEND) continue;
      const uint32_t r = sends++;
      if (r >= nfree) continue;
      emqx_ack_slot& s = row[ak_nth_set(mask, r)];
      s.pkt_id = b->pkt_ids[d];
      s.phase = static_cast<uint8_t>(AK_MSG);
      s.qos = b->box_opts[d] & AK_O_QOS;
      s.ref = b->refs ? b->refs[d] : static_cast<uint32_t>(d);
    }
    const uint32_t rec = std::min(sends, nfree);
    b->out_unrecorded[k] = sends - rec;
    sum[AK_R_SENDS] += sends;
    sum[AK_R_RECORDED] += rec;
    sum[AK_R_UNRECORDED] += sends - rec;
    if (ok && sends > rec) {
      sum[AK_R_FULL_ROWS] += 1;
      sum[AK_S_FLAGS] |= AK_F_ROW_FULL;
    }
    if (!ok) sum[AK_S_FLAGS] |= AK_F_BAD_SUB;
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

int run_host(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out) {
  if (!h || !batch_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const Common c = common_of(b);
  const uint64_t m = b->n_boxes ? *b->n_boxes : b->m;
  uint64_t sum[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(c.offsets, m)) return EMQX_EINVAL;
  sum[AK_S_TOTAL] = b->ack_offsets[m];
  sum[AK_S_BOXES] = m;
  const uint32_t W = static_cast<uint32_t>(b->w);
  std::vector<uint8_t> slot_of;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t lo = b->ack_offsets[k], hi = b->ack_offsets[k + 1];
    const uint32_t sub = b->ack_subs[k];
    const bool ok = sub < b->sub_limit;
    uint32_t* counts = b->out_counts + 4 * k;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!ok) sum[AK_S_FLAGS] |= AK_F_BAD_SUB;
    const uint8_t dead = ak_session(ok, ok ? b->sessions[sub].flags : 0u);
    if (dead) {
      for (uint64_t d = lo; d < hi; ++d) {
        b->verdicts[d] = dead;
        b->out_refs[d] = AK_NONE;
      }
      sum[AK_A_REST] += hi - lo;
      continue;
    }
    emqx_ack_slot* row = b->slots + static_cast<uint64_t>(sub) * W;
    uint32_t word0[64], first[64], comp[64];
    for (uint32_t w = 0; w < W; ++w) {
      word0[w] = ak_word0(row[w].pkt_id, row[w].phase, row[w].qos);
      first[w] = comp[w] = AK_NONE;
    }
    slot_of.assign(hi - lo, 0xFF);
    // the three passes of the device form, one after the other
    for (uint64_t d = lo; d < hi; ++d) {
      const uint32_t kind = b->acks[d] >> 16, id = b->acks[d] & 0xFFFFu, p = static_cast<uint32_t>(d - lo);
      if (kind < AK_PUBACK || kind > AK_PUBCOMP) continue;
      for (uint32_t w = 0; w < W; ++w)
        if (ak_hit(word0[w], id)) {
          slot_of[p] = static_cast<uint8_t>(w);
          break;
        }
      const uint32_t w = slot_of[p];
      if (w < W && kind != AK_PUBCOMP) first[w] = std::min(first[w], p * 2u + (kind == AK_PUBREC ? 1u : 0u));
    }
    for (uint64_t d = lo; d < hi; ++d) {
      const uint32_t p = static_cast<uint32_t>(d - lo), w = slot_of[p];
      if (w < W && (b->acks[d] >> 16) == AK_PUBCOMP && ak_comp_counts(ak_phase(word0[w]), first[w], p)) comp[w] = std::min(comp[w], p);
    }
    uint32_t oks = 0;
    for (uint64_t d = lo; d < hi; ++d) {
      const uint32_t kind = b->acks[d] >> 16, p = static_cast<uint32_t>(d - lo), w = slot_of[p];
      uint8_t v = AK_BAD_KIND;
      if (kind >= AK_PUBACK && kind <= AK_PUBCOMP)
        v = w < W ? ak_verdict(kind, ak_phase_at(ak_phase(word0[w]), first[w], comp[w], p)) : AK_NOT_FOUND;
      b->verdicts[d] = v;
      b->out_refs[d] = v == AK_OK ? row[w].ref : AK_NONE;
      oks += v == AK_OK;
      sum[v == AK_OK ? AK_A_OKS : v == AK_IN_USE ? AK_A_IN_USE : v == AK_NOT_FOUND ? AK_A_NOT_FOUND : AK_A_REST] += 1;
    }
    // the rows pass
    uint32_t released = 0, to_pubrel = 0;
    for (uint32_t w = 0; w < W; ++w) {
      const uint32_t s0 = ak_phase(word0[w]), end = ak_phase_at(s0, first[w], comp[w], AK_AT_END);
      if (end == s0) continue;
      if (s0 == AK_MSG && (first[w] & 1u)) ++to_pubrel;
      if (end == AK_EMPTY) {
        ++released;
        std::memset(&row[w], 0, sizeof(row[w]));
      } else {
        row[w].phase = static_cast<uint8_t>(end);
      }
    }
    emqx_window_session& rec = b->sessions[sub];
    const uint32_t after = ak_inflight_after(rec.inflight, released);
    counts[0] = released;
    counts[1] = to_pubrel;
    counts[2] = static_cast<uint32_t>(hi - lo) - oks;
    counts[3] = ak_room(rec.inflight_max, after);
    if (b->update_table) rec.inflight = after;
    sum[AK_A_RELEASED] += released;
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, ms_since(t0));
  }
  return status_of(sum, summary_out);
}

#ifndef EMQX_ACK_NO_DEVICE

// The scratch: of a record call the tile totals, the prefix at every inbox head (and at the end)
// and the masks of the rows; of a run call first[] and comp[]; the counters with the synchronous
// forms' summary behind them.
struct Layout {
  uint64_t tiles, heads, masks, mins, ctr, bytes;
};

Layout layout_of(uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  Layout l{};
  l.tiles = align256(4 * std::max<uint64_t>(ak_tiles(cap_in), 1));
  l.heads = align256(4 * (cap_boxes + 1));
  l.masks = align256(8 * std::max<uint64_t>(cap_boxes, 1));
  l.mins = align256(4 * std::max<uint64_t>(cap_boxes * w, 1));
  l.ctr = align256(2 * AK_S_WORDS * sizeof(uint64_t));
  l.bytes = l.tiles + l.heads + l.masks + 2 * l.mins + l.ctr;
  return l;
}

// Holds h->mu.  Grows the scratch.
int reserve_locked(emqx_ack* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  uint64_t cap = std::max(cap_in, h->cap_in), boxes = std::max(cap_boxes, h->cap_boxes), ww = std::max(w, h->w);
  const int rc = grow_scratch(h, layout_of(cap, boxes, ww).bytes);
  if (rc != EMQX_OK) cap = boxes = ww = 0;  // there is no scratch any more
  h->cap_in = cap;
  h->cap_boxes = boxes;
  h->w = ww;
  return rc;
}

bool fits(emqx_ack* h, const Common& c) {
  return h->d_scratch && c.cap_in <= h->cap_in && c.cap_boxes <= h->cap_boxes && c.w <= h->w;
}

bool common_aligned(const Common& c) { return al(c.offsets, 8) && al(c.n_boxes, 8) && al(c.subs, 4); }
// The device forms move rows and counts 16 bytes at a time.
bool aligned_ok(const emqx_ack_record_args* b) {
  return common_aligned(common_of(b)) && al(b->slots, 16) && al(b->pkt_ids, 2) && al(b->refs, 4) &&
         al(b->out_unrecorded, 4);
}
bool aligned_ok(const emqx_ack_run_args* b) {
  return common_aligned(common_of(b)) && al(b->slots, 16) && al(b->sessions, 16) && al(b->out_counts, 16) &&
         al(b->acks, 4) && al(b->out_refs, 4);
}

int reserve(emqx_ack* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > AK_MAX_TOTAL || cap_boxes > AK_MAX_TOTAL || !ak_w_ok(w)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, cap_boxes, w);
}

// The passes of one call over the handle's scratch; `summary`: where the last of them writes.
int launch(emqx_ack* h, const emqx_ack_record_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  AkRecArgs a{};
  a.inbox_subs = b->inbox_subs;
  a.inbox_offsets = b->inbox_offsets;
  a.box_opts = b->box_opts;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.verdicts = b->verdicts;
  a.pkt_ids = b->pkt_ids;
  a.refs = b->refs;
  a.slots = reinterpret_cast<uint2*>(b->slots);
  a.w = static_cast<uint32_t>(b->w);
  a.sub_limit = b->sub_limit;
  a.out_unrecorded = b->out_unrecorded;
  a.tile_tot = reinterpret_cast<uint32_t*>(p);
  a.head_pre = reinterpret_cast<uint32_t*>(p + l.tiles);
  a.masks = reinterpret_cast<uint64_t*>(p + l.tiles + l.heads);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.bytes - l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  return ak_launch_record(a, s);
}

int launch(emqx_ack* h, const emqx_ack_run_args* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
  AkRunArgs a{};
  a.ack_subs = b->ack_subs;
  a.ack_offsets = b->ack_offsets;
  a.acks = b->acks;
  a.n_boxes = b->n_boxes;
  a.m = b->m;
  a.cap_in = b->cap_in;
  a.cap_boxes = b->cap_boxes;
  a.sessions = reinterpret_cast<uint32_t*>(b->sessions);
  a.sub_limit = b->sub_limit;
  a.update_table = b->update_table;
  a.slots = reinterpret_cast<uint2*>(b->slots);
  a.w = static_cast<uint32_t>(b->w);
  a.verdicts = b->verdicts;
  a.out_refs = b->out_refs;
  a.out_counts = b->out_counts;
  a.rematch = static_cast<uint32_t>(h->rematch);
  a.first = reinterpret_cast<uint32_t*>(p + l.tiles + l.heads + l.masks);
  a.comp = reinterpret_cast<uint32_t*>(p + l.tiles + l.heads + l.masks + l.mins);
  a.ctr = reinterpret_cast<unsigned long long*>(p + l.bytes - l.ctr);
  a.summary = summary;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  return ak_launch_run(a, s);
}

struct Policy {
  static constexpr size_t WORDS = AK_S_WORDS;
  template <class B>
  static bool batch_ok(const B* b) {
    return ::batch_ok(b);
  }
  template <class B>
  static bool aligned_ok(const B* b) {
    return ::aligned_ok(b);
  }
  template <class B>
  static bool fits(emqx_ack* h, const B* b) {
    return ::fits(h, common_of(b));
  }
  template <class B>
  static int reserve(emqx_ack* h, const B* b) {
    const Common c = common_of(b);
    return reserve_locked(h, c.cap_in, c.cap_boxes, c.w);
  }
  static Layout layout(const emqx_ack* h) { return layout_of(h->cap_in, h->cap_boxes, h->w); }
  static uint64_t* own_summary(const emqx_ack* h, const Layout& l) {
    return reinterpret_cast<uint64_t*>(h->d_scratch + l.bytes - l.ctr) + AK_S_WORDS;
  }
  template <class B>
  static int launch(emqx_ack* h, const B* b, uint8_t* p, const Layout& l, uint64_t* summary, hipStream_t s) {
    return ::launch(h, b, p, l, summary, s);
  }
  static int status_of(const uint64_t* sum, uint64_t* summary_out) { return ::status_of(sum, summary_out); }
};

// The rows the call names as a table of their own: list k reads row k; a subscriber the table does
// not hold becomes id m, which that table does not hold either.
void gather_rows(const Common& c, uint64_t m, const emqx_ack_slot* slots, std::vector<uint32_t>* subs, std::vector<emqx_ack_slot>* rows) {
  subs->resize(m);
  rows->assign(std::max<uint64_t>(m * c.w, 2), emqx_ack_slot{0, 0, 0, 0});
  for (uint64_t k = 0; k < m; ++k) {
    const bool ok = c.subs[k] < c.sub_limit;
    (*subs)[k] = static_cast<uint32_t>(ok ? k : m);
    if (ok) std::memcpy(rows->data() + k * c.w, slots + static_cast<uint64_t>(c.subs[k]) * c.w, c.w * sizeof(emqx_ack_slot));
  }
}
void scatter_rows(const Common& c, uint64_t m, emqx_ack_slot* slots, const std::vector<emqx_ack_slot>& rows) {
  for (uint64_t k = 0; k < m; ++k)
    if (c.subs[k] < c.sub_limit)
      std::memcpy(slots + static_cast<uint64_t>(c.subs[k]) * c.w, rows.data() + k * c.w, c.w * sizeof(emqx_ack_slot));
}

int run_batch(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(c.offsets, m)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t total = b->inbox_offsets[m];
  std::vector<uint32_t> subs;
  std::vector<emqx_ack_slot> rows;
  gather_rows(c, m, b->slots, &subs, &rows);
  emqx_ack_record_args d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, total, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(m * 4), o_off = st.place((m + 1) * 8), o_opt = st.place(total), o_ver = st.place(total),
                 o_ids = st.place(total * 2), o_ref = st.place(total * 4), o_row = st.place(rows.size() * 8), o_unr = st.place(m * 4);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.inbox_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.inbox_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.box_opts = D + o_opt;
  d.verdicts = D + o_ver;
  d.pkt_ids = reinterpret_cast<const uint16_t*>(D + o_ids);
  d.refs = b->refs ? reinterpret_cast<const uint32_t*>(D + o_ref) : nullptr;
  d.slots = reinterpret_cast<emqx_ack_slot*>(D + o_row);
  d.out_unrecorded = reinterpret_cast<uint32_t*>(D + o_unr);
  Copier cp = stage_copier(h);
  cp.up(o_sub, subs.data(), m * 4);
  cp.up(o_off, b->inbox_offsets, (m + 1) * 8);
  cp.up(o_opt, b->box_opts, total);
  cp.up(o_ver, b->verdicts, total);
  cp.up(o_ids, b->pkt_ids, total * 2);
  if (b->refs) cp.up(o_ref, b->refs, total * 4);
  cp.up(o_row, rows.data(), m * b->w * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(rows.data(), o_row, m * b->w * 8);
    cp.down(b->out_unrecorded, o_unr, m * 4);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  scatter_rows(c, m, b->slots, rows);
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

int run_batch(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || b->n_boxes) return EMQX_EINVAL;
  const Common c = common_of(b);
  const uint64_t m = b->m;
  uint64_t sum[AK_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(c, m, sum)) return status_of(sum, summary_out);
  if (!offsets_ok(c.offsets, m)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t total = b->ack_offsets[m];
  std::vector<uint32_t> subs;
  std::vector<emqx_ack_slot> rows;
  gather_rows(c, m, b->slots, &subs, &rows);
  std::vector<emqx_window_session> recs(std::max<uint64_t>(m, 1));
  std::memset(recs.data(), 0, recs.size() * sizeof(recs[0]));
  for (uint64_t k = 0; k < m; ++k)
    if (b->ack_subs[k] < b->sub_limit) recs[k] = b->sessions[b->ack_subs[k]];
  emqx_ack_run_args d = *b;
  d.cap_in = total;
  d.cap_boxes = m;
  d.sub_limit = m;
  if (!fits(h, common_of(&d))) {
    const int rc = reserve_locked(h, total, m, b->w);
    if (rc != EMQX_OK) return rc;
  }
  Stage st{16};
  const uint64_t o_sub = st.place(m * 4), o_off = st.place((m + 1) * 8), o_ack = st.place(total * 4), o_tab = st.place(recs.size() * 32),
                 o_row = st.place(rows.size() * 8), o_ver = st.place(total), o_ref = st.place(total * 4), o_cnt = st.place(m * 16);
  const int src = stage_reserve(h, st.at, 16);
  if (src != EMQX_OK) return src;
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.ack_subs = reinterpret_cast<const uint32_t*>(D + o_sub);
  d.ack_offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.acks = reinterpret_cast<const uint32_t*>(D + o_ack);
  d.sessions = reinterpret_cast<emqx_window_session*>(D + o_tab);
  d.slots = reinterpret_cast<emqx_ack_slot*>(D + o_row);
  d.verdicts = D + o_ver;
  d.out_refs = reinterpret_cast<uint32_t*>(D + o_ref);
  d.out_counts = reinterpret_cast<uint32_t*>(D + o_cnt);
  Copier cp = stage_copier(h);
  cp.up(o_sub, subs.data(), m * 4);
  cp.up(o_off, b->ack_offsets, (m + 1) * 8);
  cp.up(o_ack, b->acks, total * 4);
  cp.up(o_tab, recs.data(), m * 32);
  cp.up(o_row, rows.data(), m * b->w * 8);
  int rc = cp.ok ? run_sync_locked<Policy>(h, &d, s, sum) : EMQX_EDEVICE;
  if (rc == EMQX_OK) {
    cp.down(rows.data(), o_row, m * b->w * 8);
    cp.down(recs.data(), o_tab, m * 32);
    cp.down(b->verdicts, o_ver, total);
    cp.down(b->out_refs, o_ref, total * 4);
    cp.down(b->out_counts, o_cnt, m * 16);
    if (!cp.ok) rc = EMQX_EDEVICE;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  scatter_rows(c, m, b->slots, rows);
  if (b->update_table) {
    for (uint64_t k = 0; k < m; ++k)
      if (b->ack_subs[k] < b->sub_limit) b->sessions[b->ack_subs[k]].inflight = recs[k].inflight;
  }
  note_call(h, ms_since(t0));
  return status_of(sum, summary_out);
}

#endif  // EMQX_ACK_NO_DEVICE

int ack_set_tuning(emqx_ack* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t lo = 1, hi;
  if (std::strcmp(key, "rematch") == 0) {
    field = &h->rematch;
    lo = 0;
    hi = 1;
  } else if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = AK_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = AK_SCAN_BLOCK;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < lo || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int ack_stats_get(emqx_ack* h, emqx_ack_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_ack_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.cap_boxes = h->cap_boxes;
  s.w = h->w;
  s.scratch_bytes = h->scratch_bytes;
  s.rematch = static_cast<uint64_t>(h->rematch);
  s.calls = h->calls;
  s.last_call_ms = h->last_call_ms;
  stats_copy(out, s);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_ack_create(int32_t device, emqx_ack** out) {
  return guarded([&] { return stage_create(device, out); });
}
int emqx_ack_destroy(emqx_ack* h) {
  return guarded([&] { return stage_destroy(h); });
}
int emqx_ack_reserve(emqx_ack* h, uint64_t cap_in, uint64_t cap_boxes, uint64_t w) {
  return guarded([&] { return reserve(h, cap_in, cap_boxes, w); });
}
int emqx_ack_record_batch(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_ack_record_batch_device(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_ack_record_batch_device_async(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_ack_record_host(emqx_ack* h, const emqx_ack_record_args* b, uint64_t* summary_out) {
  return guarded([&] { return record_host(h, b, summary_out); });
}
int emqx_ack_run_batch(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_batch(h, b, summary_out); });
}
int emqx_ack_run_batch_device(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out, void* stream) {
  return guarded([&] { return run_batch_device<Policy>(h, b, summary_out, stream); });
}
int emqx_ack_run_batch_device_async(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary, void* stream) {
  return guarded([&] { return run_batch_device_async<Policy>(h, b, summary, stream); });
}
int emqx_ack_run_host(emqx_ack* h, const emqx_ack_run_args* b, uint64_t* summary_out) {
  return guarded([&] { return run_host(h, b, summary_out); });
}
int emqx_ack_set_tuning(emqx_ack* h, const char* key, int64_t value) {
  return guarded([&] { return ack_set_tuning(h, key, value); });
}
int emqx_ack_stats_get(emqx_ack* h, emqx_ack_stats* out) {
  return guarded([&] { return ack_stats_get(h, out); });
}

}  // extern "C"
