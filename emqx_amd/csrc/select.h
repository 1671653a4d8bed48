// Snapshot layout and the per-entry predicate of the owner table (include/emqx_select.h,
// DESIGN.md §3.10).  Everything here is __host__ __device__: the kernels (select_kernels.hip)
// and the host evaluator (select.cpp) run the same functions.
#pragma once
#include <stdint.h>

#include "stage_common.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SL_HD __host__ __device__
#else
#define SL_HD
#endif

namespace emqx {

constexpr uint32_t SL_CLASSES = 32;
constexpr uint32_t SL_W_CLASS = 0x1Fu, SL_W_ENABLED = 0x80000000u;  // owner_word: the class bit, the enabled flag
constexpr uint32_t SL_F_OUT_OVERFLOW = 1u, SL_F_INPUT_REFUSED = 2u;
// words of the device counters / the summary
enum { SL_S_FLAGS = 0, SL_S_ENTRIES = 1, SL_S_POSTINGS = 2, SL_S_SELECTED = 3, SL_S_MESSAGES = 4, SL_S_DUPS = 5,
       SL_S_UNKNOWN = 6, SL_S_MAX = 7, SL_S_WORDS = 8,
       SL_C_ENTRY_TOTAL = 8, SL_C_WORDS = 16 };  // past the summary words: the owners the entries add

// The sections of one snapshot blob (each 256-byte aligned in it).
struct SlView {
  const uint32_t* post_offsets;  // [n_filters + 1], dense by filter id; no decrease, the last = n_postings
  const uint32_t* postings;      // [n_postings] owner ids, ascending and unique per filter
  const uint32_t* owner_word;    // [n_owners] SL_W_*; 0: no such owner
  const uint32_t* match_all;     // [n_match_all] ascending match-all owners; they have no postings
  uint32_t n_filters;            // the largest filter id set + 1
  uint32_t n_postings;
  uint32_t n_owners;             // the largest owner id set + 1
  uint32_t n_match_all;
  uint32_t ma_class[SL_CLASSES];  // enabled match-all owners per class
};

// enabled(o) and class(o) in mask; false for an id the table does not hold.
SL_HD inline bool sl_owner_ok(const SlView& v, uint32_t o, uint32_t mask) {
  if (o >= v.n_owners) return false;
  const uint32_t w = v.owner_word[o];
  return (w & SL_W_ENABLED) && ((mask >> (w & SL_W_CLASS)) & 1u);
}

// The posting list of filter f < n_filters as [*lo, *hi), inside [0, n_postings] whatever the
// offsets hold.
SL_HD inline void sl_list(const SlView& v, uint32_t f, uint32_t* lo, uint32_t* hi) {
  uint32_t a = v.post_offsets[f], b = v.post_offsets[f + 1];
  if (b > v.n_postings) b = v.n_postings;
  if (a > b) a = b;
  *lo = a;
  *hi = b;
}

// Whether the ascending postings[lo, hi) hold owner o: at most 32 halvings.
SL_HD inline bool sl_has(const SlView& v, uint32_t lo, uint32_t hi, uint32_t o) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint32_t x = v.postings[mid];
    if (x == o) return true;
    if (x < o) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// The match-all owners that apply under `mask`: their number by the per-class counts of the
// snapshot (what sl_match_all writes, without walking the list).
SL_HD inline uint32_t sl_match_all_count(const SlView& v, uint32_t mask) {
  if (v.n_match_all == 0) return 0;
  uint32_t c = 0;
  for (uint32_t k = 0; k < SL_CLASSES; ++k)
    if ((mask >> k) & 1u) c += v.ma_class[k];
  return c;
}

// Writes them to out[0, room) and returns how many apply (room or not).
SL_HD inline uint32_t sl_match_all(const SlView& v, uint32_t mask, uint32_t* out, uint64_t room) {
  uint32_t k = 0;
  for (uint32_t j = 0; j < v.n_match_all; ++j) {
    const uint32_t o = v.match_all[j];
    if (!sl_owner_ok(v, o, mask)) continue;
    if (out && k < room) out[k] = o;
    ++k;
  }
  return k;
}

struct SlCount {
  uint32_t kept, examined, dups, unknown;
};

// Entry d of a message whose entries start at s <= d: the owners it adds to the message's set.
// A posting (d, o) is kept iff o is enabled, of a class in `mask`, and no entry in [s, d) has o
// in its list; an entry in [s, d) with the same filter id drops all of d.  Kept owners go to
// out[0, room) in ascending order (out may be NULL: count only).  Reads filters[s, d] only.
SL_HD inline SlCount sl_entry(const SlView& v, const uint32_t* filters, uint64_t s, uint64_t d, uint32_t mask,
                              uint32_t* out, uint64_t room) {
  SlCount c{0, 0, 0, 0};
  const uint32_t f = filters[d];
  if (f >= v.n_filters) {
    c.unknown = 1;
    return c;
  }
  uint32_t lo, hi;
  sl_list(v, f, &lo, &hi);
  c.examined = hi - lo;
  if (lo == hi) {  // below the largest id set, but no owner holds it
    c.unknown = 1;
    return c;
  }
  bool same = false;
  for (uint64_t e = s; e < d && !same; ++e) same = filters[e] == f;
  for (uint32_t p = lo; p < hi; ++p) {
    const uint32_t o = v.postings[p];
    if (!sl_owner_ok(v, o, mask)) continue;
    bool dup = same;
    for (uint64_t e = s; e < d && !dup; ++e) {
      const uint32_t g = filters[e];
      if (g >= v.n_filters) continue;
      uint32_t a, b;
      sl_list(v, g, &a, &b);
      dup = sl_has(v, a, b, o);
    }
    if (dup) {
      ++c.dups;
      continue;
    }
    if (out && c.kept < room) out[c.kept] = o;
    ++c.kept;
  }
  return c;
}

// Tuning key "scan_chunk": the elements the one-block scans take per carry step, at most this.
constexpr uint32_t SL_SCAN_BLOCK = 1024;

#if defined(__HIPCC__)
// Arguments of the device passes (select_kernels.hip); the pointers are emqx_select_batch's.
struct SlArgs {
  SlView v;
  const uint64_t* offsets;
  const uint32_t* filters;
  uint64_t n, cap_in;
  const uint32_t* msg_classes;  // NULL: every class
  uint64_t* out_offsets;
  uint32_t* out_owners;
  uint64_t cap_out;
  unsigned long long* ctr;  // [SL_C_WORDS] device counters, zero when the first pass starts
  uint32_t* entry_kept;     // [cap_in] owners each entry adds
  uint64_t* tile_base;      // [ceil(cap_in / SL_TILE)] owners the entries of a tile add, then their exclusive scan
  uint64_t* mtile_base;     // [ceil((n + 1) / SL_TILE)] match-all owners of a tile of messages, then their scan
  uint64_t* ma_before;      // [n] match-all owners of the earlier messages of the same tile
  uint64_t* summary;        // device or host-pinned, written last with plain stores
  uint32_t max_blocks;      // grid cap of the by-entry passes
  uint32_t scan_chunk;      // elements per carry step of the scans, 1..SL_SCAN_BLOCK
};
constexpr uint32_t SL_TILE = 256;  // entries (messages) per tile = threads per block
int sl_launch(const SlArgs& a, void* stream);
#endif

}  // namespace emqx
