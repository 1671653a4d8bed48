// C ABI of the inbox stage (include/emqx_inbox.h): the handle and its device scratch, the three
// device entry points and the host evaluator.  The digit and pass arithmetic lives in inbox.h and
// is the same code on both sides.  With EMQX_INBOX_NO_DEVICE this file compiles with a plain C++
// compiler into the host-only part (tests/c/test_inbox_host.cpp): handles of device
// EMQX_INBOX_HOST_ONLY alone.
#ifndef EMQX_INBOX_NO_DEVICE
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/emqx_inbox.h"
#include "inbox.h"
#ifndef EMQX_INBOX_NO_DEVICE
#include "streams.h"
#endif

using namespace emqx;

static_assert(IB_F_BOX_OVERFLOW == EMQX_INBOX_F_BOX_OVERFLOW && IB_F_INPUT_REFUSED == EMQX_INBOX_F_INPUT_REFUSED &&
                  IB_F_BAD_SUB == EMQX_INBOX_F_BAD_SUB,
              "flags");
static_assert(IB_S_WORDS == EMQX_INBOX_SUMMARY_WORDS && IB_MAX_SUB_LIMIT == EMQX_INBOX_MAX_SUB_LIMIT, "layout");

struct emqx_inbox {
  int device = EMQX_INBOX_HOST_ONLY;
  std::mutex mu;  // the calls of a handle, its scratch and its stats
  int64_t path = 0;
  int64_t max_blocks = IB_MAX_BLOCKS, scan_chunk = IB_SCAN_BLOCK;
  uint64_t calls = 0, last_passes = 0;
  double last_call_ms = 0;
  uint64_t cap_in = 0, sub_limit = 0, scratch_bytes = 0;  // what the scratch takes
#ifndef EMQX_INBOX_NO_DEVICE
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // behind the last call enqueued
  bool inflight = false;
  uint8_t* d_scratch = nullptr;
  uint64_t temp_bytes = 0;  // of it, the library sort's temporary storage
  uint8_t* d_stage = nullptr;  // staging of the host entry point
  uint64_t stage_cap = 0;
#endif
};

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What every group form requires of its argument block, whichever memory it points into.
bool batch_ok(const emqx_inbox_batch* b) {
  if (!b || !b->offsets || !b->inbox_offsets) return false;
  if (b->sub_limit < 1 || b->sub_limit > IB_MAX_SUB_LIMIT || b->cap_in > IB_MAX_TOTAL) return false;
  if (b->cap_in && (!b->subs || !b->filters || !b->box_msgs || !b->box_filters)) return false;
  if ((b->box_opts && !b->opts) || (b->box_subids && !b->subids)) return false;
  if (b->cap_boxes && !b->inbox_subs) return false;
  return true;
}

// Host buffers only: offsets[0] = 0, no decrease.
bool offsets_ok(const emqx_inbox_batch* b) {
  if (b->offsets[0] != 0) return false;
  for (uint64_t i = 0; i < b->n; ++i)
    if (b->offsets[i + 1] < b->offsets[i]) return false;
  return true;
}

bool refused(const emqx_inbox_batch* b) {
  return b->n > IB_MAX_TOTAL || b->offsets[b->n] > b->cap_in || b->offsets[b->n] > IB_MAX_TOTAL;
}

// What the synchronous forms return for a finished call's summary.
int status_of(const uint64_t* sum, uint64_t* n_boxes, uint64_t* summary_out) {
  if (n_boxes) *n_boxes = sum[IB_S_BOXES];
  if (summary_out) std::memcpy(summary_out, sum, IB_S_WORDS * sizeof(uint64_t));
  if (sum[IB_S_FLAGS] & (IB_F_INPUT_REFUSED | IB_F_BAD_SUB)) return EMQX_EINVAL;
  return (sum[IB_S_FLAGS] & IB_F_BOX_OVERFLOW) ? EMQX_EOVERFLOW : EMQX_OK;
}

void note_call(emqx_inbox* h, const emqx_inbox_batch* b, double ms) {
  ++h->calls;
  h->last_passes = ib_passes(b->sub_limit);
  if (ms >= 0) h->last_call_ms = ms;
}

int inbox_create(int32_t device, emqx_inbox** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != EMQX_INBOX_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_INBOX_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<emqx_inbox> h(new (std::nothrow) emqx_inbox());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
#ifndef EMQX_INBOX_NO_DEVICE
  if (device >= 0) {
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->done, hipEventDisableTiming) != hipSuccess) {
      if (h->stream) (void)hipStreamDestroy(h->stream);
      return EMQX_EDEVICE;
    }
  }
#endif
  *out = h.release();
  return EMQX_OK;
}

int inbox_destroy(emqx_inbox* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_INBOX_NO_DEVICE
  if (h->device >= 0) {
    (void)hipSetDevice(h->device);
    if (h->inflight) (void)hipEventSynchronize(h->done);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
  }
#endif
  delete h;
  return EMQX_OK;
}

// The stable sort of the positions by subscriber, with the passes and digits of the kernels: a
// counting sort a digit.  perm ends in `idx`.
void sort_host(const uint32_t* subs, uint64_t total, uint32_t passes, std::vector<uint32_t>& key,
               std::vector<uint32_t>& idx) {
  key.assign(subs, subs + total);
  idx.resize(total);
  for (uint64_t d = 0; d < total; ++d) idx[d] = static_cast<uint32_t>(d);
  std::vector<uint32_t> key2(total), idx2(total);
  for (uint32_t p = 0; p < passes; ++p) {
    uint64_t at[IB_RADIX + 1] = {0};
    for (uint64_t d = 0; d < total; ++d) ++at[ib_digit(key[d], p) + 1];
    for (uint32_t k = 0; k < IB_RADIX; ++k) at[k + 1] += at[k];
    for (uint64_t d = 0; d < total; ++d) {
      const uint64_t pos = at[ib_digit(key[d], p)]++;
      key2[pos] = key[d];
      idx2[pos] = idx[d];
    }
    key.swap(key2);
    idx.swap(idx2);
  }
}

int group_host(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out) {
  if (!h || !batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t sum[IB_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (refused(b)) {
    sum[IB_S_FLAGS] = IB_F_INPUT_REFUSED;
    sum[IB_S_TOTAL] = b->n <= IB_MAX_TOTAL ? b->offsets[b->n] : 0;
    return status_of(sum, n_boxes, summary_out);
  }
  const uint64_t n = b->n, total = b->offsets[n];
  sum[IB_S_TOTAL] = total;
  for (uint64_t i = 0; i < n; ++i)
    if (b->offsets[i + 1] > b->offsets[i]) ++sum[IB_S_MSGS];
  for (uint64_t d = 0; d < total; ++d)
    if (b->subs[d] >= b->sub_limit) {
      sum[IB_S_FLAGS] = IB_F_BAD_SUB;
      return status_of(sum, n_boxes, summary_out);
    }
  std::vector<uint32_t> key, idx;
  sort_host(b->subs, total, ib_passes(b->sub_limit), key, idx);
  // the message of every position, in input order: one walk over the offsets
  std::vector<uint32_t> msg_of(total);
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t d = b->offsets[i]; d < b->offsets[i + 1]; ++d) msg_of[d] = static_cast<uint32_t>(i);
  uint64_t m = 0, longest = 0, start = 0;
  for (uint64_t k = 0; k < total; ++k) {
    const uint32_t src = idx[k];
    b->box_msgs[k] = msg_of[src];
    b->box_filters[k] = b->filters[src];
    if (b->box_opts) b->box_opts[k] = b->opts[src];
    if (b->box_subids) b->box_subids[k] = b->subids[src];
    if (b->box_src) b->box_src[k] = src;
    if (k == 0 || key[k] != key[k - 1]) {
      if (k) longest = std::max(longest, k - start);
      start = k;
      if (m < b->cap_boxes) b->inbox_subs[m] = key[k];
      if (m <= b->cap_boxes) b->inbox_offsets[m] = k;
      ++m;
    }
  }
  if (total) longest = std::max(longest, total - start);
  if (m <= b->cap_boxes) b->inbox_offsets[m] = total;
  else sum[IB_S_FLAGS] |= IB_F_BOX_OVERFLOW;
  sum[IB_S_BOXES] = m;
  sum[IB_S_LONGEST] = longest;
  {
    std::lock_guard<std::mutex> g(h->mu);
    note_call(h, b, ms_since(t0));
  }
  return status_of(sum, n_boxes, summary_out);
}

#ifdef EMQX_INBOX_NO_DEVICE

int inbox_reserve(emqx_inbox* h, uint64_t, uint64_t) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int group_batch(emqx_inbox* h, const emqx_inbox_batch*, uint64_t*, uint64_t*) { return h ? EMQX_EDEVICE : EMQX_EINVAL; }
int group_batch_device(emqx_inbox* h, const emqx_inbox_batch*, uint64_t*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
int group_batch_device_async(emqx_inbox* h, const emqx_inbox_batch*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

#define IB_TRY(expr)                           \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// The scratch of a call of cap deliveries: five arrays of cap words, the digit-major tile table,
// the two tile arrays of the boundary step, the zeroed block (digit totals, counters) with the
// synchronous forms' summary behind it, then the library sort's temporary storage.
struct Layout {
  uint64_t words, hist, tiles, zero, temp, bytes;
};
constexpr uint64_t ZERO_BYTES = IB_MAX_PASSES * IB_RADIX * sizeof(uint32_t) + IB_S_WORDS * sizeof(uint64_t);

Layout layout_of(uint64_t cap, uint64_t temp_bytes) {
  Layout l{};
  const uint64_t tiles = std::max<uint64_t>(ib_tiles(cap), 1);
  l.words = align256(4 * std::max<uint64_t>(cap, 1));
  l.hist = align256(4 * IB_RADIX * tiles);
  l.tiles = align256(4 * tiles);
  l.zero = align256(ZERO_BYTES + IB_S_WORDS * sizeof(uint64_t));
  l.temp = align256(temp_bytes);
  l.bytes = 5 * l.words + l.hist + 2 * l.tiles + l.zero + l.temp;
  return l;
}

// Waits for the call in flight (the scratch it uses is about to be freed or reused by a call on
// another stream's behalf from the host).
void drain(emqx_inbox* h) {
  if (h->inflight) (void)hipEventSynchronize(h->done);
  h->inflight = false;
}

// Holds h->mu.  Grows the scratch to take cap_in deliveries and ids below sub_limit.
int reserve_locked(emqx_inbox* h, uint64_t cap_in, uint64_t sub_limit) {
  const uint64_t cap = std::max(cap_in, h->cap_in), lim = std::max(sub_limit, h->sub_limit);
  // the library sort sizes its storage by the count and the key bits: take the largest of the
  // shapes asked for
  const uint64_t temp = std::max({ib_sort_temp_bytes(cap, lim), ib_sort_temp_bytes(cap, IB_MAX_SUB_LIMIT),
                                  ib_sort_temp_bytes(cap_in, sub_limit), h->temp_bytes});
  if (h->d_scratch && cap == h->cap_in && temp <= h->temp_bytes) {
    h->sub_limit = lim;
    return EMQX_OK;
  }
  drain(h);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  h->d_scratch = nullptr;
  h->cap_in = h->sub_limit = h->scratch_bytes = h->temp_bytes = 0;
  const Layout l = layout_of(cap, temp);
  if (hipMalloc(reinterpret_cast<void**>(&h->d_scratch), l.bytes) != hipSuccess) return EMQX_ENOMEM;
  h->cap_in = cap;
  h->sub_limit = lim;
  h->scratch_bytes = l.bytes;
  h->temp_bytes = l.temp;
  return EMQX_OK;
}

// Holds h->mu.  True when the scratch takes this call as it is.
bool fits(emqx_inbox* h, const emqx_inbox_batch* b) {
  if (!h->d_scratch || b->cap_in > h->cap_in || b->sub_limit > h->sub_limit) return false;
  return h->path == 0 || ib_sort_temp_bytes(b->cap_in, b->sub_limit) <= h->temp_bytes;
}

int inbox_reserve(emqx_inbox* h, uint64_t cap_in, uint64_t sub_limit) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (cap_in > IB_MAX_TOTAL || sub_limit < 1 || sub_limit > IB_MAX_SUB_LIMIT) return EMQX_EINVAL;
  IB_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  return reserve_locked(h, cap_in, sub_limit);
}

// Holds h->mu.  Orders the call behind the handle's previous one, zeroes the counters on the
// stream and enqueues the passes; `summary` NULL: the handle's own summary words.
int enqueue(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* summary, hipStream_t s, uint64_t** d_sum_out) {
  const Layout l = layout_of(h->cap_in, h->temp_bytes);
  uint8_t* p = h->d_scratch;
  IbArgs a{};
  a.offsets = b->offsets;
  a.subs = b->subs;
  a.filters = b->filters;
  a.opts = b->opts;
  a.subids = b->subids;
  a.n = b->n;
  a.cap_in = b->cap_in;
  a.sub_limit = b->sub_limit;
  a.box_msgs = b->box_msgs;
  a.box_filters = b->box_filters;
  a.box_opts = b->box_opts;
  a.box_subids = b->box_subids;
  a.box_src = b->box_src;
  a.inbox_subs = b->inbox_subs;
  a.inbox_offsets = b->inbox_offsets;
  a.cap_boxes = b->cap_boxes;
  auto take = [&p](uint64_t bytes) {
    uint8_t* at = p;
    p += bytes;
    return at;
  };
  a.key[0] = reinterpret_cast<uint32_t*>(take(l.words));
  a.key[1] = reinterpret_cast<uint32_t*>(take(l.words));
  a.idx[0] = reinterpret_cast<uint32_t*>(take(l.words));
  a.idx[1] = reinterpret_cast<uint32_t*>(take(l.words));
  a.msg_of = reinterpret_cast<uint32_t*>(take(l.words));
  a.tile_hist = reinterpret_cast<uint32_t*>(take(l.hist));
  a.tile_heads = reinterpret_cast<uint32_t*>(take(l.tiles));
  a.tile_hbase = reinterpret_cast<uint32_t*>(take(l.tiles));
  uint8_t* zero = take(l.zero);
  a.digit_tot = reinterpret_cast<uint32_t*>(zero);
  a.ctr = reinterpret_cast<unsigned long long*>(zero + IB_MAX_PASSES * IB_RADIX * sizeof(uint32_t));
  uint64_t* d_sum = reinterpret_cast<uint64_t*>(zero + ZERO_BYTES);
  a.sort_temp = take(l.temp);
  a.sort_temp_bytes = h->temp_bytes;
  a.summary = summary ? summary : d_sum;
  a.max_blocks = static_cast<uint32_t>(h->max_blocks);
  a.scan_chunk = static_cast<uint32_t>(h->scan_chunk);
  if (d_sum_out) *d_sum_out = d_sum;
  if (h->inflight) IB_TRY(hipStreamWaitEvent(s, h->done, 0));
  IB_TRY(hipMemsetAsync(zero, 0, ZERO_BYTES, s));
  const int rc = ib_launch(a, static_cast<int>(h->path), s) == 0 ? EMQX_OK : EMQX_EDEVICE;
  if (hipEventRecord(h->done, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    h->inflight = false;
    return EMQX_EDEVICE;
  }
  h->inflight = true;
  return rc;
}

int group_batch_device_async(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !batch_ok(b)) return EMQX_EINVAL;
  IB_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  if (!fits(h, b)) return EMQX_EOVERFLOW;  // nothing is enqueued
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) IB_TRY(after_null_stream(s));
  const int rc = enqueue(h, b, summary, s, nullptr);
  note_call(h, b, -1);
  return rc;
}

int group_batch_device(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b)) return EMQX_EINVAL;
  IB_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  if (!fits(h, b)) {
    const int rc = reserve_locked(h, b->cap_in, b->sub_limit);
    if (rc != EMQX_OK) return rc;
  }
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) IB_TRY(after_null_stream(s));
  uint64_t* d_sum = nullptr;
  uint64_t sum[IB_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = enqueue(h, b, nullptr, s, &d_sum);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  note_call(h, b, ms_since(t0));
  return status_of(sum, n_boxes, summary_out);
}

int group_batch(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!batch_ok(b) || !offsets_ok(b)) return EMQX_EINVAL;
  if (refused(b)) {
    uint64_t sum[IB_S_WORDS] = {IB_F_INPUT_REFUSED, b->n <= IB_MAX_TOTAL ? b->offsets[b->n] : 0, 0, 0, 0, 0, 0, 0};
    return status_of(sum, n_boxes, summary_out);
  }
  IB_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t n = b->n, total = b->offsets[n];
  const uint64_t cap_boxes = std::min(b->cap_boxes, total);  // no more than `total` inboxes can exist
  emqx_inbox_batch d = *b;
  d.cap_in = total;
  d.cap_boxes = cap_boxes;
  if (!fits(h, &d)) {
    const int rc = reserve_locked(h, total, b->sub_limit);
    if (rc != EMQX_OK) return rc;
  }
  // staging, every section 16-byte aligned
  uint64_t at = 0;
  auto place = [&at](uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + 15) & ~15ull;
    return o;
  };
  const uint64_t o_off = place((n + 1) * 8), o_subs = place(total * 4), o_fil = place(total * 4),
                 o_opts = place(b->opts ? total : 0), o_sid = place(b->subids ? total * 4 : 0), o_bmsg = place(total * 4),
                 o_bfil = place(total * 4), o_bopt = place(b->box_opts ? total : 0),
                 o_bsid = place(b->box_subids ? total * 4 : 0), o_bsrc = place(b->box_src ? total * 4 : 0),
                 o_isub = place(cap_boxes * 4), o_ioff = place((cap_boxes + 1) * 8);
  const uint64_t need = std::max<uint64_t>(at, 16);
  if (h->stage_cap < need) {
    drain(h);
    if (h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&h->d_stage), need + need / 2) != hipSuccess) return EMQX_ENOMEM;
    h->stage_cap = need + need / 2;
  }
  hipStream_t s = h->stream;
  uint8_t* D = h->d_stage;
  d.offsets = reinterpret_cast<const uint64_t*>(D + o_off);
  d.subs = reinterpret_cast<const uint32_t*>(D + o_subs);
  d.filters = reinterpret_cast<const uint32_t*>(D + o_fil);
  d.opts = b->opts ? D + o_opts : nullptr;
  d.subids = b->subids ? reinterpret_cast<const uint32_t*>(D + o_sid) : nullptr;
  d.box_msgs = reinterpret_cast<uint32_t*>(D + o_bmsg);
  d.box_filters = reinterpret_cast<uint32_t*>(D + o_bfil);
  d.box_opts = b->box_opts ? D + o_bopt : nullptr;
  d.box_subids = b->box_subids ? reinterpret_cast<uint32_t*>(D + o_bsid) : nullptr;
  d.box_src = b->box_src ? reinterpret_cast<uint32_t*>(D + o_bsrc) : nullptr;
  d.inbox_subs = reinterpret_cast<uint32_t*>(D + o_isub);
  d.inbox_offsets = reinterpret_cast<uint64_t*>(D + o_ioff);
  auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
    return bytes == 0 || hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  };
  auto down = [&](void* dst, uint64_t o, uint64_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  };
  int rc = EMQX_OK;
  if (h->inflight && hipStreamWaitEvent(s, h->done, 0) != hipSuccess) rc = EMQX_EDEVICE;  // it may read the staging
  bool ok = rc == EMQX_OK && up(o_off, b->offsets, (n + 1) * 8) && up(o_subs, b->subs, total * 4) &&
            up(o_fil, b->filters, total * 4) && up(o_opts, b->opts, b->opts ? total : 0) &&
            up(o_sid, b->subids, b->subids ? total * 4 : 0);
  if (!ok) rc = EMQX_EDEVICE;
  uint64_t* d_sum = nullptr;
  uint64_t sum[IB_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rc == EMQX_OK) rc = enqueue(h, &d, nullptr, s, &d_sum);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, s) != hipSuccess) rc = EMQX_EDEVICE;
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc == EMQX_OK && !(sum[IB_S_FLAGS] & (IB_F_INPUT_REFUSED | IB_F_BAD_SUB))) {
    const uint64_t boxes = std::min(sum[IB_S_BOXES], cap_boxes);
    ok = down(b->box_msgs, o_bmsg, total * 4) && down(b->box_filters, o_bfil, total * 4) &&
         down(b->box_opts, o_bopt, b->box_opts ? total : 0) && down(b->box_subids, o_bsid, b->box_subids ? total * 4 : 0) &&
         down(b->box_src, o_bsrc, b->box_src ? total * 4 : 0) && down(b->inbox_subs, o_isub, boxes * 4) &&
         down(b->inbox_offsets, o_ioff, (boxes + 1) * 8);
    if (!ok) rc = EMQX_EDEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  }
  if (rc != EMQX_OK) return rc;
  note_call(h, b, ms_since(t0));
  return status_of(sum, n_boxes, summary_out);
}

#endif  // EMQX_INBOX_NO_DEVICE

int inbox_set_tuning(emqx_inbox* h, const char* key, int64_t value) {
  if (!h || !key) return EMQX_EINVAL;
  int64_t* field;
  int64_t lo = 1, hi;
  if (std::strcmp(key, "path") == 0) {
    field = &h->path;
    lo = 0;
    hi = 1;
  } else if (std::strcmp(key, "max_blocks") == 0) {  // read at enqueue; a host-only handle has no grid
    field = &h->max_blocks;
    hi = IB_MAX_BLOCKS;
  } else if (std::strcmp(key, "scan_chunk") == 0) {
    field = &h->scan_chunk;
    hi = IB_SCAN_BLOCK;
  } else {
    return EMQX_ENOTFOUND;
  }
  if (value < lo || value > hi) return EMQX_EINVAL;
  std::lock_guard<std::mutex> g(h->mu);
  *field = value;
  return EMQX_OK;
}

int inbox_stats_get(emqx_inbox* h, emqx_inbox_stats* out) {
  if (!h || !out || out->size < sizeof(uint64_t)) return EMQX_EINVAL;
  emqx_inbox_stats s{};
  std::lock_guard<std::mutex> g(h->mu);
  s.cap_in = h->cap_in;
  s.sub_limit = h->sub_limit;
  s.scratch_bytes = h->scratch_bytes;
  s.path = static_cast<uint64_t>(h->path);
  s.calls = h->calls;
  s.last_passes = h->last_passes;
  s.last_call_ms = h->last_call_ms;
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
  return EMQX_OK;
}

}  // namespace

extern "C" {

int emqx_inbox_create(int32_t device, emqx_inbox** out) {
  return guarded([&] { return inbox_create(device, out); });
}
int emqx_inbox_destroy(emqx_inbox* h) {
  return guarded([&] { return inbox_destroy(h); });
}
int emqx_inbox_reserve(emqx_inbox* h, uint64_t cap_in, uint64_t sub_limit) {
  return guarded([&] { return inbox_reserve(h, cap_in, sub_limit); });
}
int emqx_inbox_group_batch(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out) {
  return guarded([&] { return group_batch(h, b, n_boxes, summary_out); });
}
int emqx_inbox_group_batch_device(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out,
                                  void* stream) {
  return guarded([&] { return group_batch_device(h, b, n_boxes, summary_out, stream); });
}
int emqx_inbox_group_batch_device_async(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* summary, void* stream) {
  return guarded([&] { return group_batch_device_async(h, b, summary, stream); });
}
int emqx_inbox_group_host(emqx_inbox* h, const emqx_inbox_batch* b, uint64_t* n_boxes, uint64_t* summary_out) {
  return guarded([&] { return group_host(h, b, n_boxes, summary_out); });
}
int emqx_inbox_set_tuning(emqx_inbox* h, const char* key, int64_t value) {
  return guarded([&] { return inbox_set_tuning(h, key, value); });
}
int emqx_inbox_stats_get(emqx_inbox* h, emqx_inbox_stats* out) {
  return guarded([&] { return inbox_stats_get(h, out); });
}

}  // extern "C"
