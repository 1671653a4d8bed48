// The host side that the six session stages share (window, ack, retry, mqueue, rel, pmqueue;
// DESIGN.md §3.9): the handle with its stream, event, scratch and staging, create and destroy, the
// ordering of a handle's calls, the three device call forms and the staging of the host-buffer one.
// What differs between the stages reaches the call forms as a policy type P (see below).  A stage
// file defines EMQX_STAGE_NO_DEVICE from its own EMQX_<STAGE>_NO_DEVICE in front of the include: then
// this header includes no HIP header, compiles with a plain C++ compiler, and the device entry
// points are stubs that answer EMQX_EDEVICE.
#pragma once
#ifndef EMQX_STAGE_NO_DEVICE
#include <hip/hip_runtime.h>
#endif

#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "../../include/emqx_match.h"
#ifndef EMQX_STAGE_NO_DEVICE
#include "streams.h"
#endif

namespace emqx {

constexpr int32_t STAGE_HOST_ONLY = -2;  // every stage's EMQX_<STAGE>_HOST_ONLY

// What every stage's handle holds; struct emqx_<stage> derives from it and adds its tuning keys and
// the capacities its scratch was sized for.
struct StageHandle {
  int device = STAGE_HOST_ONLY;
  std::mutex mu;  // the calls of a handle, its scratch and its stats
  uint64_t calls = 0;
  double last_call_ms = 0;
  uint64_t scratch_bytes = 0;
#ifndef EMQX_STAGE_NO_DEVICE
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // behind the last call enqueued
  bool inflight = false;
  uint8_t* d_scratch = nullptr;
  uint8_t* d_stage = nullptr;  // staging of the host-buffer entry points
  uint64_t stage_cap = 0;
#endif
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Holds h->mu.  ms < 0: an asynchronous call, whose time nobody has seen.
inline void note_call(StageHandle* h, double ms) {
  ++h->calls;
  if (ms >= 0) h->last_call_ms = ms;
}

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// p is a multiple of `bytes` (a power of two); NULL is.
inline bool al(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// Host buffers only: offsets[0] = 0, no decrease over offsets[0 .. m].
inline bool offsets_ok(const uint64_t* offsets, uint64_t m) {
  if (offsets[0] != 0) return false;
  for (uint64_t k = 0; k < m; ++k)
    if (offsets[k + 1] < offsets[k]) return false;
  return true;
}

// The end of every *_stats_get: as many bytes of `s` as the caller's struct takes (out->size, which
// the caller has checked to hold `size` itself), and how many that were.
template <class S>
void stats_copy(S* out, S s) {
  const uint64_t nbytes = std::min<uint64_t>(out->size, sizeof(s));
  s.size = nbytes;
  std::memcpy(out, &s, nbytes);
}

// Sections of a staging buffer, each a multiple of `align` bytes (16: the widest access of the
// device forms; 64 where a section holds the priority queue's 64-byte heads).
struct Stage {
  uint64_t align;
  uint64_t at = 0;
  uint64_t place(uint64_t bytes) {
    const uint64_t o = at;
    at += (bytes + align - 1) & ~(align - 1);
    return o;
  }
};

template <class H>
int stage_create(int32_t device, H** out) {
  if (!out) return EMQX_EINVAL;
  *out = nullptr;
  if (device < -1 && device != STAGE_HOST_ONLY) return EMQX_EINVAL;
#ifdef EMQX_STAGE_NO_DEVICE
  if (device >= -1) return EMQX_EDEVICE;
#else
  if (device == -1 && hipGetDevice(&device) != hipSuccess) return EMQX_EDEVICE;  // the current device
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return EMQX_EDEVICE;
  }
#endif
  std::unique_ptr<H> h(new (std::nothrow) H());
  if (!h) return EMQX_ENOMEM;
  h->device = device;
#ifndef EMQX_STAGE_NO_DEVICE
  if (device >= 0) {
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->done, hipEventDisableTiming) != hipSuccess) {
      if (h->stream) (void)hipStreamDestroy(h->stream);
      return EMQX_EDEVICE;
    }
  }
#endif
  *out = h.release();
  return EMQX_OK;
}

template <class H>
int stage_destroy(H* h) {
  if (!h) return EMQX_EINVAL;
#ifndef EMQX_STAGE_NO_DEVICE
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

#ifdef EMQX_STAGE_NO_DEVICE

// The device entry points of a build without a device: reserve(h, capacities ...), the
// host-buffer call and the two device forms.
template <class H, class... Caps>
int reserve(H* h, Caps...) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
template <class H, class B>
int run_batch(H* h, const B*, uint64_t*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
template <class P, class H, class B>
int run_batch_device(H* h, const B*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}
template <class P, class H, class B>
int run_batch_device_async(H* h, const B*, uint64_t*, void*) {
  return h ? EMQX_EDEVICE : EMQX_EINVAL;
}

#else

#define STAGE_TRY(expr)                        \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return EMQX_EDEVICE; \
  } while (0)

// Holds h->mu.  Behind the last call enqueued.
inline void drain(StageHandle* h) {
  if (h->inflight) (void)hipEventSynchronize(h->done);
  h->inflight = false;
}

// Holds h->mu.  The scratch becomes `bytes` long; on EMQX_ENOMEM there is none.  A scratch of that
// very size is kept, without a wait for the call in flight, although the capacities behind `bytes`
// may have grown: a stage's capacities only grow (its reserve_locked takes the max), every section
// of its layout_of is non-decreasing in each of them, so an equal total means an equal layout, and
// the call in flight and the next one agree on where everything lies.
inline int grow_scratch(StageHandle* h, uint64_t bytes) {
  if (h->d_scratch && bytes == h->scratch_bytes) return EMQX_OK;
  drain(h);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  h->d_scratch = nullptr;
  h->scratch_bytes = 0;
  if (hipMalloc(reinterpret_cast<void**>(&h->d_scratch), bytes) != hipSuccess) return EMQX_ENOMEM;
  h->scratch_bytes = bytes;
  return EMQX_OK;
}

// Holds h->mu.  The staging takes `bytes` (a Stage's `at`), at least one section.
inline int stage_reserve(StageHandle* h, uint64_t bytes, uint64_t align) {
  const uint64_t need = std::max<uint64_t>(bytes, align);
  if (h->stage_cap >= need) return EMQX_OK;
  drain(h);
  if (h->d_stage) (void)hipFree(h->d_stage);
  h->d_stage = nullptr;
  h->stage_cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(&h->d_stage), need + need / 2) != hipSuccess) return EMQX_ENOMEM;
  h->stage_cap = need + need / 2;
  return EMQX_OK;
}

// Copies between host buffers and the sections of a staging buffer on one stream; after the first
// failure it does nothing.
struct Copier {
  uint8_t* D;
  hipStream_t s;
  bool ok = true;
  void up(uint64_t o, const void* src, uint64_t bytes) {
    if (ok && bytes) ok = hipMemcpyAsync(D + o, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  }
  void down(void* dst, uint64_t o, uint64_t bytes) {
    if (ok && bytes) ok = hipMemcpyAsync(dst, D + o, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  }
};

// Holds h->mu.  The copier of a host-buffer call over the handle's staging, on the handle's stream
// and behind the call in flight: that one may read the staging.
inline Copier stage_copier(StageHandle* h) {
  Copier cp{h->d_stage, h->stream};
  if (h->inflight && hipStreamWaitEvent(h->stream, h->done, 0) != hipSuccess) cp.ok = false;
  return cp;
}

// Holds h->mu.  Orders a call behind the handle's previous one: `launch()` enqueues its passes on
// `s` and returns 0 when all of them were.
template <class Launch>
int enqueue_ordered(StageHandle* h, hipStream_t s, Launch launch) {
  if (h->inflight) STAGE_TRY(hipStreamWaitEvent(s, h->done, 0));
  const int rc = launch() == 0 ? EMQX_OK : EMQX_EDEVICE;
  if (hipEventRecord(h->done, s) != hipSuccess) {
    (void)hipStreamSynchronize(s);
    h->inflight = false;
    return EMQX_EDEVICE;
  }
  h->inflight = true;
  return rc;
}

// ---- the call forms ------------------------------------------------------------------------------
// P, a stage's policy, says what they do not share (H: the stage's handle, B: either of its
// argument blocks, L: its scratch layout):
//   P::WORDS                              the words of a summary
//   P::batch_ok(b), P::aligned_ok(b)      what every form, and what the device forms require of b
//   P::fits(h, b), P::reserve(h, b)       whether the scratch takes b's capacities; growing it to
//   P::layout(h)                          the layout of the scratch as reserved
//   P::own_summary(h, l)                  the handle's own summary words in the scratch
//   P::launch(h, b, p, l, summary, s)     the passes over the scratch at p; 0 when all were enqueued
//   P::status_of(sum, summary_out)        what a synchronous form returns for a finished summary

// Holds h->mu.  Enqueues the passes behind the handle's previous call; `summary` NULL: the handle's
// own summary words, which *d_sum_out names in either case.
template <class P, class H, class B>
int enqueue(H* h, const B* b, uint64_t* summary, hipStream_t s, uint64_t** d_sum_out) {
  const auto l = P::layout(h);
  uint64_t* d_sum = P::own_summary(h, l);
  if (d_sum_out) *d_sum_out = d_sum;
  return enqueue_ordered(h, s, [&] { return P::launch(h, b, h->d_scratch, l, summary ? summary : d_sum, s); });
}

template <class P, class H, class B>
int run_batch_device_async(H* h, const B* b, uint64_t* summary, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!summary || !P::batch_ok(b) || !P::aligned_ok(b)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  if (!P::fits(h, b)) return EMQX_EOVERFLOW;  // nothing is enqueued
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) STAGE_TRY(after_null_stream(s));
  const int rc = enqueue<P>(h, b, summary, s, nullptr);
  note_call(h, -1);
  return rc;
}

// Holds h->mu.  The call on `s` and the copy of its summary to `sum` behind it; the caller
// synchronizes.
template <class P, class H, class B>
int run_sync_locked(H* h, const B* b, hipStream_t s, uint64_t* sum) {
  uint64_t* d_sum = nullptr;
  int rc = enqueue<P>(h, b, nullptr, s, &d_sum);
  if (rc == EMQX_OK && hipMemcpyAsync(sum, d_sum, P::WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = EMQX_EDEVICE;
  return rc;
}

template <class P, class H, class B>
int run_batch_device(H* h, const B* b, uint64_t* summary_out, void* stream) {
  if (!h) return EMQX_EINVAL;
  if (h->device < 0) return EMQX_EDEVICE;
  if (!P::batch_ok(b) || !P::aligned_ok(b)) return EMQX_EINVAL;
  STAGE_TRY(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(h->mu);
  if (!P::fits(h, b)) {
    const int rc = P::reserve(h, b);
    if (rc != EMQX_OK) return rc;
  }
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  if (!stream) STAGE_TRY(after_null_stream(s));
  uint64_t sum[P::WORDS] = {};
  int rc = run_sync_locked<P>(h, b, s, sum);
  if (hipStreamSynchronize(s) != hipSuccess) rc = EMQX_EDEVICE;
  h->inflight = false;
  if (rc != EMQX_OK) return rc;
  note_call(h, ms_since(t0));
  return P::status_of(sum, summary_out);
}

#endif  // EMQX_STAGE_NO_DEVICE

}  // namespace emqx
