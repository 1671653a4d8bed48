// Stand-alone program over the host-only half of emqx_amd/csrc/stage_host.h (EMQX_STAGE_NO_DEVICE):
// Stage at both alignments the stages use, with sections of 0, 1, align - 1, align and align + 1
// bytes in both orders; offsets_ok on arrays of exactly m + 1 elements; stats_copy into a poisoned
// buffer at every kind of caller size; create and destroy of a host-only handle, every kind of
// device id a build without a device refuses, and its device entry points.  Run plainly and under
// ASan + UBSan (tests/test_stage_host_san.py).
#define EMQX_STAGE_NO_DEVICE
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../emqx_amd/csrc/stage_host.h"

namespace {

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

using namespace emqx;

void check_stage() {
  for (uint64_t align : {16ull, 64ull}) {
    const std::vector<uint64_t> sizes = {0, 1, align - 1, align, align + 1};
    for (int reversed = 0; reversed < 2; ++reversed) {
      std::vector<uint64_t> order(sizes);
      if (reversed) std::reverse(order.begin(), order.end());
      Stage st{align};
      uint64_t end = 0, rounded = 0;  // the end of the section before, the sum of the rounded sizes
      for (uint64_t bytes : order) {
        const uint64_t o = st.place(bytes);
        CHECK(o % align == 0);
        CHECK(o >= end);  // no overlap with the section before
        end = o + bytes;
        rounded += (bytes + align - 1) / align * align;
        CHECK(st.at >= end && st.at == rounded);
      }
      CHECK(st.at == 5 * align);  // 0 + align + align + align + 2 align
    }
  }
}

void check_offsets() {
  // (vectors of exactly m + 1 elements: a read past offsets[m] is a heap overflow under ASan)
  CHECK(offsets_ok(std::vector<uint64_t>{0}.data(), 0));
  CHECK(!offsets_ok(std::vector<uint64_t>{3}.data(), 0));
  CHECK(!offsets_ok(std::vector<uint64_t>{1, 1, 2, 3}.data(), 3));
  const std::vector<uint64_t> good = {0, 0, 2, 2, 5};  // (equal neighbours: empty segments)
  CHECK(offsets_ok(good.data(), 4));
  CHECK(!offsets_ok(good.data() + 2, 2));  // the tail of a good array starts above 0
  // One decrease, at the first pair a decrease can stand at (offsets[0] is 0), a middle pair and the
  // last pair: refused as soon as m reaches it, fine below it.
  const std::vector<uint64_t> first = {0, 7, 3, 9, 9}, middle = {0, 1, 3, 2, 5}, last = {0, 1, 3, 5, 4};
  CHECK(!offsets_ok(first.data(), 4) && !offsets_ok(first.data(), 2) && offsets_ok(first.data(), 1));
  CHECK(!offsets_ok(middle.data(), 4) && !offsets_ok(middle.data(), 3) && offsets_ok(middle.data(), 2));
  CHECK(!offsets_ok(last.data(), 4) && offsets_ok(last.data(), 3));
}

struct Stats {
  uint64_t size;
  uint64_t cap, bytes, calls;
  double last_call_ms;
};
struct Room {
  Stats s;
  unsigned char behind[16];
};

void check_stats_copy() {
  Stats src{};
  src.size = 0x1111111111111111ull;  // (overwritten: `size` is what was copied)
  src.cap = 0x2222222222222222ull;
  src.bytes = 0x3333333333333333ull;
  src.calls = 0x4444444444444444ull;
  src.last_call_ms = 2.5;
  for (uint64_t size : {sizeof(uint64_t), 3 * sizeof(uint64_t), sizeof(Stats), sizeof(Stats) + 16}) {
    Room room;
    std::memset(&room, 0xA5, sizeof(room));
    room.s.size = size;
    stats_copy(&room.s, src);
    const uint64_t n = size < sizeof(Stats) ? size : sizeof(Stats);
    CHECK(room.s.size == n);
    Stats want = src;
    want.size = n;
    unsigned char got[sizeof(Room)], exp[sizeof(Stats)];
    std::memcpy(got, &room, sizeof(room));
    std::memcpy(exp, &want, sizeof(want));
    CHECK(std::memcmp(got, exp, n) == 0);
    for (uint64_t i = n; i < sizeof(Room); ++i) CHECK(got[i] == 0xA5);
  }
}

struct Handle : StageHandle {
  int64_t knob = 7;
  uint64_t cap = 0;
};
struct Policy;  // the stubs of the device forms never ask it anything
struct Args {
  uint64_t m;
};

void check_handle() {
  CHECK(stage_create<Handle>(STAGE_HOST_ONLY, nullptr) == EMQX_EINVAL);
  for (int32_t device : {-1, 0, 1, 7, INT32_MAX}) {  // a device, in a build without one
    Handle* h = reinterpret_cast<Handle*>(uintptr_t{8});
    CHECK(stage_create(device, &h) == EMQX_EDEVICE && h == nullptr);
  }
  for (int32_t device : {-3, -100, INT32_MIN}) {  // neither a device nor STAGE_HOST_ONLY
    Handle* h = reinterpret_cast<Handle*>(uintptr_t{8});
    CHECK(stage_create(device, &h) == EMQX_EINVAL && h == nullptr);
  }
  Handle* h = nullptr;
  CHECK(stage_create(STAGE_HOST_ONLY, &h) == EMQX_OK && h != nullptr);
  CHECK(h->device == STAGE_HOST_ONLY && h->knob == 7 && h->calls == 0 && h->last_call_ms == 0 && h->scratch_bytes == 0);
  const auto t0 = std::chrono::steady_clock::now();
  note_call(h, 1.5);
  note_call(h, -1);  // an asynchronous call keeps the time of the one before
  CHECK(h->calls == 2 && h->last_call_ms == 1.5 && ms_since(t0) >= 0);
  // the device entry points of a build without a device
  const Args a{1};
  uint64_t sum[8];
  Handle* none = nullptr;
  CHECK(reserve(h, uint64_t{1}, uint64_t{2}) == EMQX_EDEVICE && reserve(none, uint64_t{1}, uint64_t{2}, uint64_t{3}) == EMQX_EINVAL);
  CHECK(run_batch(h, &a, sum) == EMQX_EDEVICE && run_batch(none, &a, sum) == EMQX_EINVAL);
  CHECK(run_batch_device<Policy>(h, &a, sum, nullptr) == EMQX_EDEVICE && run_batch_device<Policy>(none, &a, sum, nullptr) == EMQX_EINVAL);
  CHECK(run_batch_device_async<Policy>(h, &a, sum, nullptr) == EMQX_EDEVICE && run_batch_device_async<Policy>(none, &a, sum, nullptr) == EMQX_EINVAL);
  CHECK(stage_destroy(h) == EMQX_OK);
  CHECK(stage_destroy(none) == EMQX_EINVAL);
}

void check_small() {
  CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
  alignas(64) unsigned char buf[128];
  CHECK(al(nullptr, 64) && al(buf, 64) && al(buf + 64, 64) && !al(buf + 32, 64) && al(buf + 32, 16) && !al(buf + 8, 16) && al(buf + 8, 8));
  CHECK(!al(buf + 4, 8) && al(buf + 4, 4) && !al(buf + 2, 4) && al(buf + 2, 2) && !al(buf + 1, 2));
}

}  // namespace

int main() {
  check_stage();
  check_offsets();
  check_stats_copy();
  check_handle();
  check_small();
  std::printf("stage host ok\n");
  return 0;
}
