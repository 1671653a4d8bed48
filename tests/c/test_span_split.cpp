// Host-side check of the head / body / tail split the staged CSR scatter stores a span with
// (layout.h span_split): exhaustive over the span's start within a 16-byte block and lengths
// from nothing to several vectors, then replayed as stores into a guarded buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "layout.h"

using namespace emqx;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

int main() {
  constexpr uint32_t GUARD = 8, MAXLEN = 40;
  constexpr uint32_t MARK = 0xA5A5A5A5u;
  // a 16-byte aligned buffer of entries: guard, the span at every start offset, guard
  std::vector<uint32_t> store(GUARD + 4 + MAXLEN + GUARD + 4);
  uint32_t* buf = store.data();
  while (reinterpret_cast<uintptr_t>(buf) & 15u) ++buf;
  for (uint64_t high : {0ull, 0x7F00000000ull}) {  // the split depends on the low address bits only
    for (uint32_t start = 0; start < 16; start += 4) {
      for (uint32_t len = 0; len <= MAXLEN; ++len) {
        uint32_t* dst = buf + GUARD + start / 4;
        const uint64_t addr = high ? high + start : reinterpret_cast<uint64_t>(dst);
        CHECK((addr & 15u) == start);
        const SpanSplit s = span_split(addr, len);
        CHECK(s.head + 4u * s.vecs + s.tail == len);
        CHECK(s.head < 4 && s.tail < 4);
        CHECK(s.vecs == 0 || ((addr + 4ull * s.head) & 15u) == 0);  // the vector region is aligned
        if (len >= 7) CHECK(s.vecs >= 1);                            // a span of 7 holds a whole aligned vector
        if (s.head < len) CHECK(((addr + 4ull * s.head) & 15u) == 0);  // the head stops at the boundary
        if (high) continue;
        // replay: head entries, 16-byte vectors, tail entries, exactly as the kernel stores them
        for (uint32_t i = 0; i < store.size(); ++i) store[i] = MARK;
        uint32_t p = 0;
        for (uint32_t i = 0; i < s.head; ++i, ++p) dst[p] = p;
        for (uint32_t v = 0; v < s.vecs; ++v, p += 4) {
          CHECK((reinterpret_cast<uintptr_t>(dst + p) & 15u) == 0);
          const uint32_t x[4] = {p, p + 1, p + 2, p + 3};
          std::memcpy(dst + p, x, 16);
        }
        for (uint32_t i = 0; i < s.tail; ++i, ++p) dst[p] = p;
        CHECK(p == len);
        for (uint32_t i = 0; i < len; ++i) CHECK(dst[i] == i);  // every entry once, in place
        for (uint32_t* q = store.data(); q < store.data() + store.size(); ++q)
          if (q < dst || q >= dst + len) CHECK(*q == MARK);     // nothing outside the span
      }
    }
  }
  std::puts("ok");
  return 0;
}
