// Stand-alone program over the host side of emqx_amd/csrc/stage_common.h: csr_find, csr_lower and
// csr_upper against std::upper_bound and std::lower_bound on offsets of at most 9 elements.  Every
// non-decreasing array of 1..6 offsets over four values, starting at 0 and starting at 5, and a
// list of longer ones: n = 1, runs of equal offsets (empty segments) at the start, in the middle
// and at the end, d below the first offset and at or above the last, every sub-range [lo, hi)
// with lo > 0 and lo == hi included.  The arrays have exactly n elements and, for a sub-range, the
// elements outside it hold values that would mislead a search that read them.  Run plainly and
// under ASan + UBSan (tests/test_stage_common_host_san.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../emqx_amd/csrc/stage_common.h"

namespace {

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

uint64_t g_checks = 0;

void check_array(const std::vector<uint64_t>& off) {
  const uint64_t n = off.size();
  const uint64_t top = off.back() + 2;
  for (uint64_t d = 0; d <= top; ++d) {
    // the last k with off[k] <= d, 0 when d lies below every offset
    const uint64_t ub = static_cast<uint64_t>(std::upper_bound(off.begin(), off.end(), d) - off.begin());
    CHECK(emqx::csr_find(off.data(), n, d) == (ub ? ub - 1 : 0));
    ++g_checks;
    for (uint64_t lo = 0; lo <= n; ++lo)
      for (uint64_t hi = lo; hi <= n; ++hi) {
        std::vector<uint64_t> a(off);  // outside [lo, hi): above every d below it, 0 above it
        for (uint64_t k = 0; k < lo; ++k) a[k] = ~0ull;
        for (uint64_t k = hi; k < n; ++k) a[k] = 0;
        const auto b = off.begin() + static_cast<std::ptrdiff_t>(lo), e = off.begin() + static_cast<std::ptrdiff_t>(hi);
        CHECK(emqx::csr_lower(a.data(), lo, hi, d) == static_cast<uint64_t>(std::lower_bound(b, e, d) - off.begin()));
        CHECK(emqx::csr_upper(a.data(), lo, hi, d) == static_cast<uint64_t>(std::upper_bound(b, e, d) - off.begin()));
        g_checks += 2;
      }
  }
}

// Every non-decreasing array of n offsets over base .. base + 3.
void sweep(std::vector<uint64_t>& off, uint64_t n, uint64_t base) {
  if (off.size() == n) {
    check_array(off);
    return;
  }
  for (uint64_t v = off.empty() ? base : off.back(); v <= base + 3; ++v) {
    off.push_back(v);
    sweep(off, n, base);
    off.pop_back();
  }
}

}  // namespace

int main() {
  for (uint64_t n = 1; n <= 6; ++n)
    for (uint64_t base : {0ull, 5ull}) {
      std::vector<uint64_t> off;
      sweep(off, n, base);
    }
  const std::vector<std::vector<uint64_t>> named = {
      {0},                                  // n = 1
      {7},                                  // n = 1, not starting at 0
      {0, 0, 0, 4, 9, 9, 12, 12, 12},       // empty segments at the start, in the middle and at the end
      {3, 3, 5, 5, 5, 8, 8, 20, 20},        // the same, not starting at 0
      {0, 1, 2, 3, 4, 5, 6, 7, 8},          // no empty segment
      {6, 6, 6, 6, 6, 6, 6, 6, 6},          // nothing but empty segments
  };
  for (const auto& off : named) check_array(off);
  // offsets[0] of no elements is never read
  CHECK(emqx::csr_lower(nullptr, 0, 0, 5) == 0 && emqx::csr_upper(nullptr, 0, 0, 5) == 0 && emqx::csr_find(nullptr, 0, 5) == 0);
  std::printf("stage common host ok (%llu checks)\n", static_cast<unsigned long long>(g_checks));
  return 0;
}
