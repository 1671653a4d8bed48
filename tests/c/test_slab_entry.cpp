// Host-side check of the fast-slab entry formats and of the format choice (layout.h):
// pack / unpack at the edges of both fields, the padding marker against every valid entry of
// the narrow format's last ids, and the chooser's boundary.
#include <cstdio>
#include <cstdlib>

#include "layout.h"

using namespace emqx;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

template <class E>
static void round_trip(uint32_t max_id) {
  const uint32_t ids[] = {0u, 1u, 12345u, max_id / 2, max_id - 1, max_id};
  for (uint32_t owner = 0; owner < 64; ++owner)
    for (uint32_t id : ids) {
      const typename E::T e = E::make(owner, id);
      CHECK(E::owner(e) == owner);
      CHECK(E::id(e) == id);
      CHECK(e != E::PAD);
    }
}

int main() {
  static_assert(sizeof(SlabNarrow::T) == 4 && sizeof(SlabWide::T) == 8, "entry widths");
  // the chooser: ids below 2^26 - 1 fit; 2^26 - 1 is the padding marker's id field
  CHECK(SLAB_NARROW_IDS == (1u << 26) - 1u);
  CHECK(slab_narrow_ok(0));
  CHECK(slab_narrow_ok(SLAB_NARROW_IDS - 1));
  CHECK(!slab_narrow_ok(SLAB_NARROW_IDS));
  CHECK(!slab_narrow_ok(1u << 26));
  CHECK(!slab_narrow_ok(0xFFFFFFFEu));
  round_trip<SlabNarrow>(SLAB_NARROW_IDS - 1);
  round_trip<SlabWide>(0xFFFFFFFEu);
  // the one narrow word no entry may be: owner 63 with the first id that does not fit
  CHECK(SlabNarrow::make(63, SLAB_NARROW_IDS) == SlabNarrow::PAD);
  CHECK(SlabNarrow::make(63, SLAB_NARROW_IDS - 1) == SlabNarrow::PAD - 1);
  CHECK(SlabNarrow::make(62, SLAB_NARROW_IDS) != SlabNarrow::PAD);
  // the wide marker carries owner bits (above the 6 an entry uses) that no entry sets
  CHECK((SlabWide::PAD >> 38) != 0 && (SlabWide::make(63, 0xFFFFFFFFu) >> 38) == 0);
  std::puts("ok");
  return 0;
}
