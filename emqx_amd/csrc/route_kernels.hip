// Kernels of the batched route stage (include/emqx_route.h).
//
// Work is distributed BY CSR ENTRY over tiles of RT_TILE = 2 048 consecutive entries: RT_ROWS
// rows of RT_BLOCK, so a wave always holds 64 consecutive entries ("chunk" c = row * 4 + wave;
// entry positions ascend with c, then with the lane).  A lane loads its entry's filter id and
// gathers the filter's 16-byte record (rt_record: bounds-checked against the snapshot's slot
// count); flags, route count and forward mask come from route.h, the code the host evaluator
// runs.  No thread or wave iterates over a message's entries or over a filter's dests: a
// forward's rank within its node is a ballot over the wave, per node bit of the snapshot's union
// of forward masks (a kernel argument, so the loop is scalar), plus counts of the chunks and
// tiles before it.  The entry count is read on the device as offsets[n]; the host sizes the grid
// by cap_in only and the blocks stride over the tiles that exist.
//
// The passes, each a kernel boundary on the stream (no inter-block waiting):
//   1  route_count_kernel  per tile: entry_flags; the tile's forwards per node, stored node-major
//                          (tile_hist[node * tiles + tile]); the tile-local exclusive prefix of
//                          routes / kept / has-a-forward at every position (LDS), of which the
//                          tile totals and the value at each message head lying in the tile are
//                          stored (head_routes, head_kf);
//   2  route_scan_kernel   one block: tile_hist becomes its exclusive scan in node-major order (a
//                          node's extent follows the extents of the nodes below it), node_offsets,
//                          the tile bases of the other prefix sums, the totals, the overflow flag;
//   3  route_msgs_kernel   by message: msg_routes[i] and local_offsets[i] as differences of the
//                          global prefix (tile base + head value) at consecutive heads;
//   4  route_scatter_kernel (path 0) per tile (its entries' masks either gathered again or read
//                          back from pass 1's per-entry word, tuning key "stored_mask"): the same
//                          ballots give each forward its position =
//                          the node's scanned tile base + the chunks before it in the tile (LDS)
//                          + the popcount of the ballot below the lane; fwd_msgs (the message by
//                          a bounded search in offsets), fwd_filters; kept entries go to
//                          local_filters at their global exclusive prefix;
//      route_expand_kernel (path 1, the yardstick) per tile: (node, message << 32 | filter)
//                          pairs in entry order behind the tile's scanned forward base;
//                          route_pad_kernel keys the unused capacity behind every node,
//                          rocprim::radix_sort_pairs (stable) on 7 key bits, route_gather_kernel;
//   5  route_finish_kernel the summary with plain stores from one lane (it may be host-pinned).
// Every index is bounded before use: an entry d < offsets[n] <= cap_in, a message index <= n, a
// filter id < n_slots, a forward position < cap_fwd, a kept position < cap_in, a tile <
// rt_tiles(offsets[n]) <= rt_tiles(cap_in).  Nothing depends on the order in which blocks or
// atomics run: the atomics are sums on the counters.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "route.h"

namespace emqx {

namespace {

constexpr uint32_t RT_WAVES = RT_BLOCK / 64;
constexpr uint32_t RT_CHUNKS = RT_ROWS * RT_WAVES;
constexpr uint32_t RT_FLAT_BLOCKS = 1024;  // grid cap of the by-message and by-forward passes
static_assert(RT_CHUNKS <= 64 && RT_NODES == 64, "one lane a chunk, one lane a node");

// offsets[n] when it is an entry count this call may use, else ~0 (the call is refused).
__device__ inline uint64_t rt_total(const RtArgs& a) {
  if (a.n == 0) return 0;
  const uint64_t t = a.offsets[a.n];
  return t <= a.cap_in ? t : ~0ull;
}

// Exclusive prefix, in entry order over the tile, of the per-entry values x[row]; *all: the
// tile's sum.  `chunk` is [RT_CHUNKS] of LDS, free again after the call.  Two barriers.
template <class T>
__device__ inline void tile_scan(const T x[RT_ROWS], T pre[RT_ROWS], T* all, T* chunk) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t r = 0; r < RT_ROWS; ++r) {
    const T incl = wave_incl_scan(x[r]);
    pre[r] = incl - x[r];
    if (lane == 63) chunk[r * RT_WAVES + wave] = incl;
  }
  __syncthreads();
  const T c = lane < RT_CHUNKS ? chunk[lane] : T(0);
  const T ci = wave_incl_scan(c);
  const T ce = ci - c;
#pragma unroll
  for (uint32_t r = 0; r < RT_ROWS; ++r) pre[r] += __shfl(ce, static_cast<int>(r * RT_WAVES + wave), 64);
  *all = __shfl(ci, static_cast<int>(RT_CHUNKS - 1), 64);
  __syncthreads();
}

// The entries of one tile as a thread holds them: row r is entry ts + r * RT_BLOCK + threadIdx.x.
struct Rows {
  uint32_t f[RT_ROWS];
  RtRec rec[RT_ROWS];
  bool valid[RT_ROWS];
};

__device__ inline void rt_load(const RtArgs& a, uint64_t ts, uint64_t total, Rows& t) {
#pragma unroll
  for (uint32_t r = 0; r < RT_ROWS; ++r) {
    const uint64_t d = ts + r * RT_BLOCK + threadIdx.x;
    t.valid[r] = d < total;
    t.f[r] = t.valid[r] ? a.filters[d] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (uint32_t r = 0; r < RT_ROWS; ++r) t.rec[r] = t.valid[r] ? rt_record(a.recs, a.n_slots, t.f[r]) : RtRec{0, 0, 0};
}

__device__ inline uint32_t rt_kept(uint32_t flags) { return (flags & (RT_LOCAL | RT_SHARE)) ? 1u : 0u; }

// What the second pass needs of an entry: its filter id, its forward mask and whether it is kept.
struct Marks {
  uint32_t f[RT_ROWS];
  uint64_t m[RT_ROWS];
  uint32_t keep[RT_ROWS];
};

// Either from the word pass 1 stored per entry (the forward mask, whose bit `local` is free and
// carries the kept indicator) or from the record, gathered again.
__device__ inline void rt_load_marks(const RtArgs& a, uint64_t ts, uint64_t total, Marks& t) {
  if (a.entry_mask) {
#pragma unroll
    for (uint32_t r = 0; r < RT_ROWS; ++r) {
      const uint64_t d = ts + r * RT_BLOCK + threadIdx.x;
      const bool valid = d < total;
      t.f[r] = valid ? a.filters[d] : 0xFFFFFFFFu;
      const uint64_t x = valid ? a.entry_mask[d] : 0ull;
      t.m[r] = x & ~(1ull << a.local);
      t.keep[r] = static_cast<uint32_t>((x >> a.local) & 1ull);
    }
  } else {
    Rows w;
    rt_load(a, ts, total, w);
#pragma unroll
    for (uint32_t r = 0; r < RT_ROWS; ++r) {
      t.f[r] = w.f[r];
      t.m[r] = rt_fwd_mask(w.rec[r], a.local);
      t.keep[r] = rt_kept(rt_flags(w.rec[r], a.local));
    }
  }
}

__global__ __launch_bounds__(RT_BLOCK) void route_count_kernel(RtArgs a) {
  __shared__ uint64_t pre_r[RT_TILE + 1];   // exclusive prefix of routes at every position of the tile, and at its end
  __shared__ uint32_t pre_kf[RT_TILE + 1];  // kept (low 16 bits) and has-a-forward (high): neither exceeds 2 048
  __shared__ uint64_t chunk64[RT_CHUNKS];
  __shared__ uint32_t chunk32[RT_CHUNKS];
  __shared__ uint32_t hist[RT_WAVES][RT_NODES];
  const uint64_t total = rt_total(a);
  if (total == ~0ull) return;
  const uint64_t tiles = rt_tiles(total);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t unknown = 0;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * RT_TILE;
    const bool last = tile + 1 == tiles;
    Rows t;
    rt_load(a, ts, total, t);
    uint64_t xr[RT_ROWS], pr[RT_ROWS], all_r;
    uint32_t xk[RT_ROWS], pk[RT_ROWS], all_k;
    uint32_t mine = 0;  // lane v: this wave's forwards to node v in the tile
#pragma unroll
    for (uint32_t r = 0; r < RT_ROWS; ++r) {
      const uint32_t fl = rt_flags(t.rec[r], a.local);
      const uint64_t m = rt_fwd_mask(t.rec[r], a.local);
      if (t.valid[r]) {
        const uint64_t d = ts + r * RT_BLOCK + threadIdx.x;
        if (a.entry_flags) a.entry_flags[d] = static_cast<uint8_t>(fl);
        if (a.entry_mask) a.entry_mask[d] = m | (static_cast<uint64_t>(rt_kept(fl)) << a.local);
        unknown += fl == 0;
      }
      xr[r] = rt_routes(t.rec[r]);
      xk[r] = rt_kept(fl) | (m ? 1u << 16 : 0u);
      for (uint64_t u = a.fwd_nodes; u; u &= u - 1) {  // scalar: a kernel argument
        const uint32_t v = static_cast<uint32_t>(__builtin_ctzll(u));
        const uint64_t b = __ballot((m >> v) & 1ull);
        if (lane == v) mine += static_cast<uint32_t>(__popcll(b));
      }
    }
    hist[wave][lane] = mine;
    tile_scan<uint64_t>(xr, pr, &all_r, chunk64);  // its barriers publish hist too
    tile_scan<uint32_t>(xk, pk, &all_k, chunk32);
#pragma unroll
    for (uint32_t r = 0; r < RT_ROWS; ++r) {
      pre_r[r * RT_BLOCK + threadIdx.x] = pr[r];
      pre_kf[r * RT_BLOCK + threadIdx.x] = pk[r];
    }
    if (threadIdx.x == 0) {
      pre_r[RT_TILE] = all_r;
      pre_kf[RT_TILE] = all_k;
      a.tile_routes[tile] = all_r;  // scanned in place by pass 2
      a.tile_kept[tile] = all_k & 0xFFFFu;
      a.tile_hasfwd[tile] = all_k >> 16;
    }
    if (wave == 0) {
      uint64_t h = 0;
#pragma unroll
      for (uint32_t w = 0; w < RT_WAVES; ++w) h += hist[w][lane];
      a.tile_hist[static_cast<uint64_t>(lane) * tiles + tile] = h;
      h = wave_sum(h);
      if (lane == 0) a.tile_fwd[tile] = h;
    }
    __syncthreads();
    // the messages whose head lies in [ts, ts + RT_TILE); the last tile also takes the heads at
    // its end (messages without entries behind the last entry, and offsets[n] itself)
    const uint64_t k_lo = csr_lower(a.offsets, 0, a.n + 1, ts);
    const uint64_t k_hi = last ? a.n + 1 : csr_lower(a.offsets, 0, a.n + 1, ts + RT_TILE);
    for (uint64_t k = k_lo + threadIdx.x; k < k_hi; k += RT_BLOCK) {
      const uint64_t off = a.offsets[k];
      const uint64_t p = off < total ? off : total;
      if (p >= ts && p - ts <= (last ? RT_TILE : RT_TILE - 1)) {
        a.head_routes[k] = pre_r[p - ts];
        a.head_kf[k] = pre_kf[p - ts];
      }
    }
    __syncthreads();  // the next tile writes pre_* and hist
  }
  unknown = wave_sum(unknown);
  if (lane == 0 && unknown) atomicAdd(a.ctr + RT_S_UNKNOWN, static_cast<unsigned long long>(unknown));
}

__global__ __launch_bounds__(RT_SCAN_BLOCK) void route_scan_kernel(RtArgs a) {
  __shared__ uint64_t wsum[RT_SCAN_BLOCK / 64];
  const uint64_t total = rt_total(a);
  if (total == ~0ull) return;
  const uint64_t tiles = rt_tiles(total);
  const uint32_t chunk = scan_chunk_of<RT_SCAN_BLOCK>(a.scan_chunk);
  const uint64_t fwd = block_scan_in_place<RT_SCAN_BLOCK>(a.tile_hist, a.tile_hist, RT_NODES * tiles, wsum, chunk);
  (void)block_scan_in_place<RT_SCAN_BLOCK>(a.tile_routes, a.tile_routes, tiles, wsum, chunk);
  const uint64_t kept = block_scan_in_place<RT_SCAN_BLOCK>(a.tile_kept, a.tile_kept, tiles, wsum, chunk);
  (void)block_scan_in_place<RT_SCAN_BLOCK>(a.tile_hasfwd, a.tile_hasfwd, tiles, wsum, chunk);
  (void)block_scan_in_place<RT_SCAN_BLOCK>(a.tile_fwd, a.tile_fwd, tiles, wsum, chunk);
  // (tiles >= 1: the barriers of the later scans stand between the stores of the first and these loads)
  if (threadIdx.x < RT_NODES) a.node_offsets[threadIdx.x] = a.tile_hist[static_cast<uint64_t>(threadIdx.x) * tiles];
  if (threadIdx.x == 0) {
    a.node_offsets[RT_NODES] = fwd;
    a.ctr[RT_S_FWD] = fwd;
    a.ctr[RT_S_KEPT] = kept;
    a.ctr[RT_S_FLAGS] = fwd > a.cap_fwd ? RT_F_FWD_OVERFLOW : 0u;
  }
}

struct Prefix {
  uint64_t routes, kept, hasfwd;
};

// The global prefix at the head of message k (k <= n): the tile's base plus the part inside it.
__device__ inline Prefix rt_head(const RtArgs& a, uint64_t k, uint64_t total, uint64_t tiles) {
  const uint64_t off = a.offsets[k];
  const uint64_t p = off < total ? off : total;
  uint64_t t = p / RT_TILE;
  if (t >= tiles) t = tiles - 1;
  const uint32_t kf = a.head_kf[k];
  return Prefix{a.tile_routes[t] + a.head_routes[k], a.tile_kept[t] + (kf & 0xFFFFu), a.tile_hasfwd[t] + (kf >> 16)};
}

__global__ __launch_bounds__(RT_BLOCK) void route_msgs_kernel(RtArgs a) {
  const uint64_t total = rt_total(a);
  if (total == ~0ull) return;
  const uint64_t tiles = rt_tiles(total);
  uint64_t dropped = 0, fwd_msgs = 0;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * RT_BLOCK + threadIdx.x; j <= a.n;
       j += static_cast<uint64_t>(gridDim.x) * RT_BLOCK) {
    const Prefix p = rt_head(a, j, total, tiles);
    if (a.local_offsets) a.local_offsets[j] = p.kept;
    if (j == a.n) continue;
    const Prefix q = rt_head(a, j + 1, total, tiles);
    a.msg_routes[j] = static_cast<uint32_t>(q.routes - p.routes);
    dropped += q.routes == p.routes;
    fwd_msgs += q.hasfwd > p.hasfwd;
  }
  dropped = wave_sum(dropped);
  fwd_msgs = wave_sum(fwd_msgs);
  if ((threadIdx.x & 63u) == 0) {
    if (dropped) atomicAdd(a.ctr + RT_S_DROPPED, static_cast<unsigned long long>(dropped));
    if (fwd_msgs) atomicAdd(a.ctr + RT_S_FWD_MSGS, static_cast<unsigned long long>(fwd_msgs));
  }
}

// Kept entries of the tile to local_filters at their global exclusive prefix.
__device__ inline void rt_write_kept(const RtArgs& a, uint64_t tile, const Marks& t, uint32_t* chunk32) {
  uint32_t pk[RT_ROWS], all;
  const uint32_t* xk = t.keep;
  tile_scan<uint32_t>(xk, pk, &all, chunk32);
  if (!a.local_filters) return;
  const uint64_t base = a.tile_kept[tile];
#pragma unroll
  for (uint32_t r = 0; r < RT_ROWS; ++r) {
    const uint64_t pos = base + pk[r];
    if (xk[r] && pos < a.cap_in) a.local_filters[pos] = t.f[r];
  }
}

__global__ __launch_bounds__(RT_BLOCK) void route_scatter_kernel(RtArgs a) {
  __shared__ uint32_t cnt[RT_CHUNKS][RT_NODES];  // forwards of chunk c to node v, then their exclusive scan over c
  __shared__ uint64_t base[RT_NODES];            // where node v's forwards of this tile start
  __shared__ uint32_t chunk32[RT_CHUNKS];
  const uint64_t total = rt_total(a);
  if (total == ~0ull) return;
  const uint64_t tiles = rt_tiles(total);
  const bool write = !(a.ctr[RT_S_FLAGS] & RT_F_FWD_OVERFLOW);  // complete: pass 2 has finished
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * RT_TILE;
    Marks t;
    rt_load_marks(a, ts, total, t);
    if (write) {
#pragma unroll
      for (uint32_t r = 0; r < RT_ROWS; ++r) {
        const uint64_t m = t.m[r];
        uint32_t mine = 0;
        for (uint64_t u = a.fwd_nodes; u; u &= u - 1) {
          const uint32_t v = static_cast<uint32_t>(__builtin_ctzll(u));
          const uint64_t b = __ballot((m >> v) & 1ull);
          if (lane == v) mine = static_cast<uint32_t>(__popcll(b));
        }
        cnt[r * RT_WAVES + wave][lane] = mine;
      }
      __syncthreads();
      if (threadIdx.x < RT_NODES) {
        base[threadIdx.x] = a.tile_hist[static_cast<uint64_t>(threadIdx.x) * tiles + tile];
        uint32_t run = 0;
        for (uint32_t c = 0; c < RT_CHUNKS; ++c) {
          const uint32_t x = cnt[c][threadIdx.x];
          cnt[c][threadIdx.x] = run;
          run += x;
        }
      }
      __syncthreads();
#pragma unroll
      for (uint32_t r = 0; r < RT_ROWS; ++r) {
        const uint64_t m = t.m[r];
        const uint32_t c = r * RT_WAVES + wave;
        // n >= 1 here: an entry exists
        const uint32_t msg = m ? static_cast<uint32_t>(csr_find(a.offsets, a.n, ts + r * RT_BLOCK + threadIdx.x)) : 0u;
        for (uint64_t u = a.fwd_nodes; u; u &= u - 1) {
          const uint32_t v = static_cast<uint32_t>(__builtin_ctzll(u));
          const uint64_t b = __ballot((m >> v) & 1ull);
          if ((m >> v) & 1ull) {
            const uint64_t pos = base[v] + cnt[c][v] + static_cast<uint32_t>(__popcll(b & below));
            if (pos < a.cap_fwd) {
              a.fwd_msgs[pos] = msg;
              a.fwd_filters[pos] = t.f[r];
            }
          }
        }
      }
    }
    rt_write_kept(a, tile, t, chunk32);  // its barriers: the next tile may write cnt and base
  }
}

__global__ __launch_bounds__(RT_BLOCK) void route_expand_kernel(RtArgs a) {
  __shared__ uint32_t chunk32[RT_CHUNKS];
  const uint64_t total = rt_total(a);
  if (total == ~0ull) return;
  const uint64_t tiles = rt_tiles(total);
  const bool write = !(a.ctr[RT_S_FLAGS] & RT_F_FWD_OVERFLOW);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t ts = tile * RT_TILE;
    Marks t;
    rt_load_marks(a, ts, total, t);
    uint32_t xf[RT_ROWS], pf[RT_ROWS], all;
#pragma unroll
    for (uint32_t r = 0; r < RT_ROWS; ++r) xf[r] = rt_popc(t.m[r]);
    tile_scan<uint32_t>(xf, pf, &all, chunk32);
    if (write) {
      const uint64_t base = a.tile_fwd[tile];
#pragma unroll
      for (uint32_t r = 0; r < RT_ROWS; ++r) {
        uint64_t m = t.m[r];
        if (!m) continue;
        const uint64_t msg = csr_find(a.offsets, a.n, ts + r * RT_BLOCK + threadIdx.x);
        uint64_t pos = base + pf[r];
        for (; m; m &= m - 1, ++pos)  // the yardstick expands per dest
          if (pos < a.cap_fwd) {
            a.sort_key[0][pos] = static_cast<uint32_t>(__builtin_ctzll(m));
            a.sort_val[0][pos] = (msg << 32) | t.f[r];
          }
      }
    }
    rt_write_kept(a, tile, t, chunk32);
  }
}

// The capacity behind the forwards sorts behind every node.
__global__ __launch_bounds__(RT_BLOCK) void route_pad_kernel(RtArgs a) {
  if (rt_total(a) == ~0ull) return;
  const uint64_t fwd = a.ctr[RT_S_FWD];
  for (uint64_t p = fwd + static_cast<uint64_t>(blockIdx.x) * RT_BLOCK + threadIdx.x; p < a.cap_fwd;
       p += static_cast<uint64_t>(gridDim.x) * RT_BLOCK)
    a.sort_key[0][p] = RT_PAD_KEY;
}

__global__ __launch_bounds__(RT_BLOCK) void route_gather_kernel(RtArgs a) {
  if (rt_total(a) == ~0ull || (a.ctr[RT_S_FLAGS] & RT_F_FWD_OVERFLOW)) return;
  const uint64_t fwd = a.ctr[RT_S_FWD];  // <= cap_fwd
  for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * RT_BLOCK + threadIdx.x; p < fwd && p < a.cap_fwd;
       p += static_cast<uint64_t>(gridDim.x) * RT_BLOCK) {
    const uint64_t x = a.sort_val[1][p];
    a.fwd_msgs[p] = static_cast<uint32_t>(x >> 32);
    a.fwd_filters[p] = static_cast<uint32_t>(x);
  }
}

__global__ void route_finish_kernel(RtArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t total = rt_total(a);
  uint64_t s[RT_S_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  s[RT_S_ENTRIES] = a.n ? a.offsets[a.n] : 0;
  if (total == ~0ull) {
    s[RT_S_FLAGS] = RT_F_INPUT_REFUSED;
  } else {
    for (uint32_t k = RT_S_FLAGS; k < RT_S_FWD_NODES; ++k)
      if (k != RT_S_ENTRIES) s[k] = a.ctr[k];
    for (uint32_t v = 0; v < RT_NODES; ++v) s[RT_S_FWD_NODES] += a.node_offsets[v + 1] > a.node_offsets[v];
  }
  for (uint32_t k = 0; k < RT_S_WORDS; ++k) a.summary[k] = s[k];
}

uint32_t flat_blocks(uint64_t items) {
  const uint64_t rows = (items + RT_BLOCK - 1) / RT_BLOCK;
  return static_cast<uint32_t>(rows < 1 ? 1 : (rows < RT_FLAT_BLOCKS ? rows : RT_FLAT_BLOCKS));
}

}  // namespace

uint64_t rt_sort_temp_bytes(uint64_t cap_fwd) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                  static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                  static_cast<size_t>(cap_fwd), 0u, RT_SORT_BITS);
  return bytes;
}

// Enqueues the passes of one call; a.ctr must be zero when the stream reaches the first of them.
int rt_launch(const RtArgs& a, int path, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t tiles = rt_tiles(a.cap_in);
  const uint32_t cap = a.max_blocks ? a.max_blocks : 1u;
  const uint32_t blocks = static_cast<uint32_t>(tiles < cap ? tiles : cap);
  route_count_kernel<<<dim3(blocks), dim3(RT_BLOCK), 0, s>>>(a);
  route_scan_kernel<<<dim3(1), dim3(RT_SCAN_BLOCK), 0, s>>>(a);
  route_msgs_kernel<<<dim3(flat_blocks(a.n + 1)), dim3(RT_BLOCK), 0, s>>>(a);
  if (path == 0) {
    route_scatter_kernel<<<dim3(blocks), dim3(RT_BLOCK), 0, s>>>(a);
  } else {
    route_expand_kernel<<<dim3(blocks), dim3(RT_BLOCK), 0, s>>>(a);
    if (a.cap_fwd) {
      route_pad_kernel<<<dim3(flat_blocks(a.cap_fwd)), dim3(RT_BLOCK), 0, s>>>(a);
      size_t tb = a.sort_temp_bytes;
      const hipError_t e = rocprim::radix_sort_pairs(a.sort_temp, tb, a.sort_key[0], a.sort_key[1], a.sort_val[0],
                                                     a.sort_val[1], static_cast<size_t>(a.cap_fwd), 0u, RT_SORT_BITS, s);
      if (e != hipSuccess) return static_cast<int>(e);
      route_gather_kernel<<<dim3(flat_blocks(a.cap_fwd)), dim3(RT_BLOCK), 0, s>>>(a);
    }
  }
  route_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
