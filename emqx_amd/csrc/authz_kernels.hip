// Kernels of the batched authorization check (include/emqx_authz.h).
//
// A request's work is the concatenation of its client's entry ranges (segments, resolved at
// commit); its answer is the LOWEST entry whose rule also passes action and who.  G lanes share
// one request (G = 1, 4, 16 or 64, chosen on the host per call: pick_group, authz.cpp):
// each step the group's lanes evaluate G consecutive entries with the predicate of authz.h (the
// same functions emqx_authz_check_host runs), a ballot restricted to the group's lanes finds the
// first hit, and the group stops at the first step that has one, so a later rule never overrides
// an earlier one.  G = 1 is a lane per request (three-entry tables: every lane works), G = 64 a
// wave per request (thousands of entries: 64 at a time).
// No inter-wave communication, no waiting, no atomics on results: every request writes its own
// two outputs, every loop is bounded by a count read from the snapshot (segments per client <=
// AZ_SEG_STRIDE, entries per segment) or by a level of the topic or filter.
#include <hip/hip_runtime.h>

#include "authz.h"

namespace emqx {

namespace {

constexpr uint32_t AZ_BLOCK = 256;

template <uint32_t G>
__global__ __launch_bounds__(AZ_BLOCK) void authz_check_kernel(AzView v, const uint32_t* __restrict__ clients,
                                                                const uint8_t* __restrict__ actions,
                                                                const uint8_t* __restrict__ tbytes,
                                                                const uint64_t* __restrict__ toffs,
                                                                uint64_t offset_base, uint64_t n,
                                                                uint8_t* __restrict__ verdict_out,
                                                                uint32_t* __restrict__ tag_out,
                                                                unsigned long long* __restrict__ evals_out) {
  const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * AZ_BLOCK + threadIdx.x;
  const uint64_t r = gid / G;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gl = lane % G;        // lane within the request's group
  const uint32_t gbase = lane - gl;    // first lane of the group
  const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << (G & 63u)) - 1ull)) << gbase;
  const bool valid = r < n;

  AzClient c{};
  const AzRange* segs = v.segs;
  const uint8_t* t = tbytes;
  uint32_t tn = 0, act = 0, n_seg = 0;
  uint32_t verdict = AZ_BAD, tag = AZ_TAG_NONE;
  bool done = true;
  if (valid) {
    const uint32_t cl = clients[r];
    act = actions[r];
    const uint64_t o0 = toffs[r], o1 = toffs[r + 1];
    // the client id is compared with the table's size before the table is touched
    // offset_base: offset of tbytes[0] (the host entry point uploads the bytes from offsets[0] on)
    if (cl < v.n_clients && act >= 1 && act <= 2 && o0 >= offset_base && o1 >= o0 && o1 - o0 <= 0xFFFFFFFFull) {
      c = v.clients[cl];
      if (c.present & AZ_REGISTERED) {
        verdict = AZ_NOMATCH;
        t = tbytes + (o0 - offset_base);
        tn = static_cast<uint32_t>(o1 - o0);
        segs = v.segs + static_cast<uint64_t>(cl) * AZ_SEG_STRIDE;
        n_seg = c.n_seg < AZ_SEG_STRIDE ? c.n_seg : AZ_SEG_STRIDE;
        done = n_seg == 0;
      }
    }
  }
  uint32_t s = 0, pos = 0, end = 0;
  if (!done) {
    pos = segs[0].lo;
    end = segs[0].hi < v.n_entries ? segs[0].hi : v.n_entries;
  }
  unsigned long long evals = 0;
  while (__any(!done)) {
    bool hit = false;
    // pos + gl cannot wrap: pos < end <= n_entries < 2^31 (commit refuses more)
    if (!done && pos + gl < end) {
      ++evals;
      hit = az_entry_hit(v, v.entries[pos + gl], c, act, t, tn);
    }
    const unsigned long long b = __ballot(hit) & gmask;
    if (!done) {
      if (b) {
        const uint32_t first = static_cast<uint32_t>(__ffsll(b)) - 1u - gbase;
        const AzRule rule = v.rules[v.entries[pos + first].rule];
        verdict = rule.permission;
        tag = rule.tag;
        done = true;
      } else {
        pos += G;
        if (pos >= end) {
          if (++s >= n_seg) {
            done = true;
          } else {
            pos = segs[s].lo;
            end = segs[s].hi < v.n_entries ? segs[s].hi : v.n_entries;
          }
        }
      }
    }
  }
  if (valid && gl == 0) {
    verdict_out[r] = static_cast<uint8_t>(verdict);
    if (tag_out) tag_out[r] = tag;
  }
  // statistics only (emqx_authz_stats.last_evals): one add per wave
  for (uint32_t d = 32; d; d >>= 1) evals += __shfl_down(evals, d);
  if (lane == 0 && evals) atomicAdd(evals_out, evals);
}

// One block: the numbers of each verdict of a finished call, for the asynchronous form.
constexpr uint32_t AZ_SUM_BLOCK = 1024;
__global__ __launch_bounds__(AZ_SUM_BLOCK) void authz_summary_kernel(const uint8_t* __restrict__ verdict, uint64_t n,
                                                                     const unsigned long long* __restrict__ evals,
                                                                     uint64_t* __restrict__ summary) {
  __shared__ uint32_t part[4][AZ_SUM_BLOCK / 64];
  uint32_t cnt[4] = {0, 0, 0, 0};
  for (uint64_t i = threadIdx.x; i < n; i += AZ_SUM_BLOCK) {
    const uint32_t x = verdict[i] & 3u;
    cnt[0] += x == 0;
    cnt[1] += x == 1;
    cnt[2] += x == 2;
    cnt[3] += x == 3;
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t k = 0; k < 4; ++k) {
    uint32_t x = cnt[k];
    for (uint32_t d = 32; d; d >>= 1) x += __shfl_down(x, d);
    if (lane == 0) part[k][wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tot[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t w = 0; w < AZ_SUM_BLOCK / 64; ++w) tot[k] += part[k][w];
    summary[0] = tot[AZ_BAD] ? 1u : 0u;
    summary[1] = tot[AZ_ALLOW];
    summary[2] = tot[AZ_DENY];
    summary[3] = tot[AZ_NOMATCH];
    summary[4] = tot[AZ_BAD];
    summary[5] = *evals;
    summary[6] = 0;
    summary[7] = 0;
  }
}

}  // namespace

int az_launch_check(const AzView& v, const uint32_t* clients, const uint8_t* actions, const uint8_t* tbytes,
                    const uint64_t* toffs, uint64_t n, uint8_t* verdict_out, uint32_t* tag_out,
                    unsigned long long* evals_out, uint32_t group, uint64_t offset_base, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return 0;
  const uint64_t blocks = (n * group + AZ_BLOCK - 1) / AZ_BLOCK;
  if (blocks > 0x7FFFFFFFull) return static_cast<int>(hipErrorInvalidValue);
  const dim3 grid(static_cast<uint32_t>(blocks)), block(AZ_BLOCK);
  switch (group) {
    case 1:
      authz_check_kernel<1><<<grid, block, 0, s>>>(v, clients, actions, tbytes, toffs, offset_base, n, verdict_out, tag_out,
                                                   evals_out);
      break;
    case 4:
      authz_check_kernel<4><<<grid, block, 0, s>>>(v, clients, actions, tbytes, toffs, offset_base, n, verdict_out, tag_out,
                                                   evals_out);
      break;
    case 16:
      authz_check_kernel<16><<<grid, block, 0, s>>>(v, clients, actions, tbytes, toffs, offset_base, n, verdict_out, tag_out,
                                                   evals_out);
      break;
    case 64:
      authz_check_kernel<64><<<grid, block, 0, s>>>(v, clients, actions, tbytes, toffs, offset_base, n, verdict_out, tag_out,
                                                   evals_out);
      break;
    default:
      return static_cast<int>(hipErrorInvalidValue);
  }
  return static_cast<int>(hipGetLastError());
}

int az_launch_summary(const uint8_t* verdict, uint64_t n, const unsigned long long* evals, uint64_t* summary,
                      void* stream) {
  authz_summary_kernel<<<dim3(1), dim3(AZ_SUM_BLOCK), 0, static_cast<hipStream_t>(stream)>>>(verdict, n, evals, summary);
  return static_cast<int>(hipGetLastError());
}

}  // namespace emqx
