// Search rounds on the device (cabac_hip_search.h): the segmented arg-min that picks the cheapest candidate of every group.
// The other two parts of a round are the fused residual estimator and its exporting variant (cabac_residual_estimate.hip),
// run over all candidates and then over the picked ones; cabac_capi.cpp chains the three on the ctx's stream.
//
// Layout: one GROUP (the candidates [group_first[g], group_first[g + 1])) per 16-lane DPP row, four per wave, sixteen per
// 256-thread workgroup.  A lane walks the candidates first + l, first + l + 16, ... in ascending order and keeps the
// smallest cost it met with a strict comparison, so among equal costs it holds the lowest index; the row then reduces
// (cost, index) pairs with four __shfl_xor steps under the same order.  A group of any size costs size / 16 iterations
// of coalesced 8-byte loads, no host-known maximum is needed, and no workgroup waits for another.
// Reads 8 B (16 B with distortions) per candidate and 8 B per group, writes 12 B per group: memory bound.  No MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_kernels.h"

namespace cabac {

namespace {

constexpr uint32_t kSelRows = 16;  // groups per workgroup (256 threads)
constexpr uint64_t kCostNone = ~0ull, kCostMax = ~0ull - 1ull;

// dist + floor(lambda_q16 * frac_bits / 2^31) with the product taken in 128 bits, saturating at 2^64 - 2
__device__ __forceinline__ uint64_t search_cost(uint64_t dist, uint64_t lambda_q16, uint64_t frac) {
  const uint64_t hi = __umul64hi(lambda_q16, frac), lo = lambda_q16 * frac;
  if ((hi >> 31) != 0ull) return kCostMax;
  const uint64_t rate = (hi << 33) | (lo >> 31);
  const uint64_t sum = dist + rate;
  return (sum < dist || sum > kCostMax) ? kCostMax : sum;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace

__global__ __launch_bounds__(256) void search_select_kernel(uint32_t n_group, uint32_t n_cand_max,
                                                             const uint32_t *__restrict__ group_first,
                                                             const uint64_t *__restrict__ frac_bits, const uint64_t *__restrict__ dist,
                                                             uint64_t lambda_q16, uint32_t *__restrict__ pick, uint64_t *__restrict__ cost) {
  const uint32_t l = threadIdx.x & 15u;
  const uint32_t g = blockIdx.x * kSelRows + (threadIdx.x >> 4);
  uint32_t first = 0, end = 0;
  if (g < n_group) {  // clipped as est_cand_range clips: to the candidates there are, a run that goes backwards is empty
    const uint32_t n = min(group_first[n_group], n_cand_max);
    first = min(group_first[g], n);
    end = max(min(group_first[g + 1u], n), first);
  }
  uint64_t best = kCostNone;
  uint32_t best_c = 0xffffffffu;
  // first + l cannot wrap: first <= end <= 2^32 - 1 and the loop is entered only below end
  for (uint64_t c = (uint64_t)first + l; c < (uint64_t)end; c += 16u) {
    const uint64_t d = dist ? dist[c] : 0ull;
    if (d == kCostNone) continue;  // excluded by the caller
    const uint64_t v = search_cost(d, lambda_q16, frac_bits[c]);
    if (v < best) {
      best = v;
      best_c = (uint32_t)c;
    }
  }
  for (int d = 1; d < 16; d <<= 1) {
    const uint64_t ov = shfl_xor64(best, d);
    const uint32_t oc = (uint32_t)__shfl_xor((int)best_c, d);
    if (ov < best || (ov == best && oc < best_c)) {
      best = ov;
      best_c = oc;
    }
  }
  if (g < n_group && l == 0u) {
    pick[g] = best_c;
    cost[g] = best;
  }
}

hipError_t launch_search_select(hipStream_t st, uint32_t n_group, uint32_t n_cand_max, const uint32_t *group_first,
                                const uint64_t *frac_bits, const uint64_t *dist, uint64_t lambda_q16, uint32_t *pick, uint64_t *cost) {
  if (n_group == 0) return hipSuccess;
  const dim3 grid((n_group + kSelRows - 1u) / kSelRows);
  hipLaunchKernelGGL(search_select_kernel, grid, dim3(256), 0, st, n_group, n_cand_max, group_first, frac_bits, dist, lambda_q16, pick,
                     cost);
  return hipGetLastError();
}

}  // namespace cabac
