// Device binariser: syntax-element records -> bin records (cabac_hip.h, "Syntax-element record").
// Restates the value -> bin-string helpers of the reference:
//   BinEncIf::encodeBinsEP / encodeRemAbsEP          entropy_codec/arith_codec.cpp:401-458
//   CABACWriter::unary_max_symbol / unary_max_eqprob / exp_golomb_eqprob   cabac_writer.cpp:3072-3118
//   CABACWriter::xWriteTruncBinCode                                          cabac_writer.cpp:854-882
// Every helper emits at most one context-coded unary run or two bypass code words, so a syntax
// element is reduced to {n_bins, (code1,len1), (code2,len2) | unary run}; bins are then written by
// OUTPUT position: a workgroup scans the bin counts of a tile of 256 elements, and thread o of the
// tile's output range finds its element by binary search in LDS and extracts its bin.  Reads are 8 B
// per element and writes 2 B per bin, both coalesced: the kernel is HBM-bound by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_rem_abs.hpp"
#include "cabac_kernels.h"
#include "cabac_se_code.h"

namespace cabac {

constexpr int kBzThreads = 256;

__global__ __launch_bounds__(kBzThreads) void binarize_kernel(uint32_t n_sub, const uint64_t *__restrict__ se_offset,
                                                              const uint32_t *__restrict__ se,
                                                              const uint64_t *__restrict__ rec_offset,
                                                              uint32_t *__restrict__ n_records,
                                                              uint16_t *__restrict__ records) {
  __shared__ uint32_t scan[kBzThreads + 1];  // exclusive bin offsets of the tile's elements
  __shared__ uint32_t w0s[kBzThreads], vals[kBzThreads];
  __shared__ uint32_t wave_sum[kBzThreads / 64];
  const uint32_t sub = blockIdx.x;
  if (sub >= n_sub) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t se_begin = se_offset[sub], se_end = se_offset[sub + 1];
  uint16_t *out = records ? records + rec_offset[sub] : nullptr;
  uint32_t produced = 0;  // bins written by earlier tiles (uniform)

  for (uint64_t tile = se_begin; tile < se_end; tile += kBzThreads) {
    const uint64_t e = tile + tid;
    uint32_t w0 = 0xfu, value = 0;  // kind 15: no bins
    if (e < se_end) {
      const uint2 rec = *reinterpret_cast<const uint2 *>(se + 2 * e);
      w0 = rec.x;
      value = rec.y;
    }
    const uint32_t cnt = se_decode(w0, value).n;
    // exclusive scan of cnt over the 256 threads: wave scan + 4 wave totals
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kBzThreads / 64; k++) {
      if (k < (int)wave) wave_base += wave_sum[k];
      total += wave_sum[k];
    }
    scan[tid] = wave_base + incl - cnt;
    w0s[tid] = w0;
    vals[tid] = value;
    if (tid == 0) scan[kBzThreads] = total;
    __syncthreads();
    if (out) {
      // output-position loop: thread o finds its element (largest i with scan[i] <= o) and its bin
      for (uint32_t o = tid; o < total; o += kBzThreads) {
        uint32_t lo = 0, hi = kBzThreads;  // invariant: scan[lo] <= o < scan[hi]
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (scan[mid] <= o) lo = mid;
          else hi = mid;
        }
        const SeCode s = se_decode(w0s[lo], vals[lo]);
        out[produced + o] = se_bin(s, o - scan[lo]);
      }
    }
    produced += total;
    __syncthreads();
  }
  if (tid == 0) n_records[sub] = produced;
}

hipError_t launch_binarize(hipStream_t st, uint32_t n_sub, const uint64_t *se_offset, const uint32_t *se,
                           const uint64_t *rec_offset, uint32_t *n_records, uint16_t *records) {
  if (n_sub == 0) return hipSuccess;
  hipLaunchKernelGGL(binarize_kernel, dim3(n_sub), dim3(kBzThreads), 0, st, n_sub, se_offset, se, rec_offset, n_records,
                     records);
  return hipGetLastError();
}

}  // namespace cabac
