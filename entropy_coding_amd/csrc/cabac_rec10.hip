// The packed bin records on the device (include/cabac_hip_rec10.h): a block of 64 records is 64 id bytes, a 64-bit plane of the
// ids' bit 8 and a 64-bit plane of the bins, 80 bytes.  Both kernels stream: a lane owns EIGHT consecutive records, i.e. 8 id
// bytes (one dwordx2), one byte of each plane and 16 bytes of 16-bit records (one dwordx4), so a wave covers 8 blocks, 640
// packed bytes against 1 024 bytes of records, every access of a wave contiguous.  The grid is capped and strides over the
// rest.  No workgroup waits for another; nothing is allocated; the only atomics are the vector unit's, on the pack's status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cabac_rec10_kernels.h"

namespace cabac {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxGrid = 256u * 8u;  // eight workgroups a CU; the loop strides over what is left

__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- unpack: records [first, first + n) of a packed buffer.  Groups of eight records are aligned to 8 in the record index, so a
// group that lies inside the range is one 16-byte store (records 16-byte aligned); the two groups the range may cut, and every
// group of a records pointer that is not 16-byte aligned, store their records one by one ----------------------------------------
__global__ __launch_bounds__(kThreads) void rec10_unpack_kernel(const uint8_t *__restrict__ packed, uint64_t first, uint64_t end,
                                                               uint16_t *__restrict__ records) {
  const uint64_t g_first = first >> 3, g_end = (end + 7u) >> 3;
  const bool wide = aligned16(records);
  for (uint64_t g = g_first + uint64_t(blockIdx.x) * kThreads + threadIdx.x; g < g_end; g += uint64_t(gridDim.x) * kThreads) {
    const uint8_t *blk = packed + (g >> 3) * CABAC_REC10_BLOCK_BYTES;
    const uint32_t j = uint32_t(g & 7u);
    const uint2 ids = *reinterpret_cast<const uint2 *>(blk + 8u * j);
    // bit i of m: bit 8 of record i's id; bit 16 + i: its bin
    const uint32_t m = uint32_t(blk[64u + j]) | uint32_t(blk[72u + j]) << 16;
    uint32_t w[4];
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
      const uint32_t two = (p < 2 ? ids.x : ids.y) >> (16u * (p & 1u));  // id bytes of records 2p and 2p + 1
      const uint32_t m_lo = m >> (2u * p), m_hi = m >> (2u * p + 1u);
      const uint32_t lo = (two & 0xFFu) | (m_lo & 1u) << 8 | ((m_lo >> 1) & 0x8000u);
      const uint32_t hi = ((two >> 8) & 0xFFu) | (m_hi & 1u) << 8 | ((m_hi >> 1) & 0x8000u);
      w[p] = lo | hi << 16;
    }
    const uint64_t r0 = g << 3;
    if (wide && r0 >= first && r0 + 8u <= end) {
      *reinterpret_cast<uint4 *>(records + r0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 8; i++) {
        const uint64_t r = r0 + i;
        if (r >= first && r < end) records[r] = uint16_t(w[i >> 1] >> (16u * (i & 1u)));
      }
    }
  }
}

// ---- pack: records [0, n) into ceil(n / 64) whole blocks, the records behind n as zeros.  A lane turns its eight records into 8
// id bytes (one dwordx2 store) and one byte of each plane; the eight lanes of a block then OR their bytes together with three
// exchanges (lanes 1, 2 and 4 apart), and the block's first lane stores both planes as one dwordx4.  Every lane of a wave takes
// part in the exchanges: a lane whose group lies behind the last block carries zeros and stores nothing -------------------------
__global__ void rec10_status_reset_kernel(cabac_rec10_status *status, uint32_t flags) {
  status->first_bad = UINT64_MAX;
  status->flags = flags;
  status->reserved = 0;
}

__global__ __launch_bounds__(kThreads) void rec10_pack_kernel(const uint16_t *__restrict__ records, uint64_t n, uint8_t *__restrict__ packed,
                                                             cabac_rec10_status *status) {
  const uint64_t n_groups = ((n + 63u) >> 6) << 3;  // eight to a block, a multiple of 8: the lanes of a block stay together
  const bool wide = aligned16(records);
  const uint32_t lane = threadIdx.x & 63u, j = lane & 7u;
  // g_wave is the same in all lanes of a wave, so the wave leaves the loop as one
  for (uint64_t g_wave = uint64_t(blockIdx.x) * kThreads + (threadIdx.x & ~63u); g_wave < n_groups; g_wave += uint64_t(gridDim.x) * kThreads) {
    const uint64_t g = g_wave + lane, r0 = g << 3;
    const bool active = g < n_groups;
    uint32_t w[4] = {0, 0, 0, 0};
    if (active && r0 < n) {
      if (wide && r0 + 8u <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(records + r0);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else {
#pragma unroll
        for (uint32_t i = 0; i < 8; i++)
          if (r0 + i < n) w[i >> 1] |= uint32_t(records[r0 + i]) << (16u * (i & 1u));
      }
    }
    const uint32_t bad = (w[0] | w[1] | w[2] | w[3]) & (CABAC_REC10_RESERVED_BITS | CABAC_REC10_RESERVED_BITS << 16);
    if (bad) {  // rare: the smallest index of this lane's eight, then the smallest of all
      uint32_t i = 7;
#pragma unroll
      for (uint32_t k = 7; k-- > 0;)
        if ((w[k >> 1] >> (16u * (k & 1u))) & CABAC_REC10_RESERVED_BITS) i = k;
      atomicMin(reinterpret_cast<unsigned long long *>(&status->first_bad), static_cast<unsigned long long>(r0 + i));
      atomicOr(&status->flags, CABAC_REC10_BAD_BITS);
    }
    uint32_t hi = 0, bin = 0;
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
      hi |= ((w[p] >> 8) & 1u) << (2u * p) | ((w[p] >> 24) & 1u) << (2u * p + 1u);
      bin |= ((w[p] >> 15) & 1u) << (2u * p) | (w[p] >> 31) << (2u * p + 1u);
    }
    const uint2 ids = make_uint2((w[0] & 0xFFu) | ((w[0] >> 8) & 0xFF00u) | (w[1] & 0xFFu) << 16 | ((w[1] << 8) & 0xFF000000u),
                                 (w[2] & 0xFFu) | ((w[2] >> 8) & 0xFF00u) | (w[3] & 0xFFu) << 16 | ((w[3] << 8) & 0xFF000000u));
    // lane j's byte goes to byte j of the plane: to byte j & 3 of a dword, lanes 0..3 making the low and lanes 4..7 the high one
    hi <<= 8u * (j & 3u);
    bin <<= 8u * (j & 3u);
    hi |= __shfl_xor(hi, 1);
    bin |= __shfl_xor(bin, 1);
    hi |= __shfl_xor(hi, 2);
    bin |= __shfl_xor(bin, 2);
    const uint32_t hi_up = __shfl_xor(hi, 4), bin_up = __shfl_xor(bin, 4);
    if (active) {
      uint8_t *blk = packed + (g >> 3) * CABAC_REC10_BLOCK_BYTES;
      *reinterpret_cast<uint2 *>(blk + 8u * j) = ids;
      if (j == 0) *reinterpret_cast<uint4 *>(blk + 64u) = make_uint4(hi, hi_up, bin, bin_up);
    }
  }
}

uint32_t grid_for(uint64_t lanes) { return uint32_t(std::min<uint64_t>((lanes + kThreads - 1) / kThreads, kMaxGrid)); }

}  // namespace

hipError_t launch_rec10_unpack(hipStream_t st, const uint8_t *packed, uint64_t first, uint64_t n, uint16_t *records) {
  if (n == 0) return hipSuccess;
  const uint64_t end = first + n, groups = ((end + 7u) >> 3) - (first >> 3);
  hipLaunchKernelGGL(rec10_unpack_kernel, dim3(grid_for(groups)), dim3(kThreads), 0, st, packed, first, end, records);
  return hipGetLastError();
}

hipError_t launch_rec10_pack(hipStream_t st, const uint16_t *records, uint64_t n, uint8_t *packed, uint64_t packed_capacity,
                             cabac_rec10_status *status) {
  const bool fits = packed_capacity >= CABAC_REC10_BYTES(n);
  hipLaunchKernelGGL(rec10_status_reset_kernel, dim3(1), dim3(1), 0, st, status, fits ? 0u : CABAC_REC10_OVERFLOW);
  if (fits && n) hipLaunchKernelGGL(rec10_pack_kernel, dim3(grid_for(((n + 63u) >> 6) << 3)), dim3(kThreads), 0, st, records, n, packed, status);
  return hipGetLastError();
}

}  // namespace cabac
