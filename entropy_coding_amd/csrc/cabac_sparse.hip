// Sparse coefficient transport (include/cabac_hip_sparse.h): dense transform blocks <-> lists of their non-zero coefficients.
// Both directions are streams over the dense array; the yardstick is memory bandwidth.
//
// The walk every kernel here shares: one 16-lane row per block, four blocks per wave, sixteen per workgroup.  A row walks a run of
// contiguous elements in 16-byte vectors (8 int16 or 4 int32 per lane, 256 bytes per row and trip) laid on the ADDRESS grid, so
// that the vectors inside the run are aligned whatever coeff_offset is; the vector that holds the run's head and the one that
// holds its tail are touched element by element, inside the run only (1 x 2 and 2 x 2 blocks at odd offsets are legal).  The coded
// region of a block up to 32 wide is one run of w * min(h, 32) elements; of a 64-wide block min(h, 32) runs of 32, stride 64.
//
// compact: count launch (non-zero mask, popcount per lane, row sum by DPP -> one count per block, parked in ent_first, and one
// per workgroup) / scan launch (one workgroup: the workgroups' bases, ent_first[n_tu], the status) / write launch (the same
// walk; the block's first from its workgroup's base and the counts of the rows below it, the lane prefix inside the row by DPP,
// entries stored in ascending pos).  expand: zero launch over the blocks' elements / scatter launch, 4 or 16 lanes per block
// looping over its entries / status.  Stream order between the launches is the only ordering; no workgroup waits for another and
// the data path has no atomics (the error words, raised by bad input alone, are an atomicOr and an atomicMax).
#include <hip/hip_runtime.h>

#include "cabac_scan.h"
#include "cabac_sparse_kernels.h"

namespace cabac {
namespace {

constexpr uint32_t kRows = 16;  // blocks per workgroup of 256 threads
constexpr uint32_t kErrWords = 4;  // scratch: [0] flags, [1] ~first_bad (so that zeroes clear both), [2..3] pad; then the counts

__device__ __forceinline__ void raise(uint32_t *err, uint32_t flag, uint32_t t) {
  atomicOr(&err[0], flag);
  atomicMax(&err[1], ~t);
}

struct Blk {
  bool good;
  uint32_t lw, lh;
  uint64_t off;
};

__device__ __forceinline__ Blk load_blk(const cabac_tu_desc *tu, uint32_t t, uint64_t n_total) {
  const uint2 q = reinterpret_cast<const uint2 *>(tu + t)[1];
  Blk b;
  b.off = tu[t].coeff_offset;
  b.lw = q.x & 0xffu;
  b.lh = (q.x >> 8) & 0xffu;
  b.good = b.lw <= 6u && b.lh <= 6u && b.off <= n_total && (uint64_t(1) << ((b.lw + b.lh) & 31u)) <= n_total - b.off;
  return b;
}

template <class T>
struct VecOf {
  static constexpr int V = 16 / (int)sizeof(T);
};

// The vectors of a run of n elements at p, a trip of sixteen per row: f(e0, live) with e0 the run index of the vector's first
// element (negative in the head vector), called by all sixteen lanes of the row the same number of times.
template <class T, class F>
__device__ __forceinline__ void row_walk(const T *p, uint32_t n, uint32_t lane, F &&f) {
  constexpr int V = VecOf<T>::V;
  const uint32_t a = (uint32_t)((reinterpret_cast<uintptr_t>(p) & 15u) / sizeof(T));
  const uint32_t nv = (a + n + V - 1u) / V;
  for (uint32_t k0 = 0; k0 < nv; k0 += 16u) {
    const uint32_t k = k0 + lane;
    f((int)(k * V) - (int)a, k < nv);
  }
}

template <class T>
__device__ __forceinline__ void load_vec(const T *p, uint32_t n, int e0, bool live, int32_t (&v)[VecOf<T>::V]) {
  constexpr int V = VecOf<T>::V;
#pragma unroll
  for (int j = 0; j < V; j++) v[j] = 0;
  if (!live) return;
  if (e0 >= 0 && (uint32_t)e0 + V <= n) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p + e0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if (sizeof(T) == 2) {
#pragma unroll
      for (int j = 0; j < V; j++) v[j] = (int32_t)(int16_t)(uint16_t)(w[(j >> 1) & 3] >> (16 * (j & 1)));
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) v[j] = (int32_t)w[j & 3];
    }
  } else {  // the head or the tail of the run: element by element, inside the run only
#pragma unroll
    for (int j = 0; j < V; j++) {
      const int i = e0 + j;
      if (i >= 0 && (uint32_t)i < n) v[j] = (int32_t)p[i];
    }
  }
}

// the runs of a block's coded region
struct Runs {
  uint32_t n_run, run_len, stride;
};
__device__ __forceinline__ Runs coded_runs(const Blk &b) {
  const uint32_t ch = b.lh < 5u ? (1u << b.lh) : 32u;
  if (b.lw == 6u) return {ch, 32u, 64u};
  return {1u, ch << b.lw, 0u};
}

// ------------------------------------------------------------------------------------------------------------------ compact
template <class T>
__global__ __launch_bounds__(256) void sparse_count_kernel(uint32_t n_tu, const cabac_tu_desc *__restrict__ tu, const T *__restrict__ coeff,
                                                           uint64_t n_total, uint32_t *__restrict__ cnt, uint32_t *__restrict__ wg_cnt,
                                                           uint32_t *err) {
  constexpr int V = VecOf<T>::V;
  __shared__ uint32_t sh[kRows];
  const uint32_t row = threadIdx.x >> 4, lane = threadIdx.x & 15u;
  const uint32_t t = blockIdx.x * kRows + row;
  uint32_t c = 0;
  if (t < n_tu) {
    const Blk b = load_blk(tu, t, n_total);
    if (!b.good) {
      if (lane == 0) raise(err, CABAC_SPARSE_BAD_BLOCK, t);
    } else {
      const Runs r = coded_runs(b);
      bool wide = false;
      for (uint32_t s = 0; s < r.n_run; s++) {
        const T *p = coeff + b.off + s * r.stride;
        row_walk(p, r.run_len, lane, [&](int e0, bool live) {
          int32_t v[V];
          load_vec(p, r.run_len, e0, live, v);
#pragma unroll
          for (int j = 0; j < V; j++) {
            c += v[j] != 0;
            if (sizeof(T) == 4) wide |= v[j] != (int32_t)(int16_t)v[j];
          }
        });
      }
      if (wide) raise(err, CABAC_SPARSE_RANGE, t);
    }
  }
  const uint32_t total = row_sum_below(c) + c;  // lane 15: the block's count
  if (lane == 15u) {
    sh[row] = total;
    if (t < n_tu) cnt[t] = total;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t i = 0; i < kRows; i++) s += sh[i];
    wg_cnt[blockIdx.x] = s;
  }
}

// one workgroup: the exclusive scan of the workgroups' counts in place, ent_first[n_tu] and the status
__global__ __launch_bounds__(1024) void sparse_scan_kernel(uint32_t n_wg, uint32_t *__restrict__ wg_cnt, uint32_t n_tu,
                                                           uint32_t *__restrict__ ent_first, uint64_t capacity, const uint32_t *err,
                                                           cabac_sparse_status *__restrict__ status) {
  __shared__ uint64_t sh[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n_wg + 1023u) / 1024u;
  const uint64_t lo = (uint64_t)tid * per, hi = lo + per < n_wg ? lo + per : n_wg;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; i++) s += wg_cnt[i];
  sh[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const uint64_t add = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  uint64_t run = sh[tid] - s;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t v = wg_cnt[i];
    wg_cnt[i] = (uint32_t)run;
    run += v;
  }
  if (tid == 1023u) {
    const uint64_t total = sh[1023];
    ent_first[n_tu] = (uint32_t)total;
    cabac_sparse_status out;
    out.n_entries = total;
    out.flags = err[0] | (total > capacity ? CABAC_SPARSE_OVERFLOW : 0u);
    out.first_bad = ~err[1];
    *status = out;
  }
}

template <class T>
__global__ __launch_bounds__(256) void sparse_write_kernel(uint32_t n_tu, const cabac_tu_desc *__restrict__ tu, const T *__restrict__ coeff,
                                                           uint64_t n_total, uint32_t *__restrict__ ent_first,
                                                           const uint32_t *__restrict__ wg_base, uint32_t *__restrict__ entries,
                                                           uint64_t capacity) {
  constexpr int V = VecOf<T>::V;
  __shared__ uint32_t sh[kRows];
  const uint32_t row = threadIdx.x >> 4, lane = threadIdx.x & 15u;
  const uint32_t t = blockIdx.x * kRows + row;
  if (lane == 0) sh[row] = t < n_tu ? ent_first[t] : 0u;  // the count the count launch parked there
  __syncthreads();
  uint32_t base = wg_base[blockIdx.x];
  for (uint32_t i = 0; i < row; i++) base += sh[i];
  if (t >= n_tu) return;
  const bool any = sh[row] != 0u;
  if (lane == 0) ent_first[t] = base;
  if (!any) return;  // bad blocks too: their count is 0
  const Blk b = load_blk(tu, t, n_total);
  const Runs r = coded_runs(b);
  for (uint32_t s = 0; s < r.n_run; s++) {
    const T *p = coeff + b.off + s * r.stride;
    row_walk(p, r.run_len, lane, [&](int e0, bool live) {
      int32_t v[V];
      load_vec(p, r.run_len, e0, live, v);
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < V; j++) c += v[j] != 0;
      const uint32_t below = row_sum_below(c);
      const uint32_t trip = (uint32_t)__shfl((int)(below + c), 15, 16);  // the row's count of this trip
      uint64_t at = (uint64_t)base + below;
#pragma unroll
      for (int j = 0; j < V; j++)
        if (v[j] != 0) {
          if (at < capacity) entries[at] = (s * 64u + (uint32_t)(e0 + j)) | ((uint32_t)v[j] << 16);
          at++;
        }
      base += trip;
    });
  }
}

// ------------------------------------------------------------------------------------------------------------------- expand
template <class T>
__global__ __launch_bounds__(256) void sparse_zero_kernel(uint32_t n_tu, const cabac_tu_desc *__restrict__ tu, T *__restrict__ coeff,
                                                          uint64_t n_total, uint32_t *err) {
  constexpr int V = VecOf<T>::V;
  const uint32_t row = threadIdx.x >> 4, lane = threadIdx.x & 15u;
  const uint32_t t = blockIdx.x * kRows + row;
  if (t >= n_tu) return;
  const Blk b = load_blk(tu, t, n_total);
  if (!b.good) {
    if (lane == 0) raise(err, CABAC_SPARSE_BAD_BLOCK, t);
    return;
  }
  const uint32_t n = 1u << (b.lw + b.lh);  // inside n_total: good
  T *p = coeff + b.off;
  row_walk(p, n, lane, [&](int e0, bool live) {
    if (!live) return;
    if (e0 >= 0 && (uint32_t)e0 + V <= n) {
      *reinterpret_cast<uint4 *>(p + e0) = make_uint4(0u, 0u, 0u, 0u);
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int i = e0 + j;
        if (i >= 0 && (uint32_t)i < n) p[i] = 0;
      }
    }
  });
}

template <class T, int LPB>
__global__ __launch_bounds__(256) void sparse_scatter_kernel(uint32_t n_tu, const cabac_tu_desc *__restrict__ tu,
                                                             const uint32_t *__restrict__ ent_first, const uint32_t *__restrict__ entries,
                                                             uint64_t n_entries, T *__restrict__ coeff, uint64_t n_total, uint32_t *err) {
  const uint32_t t = blockIdx.x * (256u / LPB) + threadIdx.x / LPB, lane = threadIdx.x % LPB;
  if (t >= n_tu) return;
  const Blk b = load_blk(tu, t, n_total);
  if (!b.good) return;  // raised by the zero launch
  const uint32_t n = 1u << (b.lw + b.lh);
  uint64_t lo = ent_first[t], hi = ent_first[t + 1];
  bool bad_first = false;
  if (lo > hi) {
    bad_first = true;
    hi = lo;
  }
  if (hi > n_entries) {
    bad_first = true;
    hi = n_entries;
    if (lo > hi) lo = hi;
  }
  if (bad_first && lane == 0) raise(err, CABAC_SPARSE_BAD_FIRST, t);
  T *p = coeff + b.off;
  for (uint64_t k = lo + lane; k < hi; k += LPB) {
    const uint32_t e = entries[k], pos = e & 0xffffu;
    if (pos >= n) raise(err, CABAC_SPARSE_BAD_POS, t);
    else p[pos] = (T)(int16_t)(uint16_t)(e >> 16);  // inside the block, and the block inside n_total
  }
}

__global__ void sparse_expand_status_kernel(uint32_t n_tu, const uint32_t *__restrict__ ent_first, uint64_t n_entries, const uint32_t *err,
                                            cabac_sparse_status *__restrict__ status) {
  const uint64_t last = ent_first[n_tu];
  cabac_sparse_status out;
  out.n_entries = last < n_entries ? last : n_entries;
  out.flags = err[0];
  out.first_bad = ~err[1];
  *status = out;
}

template <class T>
hipError_t expand(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const uint32_t *ent_first, const uint32_t *entries,
                  uint64_t n_entries, T *coeff, uint64_t n_total, cabac_sparse_status *status, uint32_t *err) {
  if (hipError_t e = hipMemsetAsync(err, 0, kErrWords * sizeof(uint32_t), st); e != hipSuccess) return e;
  if (n_tu) {
    hipLaunchKernelGGL(sparse_zero_kernel<T>, dim3((n_tu + kRows - 1u) / kRows), dim3(256), 0, st, n_tu, tu, coeff, n_total, err);
    // a row per block where the lists are long, four lanes where they are short (the residual tiles: 2.7 entries per block)
    if (n_entries / n_tu >= 8u)
      hipLaunchKernelGGL((sparse_scatter_kernel<T, 16>), dim3((n_tu + 15u) / 16u), dim3(256), 0, st, n_tu, tu, ent_first, entries, n_entries,
                         coeff, n_total, err);
    else
      hipLaunchKernelGGL((sparse_scatter_kernel<T, 4>), dim3((n_tu + 63u) / 64u), dim3(256), 0, st, n_tu, tu, ent_first, entries, n_entries,
                         coeff, n_total, err);
  }
  hipLaunchKernelGGL(sparse_expand_status_kernel, dim3(1), dim3(1), 0, st, n_tu, ent_first, n_entries, err, status);
  return hipGetLastError();
}

template <class T>
hipError_t compact(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const T *coeff, uint64_t n_total, uint32_t *ent_first,
                   uint32_t *entries, uint64_t capacity, cabac_sparse_status *status, uint32_t *err) {
  if (hipError_t e = hipMemsetAsync(err, 0, kErrWords * sizeof(uint32_t), st); e != hipSuccess) return e;
  uint32_t *wg_cnt = err + kErrWords;
  const uint32_t n_wg = (n_tu + kRows - 1u) / kRows;
  if (n_wg) hipLaunchKernelGGL(sparse_count_kernel<T>, dim3(n_wg), dim3(256), 0, st, n_tu, tu, coeff, n_total, ent_first, wg_cnt, err);
  hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(1024), 0, st, n_wg, wg_cnt, n_tu, ent_first, capacity, err, status);
  if (n_wg)
    hipLaunchKernelGGL(sparse_write_kernel<T>, dim3(n_wg), dim3(256), 0, st, n_tu, tu, coeff, n_total, ent_first, wg_cnt, entries, capacity);
  return hipGetLastError();
}

}  // namespace

size_t sparse_scratch_bytes(uint32_t n_tu) { return (kErrWords + (size_t(n_tu) + kRows - 1u) / kRows + 1u) * sizeof(uint32_t); }

hipError_t launch_sparse_expand(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const uint32_t *ent_first, const uint32_t *entries,
                                uint64_t n_entries_max, void *coeff, int coeff_bytes, uint64_t n_coeff_total, cabac_sparse_status *status,
                                void *scratch) {
  uint32_t *err = static_cast<uint32_t *>(scratch);
  if (coeff_bytes == 2)
    return expand(st, n_tu, tu, ent_first, entries, n_entries_max, static_cast<int16_t *>(coeff), n_coeff_total, status, err);
  return expand(st, n_tu, tu, ent_first, entries, n_entries_max, static_cast<int32_t *>(coeff), n_coeff_total, status, err);
}

hipError_t launch_sparse_compact(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const void *coeff, int coeff_bytes,
                                 uint64_t n_coeff_total, uint32_t *ent_first, uint32_t *entries, uint64_t entry_capacity,
                                 cabac_sparse_status *status, void *scratch) {
  uint32_t *err = static_cast<uint32_t *>(scratch);
  if (coeff_bytes == 2)
    return compact(st, n_tu, tu, static_cast<const int16_t *>(coeff), n_coeff_total, ent_first, entries, entry_capacity, status, err);
  return compact(st, n_tu, tu, static_cast<const int32_t *>(coeff), n_coeff_total, ent_first, entries, entry_capacity, status, err);
}

}  // namespace cabac
