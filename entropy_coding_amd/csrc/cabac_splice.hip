// Splicing residual records into host-recorded substreams on the device (the writer's side).
//
// In the reference every bin of CABACWriter::residual_coding goes straight into the bin encoder, between the bins of the
// syntax elements around it (cabac_writer.cpp:2424-2525; the flags :2766-2803, escapes :2822 / :2843, signs :2871).  Here the
// host records the syntax elements it walks itself as bin records and marks where a transform block's bins belong — a
// *splice*: (position in the substream's host records, block index) — and hands the coefficients over instead of bins.  The
// kernels below put the two together without the block records ever existing on the host:
//   residual sizes pass (cabac_residual.hip)  ->  n_records per block
//   splice_plan_kernel    per substream: running sum of its blocks' sizes at every splice, expanded length, byte-slot size
//   splice_scan_kernel    across substreams: where each expanded substream starts (records, bytes); totals; list check
//   splice_expand_kernel  per substream: its final descriptor, every block's destination, the host records moved apart
//   splice_sync_index_kernel  (rows form, cabac_hip_splice_rows.h) per substream: its hand-over point as an index into its expanded string
//   residual records pass (cabac_residual.hip) writes each block's records at its destination
//   encode kernel (cabac_kernels_v4.hip) on the expanded substreams; bin_count_kernel for the BinCounter totals
// No atomics on the data path (one atomicAdd per splice checks that every block is spliced exactly once).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_kernels.h"

namespace cabac {

namespace {

// block-wide exclusive scan of one 64-bit value per thread (256 threads); returns the exclusive prefix, total in *total
__device__ __forceinline__ uint64_t block_excl_scan256(uint64_t v, uint64_t *wave_sum /* [4] LDS */, uint64_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint64_t base = 0, all = 0;
  for (uint32_t k = 0; k < 4; k++) {
    if (k < wave) base += wave_sum[k];
    all += wave_sum[k];
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

// worst case bytes of n coded records: a record shifts out at most 7 bits (terminate bin; a context bin at most 6,
// contexts.cpp:787-789), finish() up to 4 bytes more, the alignment one; rounded up to the slots' 16-byte alignment
__device__ __forceinline__ uint64_t slot_bytes(uint64_t n_records) { return ((7u * n_records + 7u) / 8u + 8u + 15u) / 16u * 16u; }

}  // namespace

// pre[j + s] = records of the substream's blocks spliced in before splice j (pre[j1 + s] = of all of them).  kDevCount (the
// log's emit on a fixed workspace): the blocks and splices that count are the first *n_dev, a number only the device knows
template <bool kDevCount>
__global__ __launch_bounds__(256) void splice_plan_kernel(const uint64_t *__restrict__ n_dev, uint32_t n_sub, uint32_t n_tu, uint32_t n_splice,
                                                          const cabac_substream_desc *__restrict__ desc,
                                                          const uint32_t *__restrict__ splice_first,
                                                          const cabac_splice *__restrict__ splices,
                                                          const uint32_t *__restrict__ tu_n_records, uint32_t *__restrict__ pre,
                                                          uint32_t *__restrict__ sub_n, uint32_t *__restrict__ sub_cap,
                                                          uint32_t *__restrict__ seen, uint32_t *__restrict__ err) {
  __shared__ uint64_t wave_sum[4];
  const uint32_t s = blockIdx.x;
  if (s >= n_sub) return;
  if (kDevCount) n_tu = n_splice = (uint32_t)*n_dev;
  uint32_t j0 = splice_first[s], j1 = splice_first[s + 1];
  const uint32_t n_host = desc[s].n_records;
  uint64_t carry = 0;
  // a list that is not one: nothing of it is read (the arrays hold n_splice splices and n_splice + n_sub + 1 sums)
  uint32_t bad = (j1 < j0 || j1 > n_splice || (s == 0u && j0 != 0u) || (s + 1u == n_sub && j1 != n_splice)) ? 1u : 0u;
  if (bad) j0 = j1 = 0u;
  for (uint32_t base = j0; base < j1; base += 256u) {
    const uint32_t j = base + threadIdx.x;
    const bool valid = j < j1;
    uint64_t sz = 0;
    if (valid) {
      const cabac_splice sp = splices[j];
      const bool ok = sp.tu < n_tu && sp.at <= n_host && (j == j0 || splices[j - 1].at <= sp.at);
      if (ok) {
        sz = tu_n_records[sp.tu];
        atomicAdd(&seen[sp.tu], 1u);
      } else {
        bad = 1;
      }
    }
    uint64_t total;
    const uint64_t excl = block_excl_scan256(sz, wave_sum, &total);
    if (valid) pre[j + s] = (uint32_t)(carry + excl);
    carry += total;
  }
  const uint64_t expanded = (uint64_t)n_host + carry;
  if (expanded > 0xfffffff0ull || slot_bytes(expanded) > 0xfffffff0ull) bad = 1;
  if (threadIdx.x == 0) {
    pre[j1 + s] = (uint32_t)carry;
    sub_n[s] = (uint32_t)expanded;
    sub_cap[s] = (uint32_t)slot_bytes(expanded);
  }
  if (bad) atomicOr(err, 1u);
}

// every block spliced exactly once (the whole grid looks: one workgroup doing it alone took 0.26 ms for 1.6 M blocks)
template <bool kDevCount>
__global__ __launch_bounds__(256) void splice_seen_kernel(const uint64_t *__restrict__ n_dev, uint32_t n_tu, const uint32_t *__restrict__ seen,
                                                          uint32_t *__restrict__ err) {
  if (kDevCount) n_tu = (uint32_t)*n_dev;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const bool bad = t < n_tu && seen[t] != 1u;
  if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(err, 1u);
}

// one workgroup: exclusive scans over the substreams; the totals {records, bytes} are left in the two shared words
__device__ __forceinline__ void scan_substreams(uint32_t n_sub, const uint32_t *sub_n, const uint32_t *sub_cap, uint64_t *rec_base,
                                                uint64_t *byte_base, uint64_t (&wave_a)[16], uint64_t (&wave_b)[16], uint64_t &carry_a,
                                                uint64_t &carry_b) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) carry_a = carry_b = 0;
  __syncthreads();
  for (uint32_t tile = 0; tile < n_sub; tile += 1024u) {
    const uint32_t s = tile + tid;
    const uint64_t a = s < n_sub ? sub_n[s] : 0, b = s < n_sub ? sub_cap[s] : 0;
    uint64_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t ua = __shfl_up(ia, d), ub = __shfl_up(ib, d);
      if ((int)lane >= d) {
        ia += ua;
        ib += ub;
      }
    }
    if (lane == 63) {
      wave_a[wave] = ia;
      wave_b[wave] = ib;
    }
    __syncthreads();
    uint64_t ba = carry_a, bb = carry_b;
    for (uint32_t k = 0; k < wave; k++) {
      ba += wave_a[k];
      bb += wave_b[k];
    }
    if (s < n_sub) {
      rec_base[s] = ba + ia - a;
      byte_base[s] = bb + ib - b;
    }
    __syncthreads();
    if (tid == 1023) {
      carry_a = ba + ia;
      carry_b = bb + ib;
    }
    __syncthreads();
  }
}

// ... and the totals {records, bytes, error}
__global__ __launch_bounds__(1024) void splice_scan_kernel(uint32_t n_sub, const uint32_t *__restrict__ sub_n,
                                                           const uint32_t *__restrict__ sub_cap,
                                                           uint64_t *__restrict__ rec_base, uint64_t *__restrict__ byte_base,
                                                           const uint32_t *__restrict__ err, uint64_t *__restrict__ totals) {
  __shared__ uint64_t wave_a[16], wave_b[16];
  __shared__ uint64_t carry_a, carry_b;
  scan_substreams(n_sub, sub_n, sub_cap, rec_base, byte_base, wave_a, wave_b, carry_a, carry_b);
  if (threadIdx.x == 0) {
    totals[0] = carry_a;
    totals[1] = carry_b;
    totals[2] = *err ? 1u : 0u;
  }
}

// The scan of a call on a fixed workspace (cabac_hip_workspace.h), with THE GATE as its tail: no host reads the totals, so the
// workgroup that has them decides.  The call is VOIDED when the error word is set (reported as g.err_flag), the log's place pass
// left flags, or a total exceeds its room; the status takes the needs, the flags and the counts; and a voided call's tables are
// emptied — length, slot size and bases 0, the plan write's stop word CABAC_RES_OVERFLOW, the binariser's block order — so that
// everything behind finds empty substreams with zero-capacity slots.
__global__ __launch_bounds__(1024) void splice_scan_gate_kernel(uint32_t n_sub, uint32_t *sub_n, uint32_t *sub_cap, uint64_t *rec_base,
                                                                uint64_t *byte_base, const uint32_t *err, uint64_t *totals, WsGate g) {
  __shared__ uint64_t wave_a[16], wave_b[16];
  __shared__ uint64_t carry_a, carry_b;
  __shared__ uint32_t voided;
  scan_substreams(n_sub, sub_n, sub_cap, rec_base, byte_base, wave_a, wave_b, carry_a, carry_b);
  if (threadIdx.x == 0) {
    const uint64_t rec = carry_a, bytes = carry_b;
    WsState *ws = g.ws;
    uint32_t flags = (*err ? g.err_flag : 0u) | ws->log_flags;
    totals[0] = rec;
    totals[1] = bytes;
    totals[2] = *err ? 1u : 0u;
    cabac_workspace_status st = ws->status;
    if (flags == 0u) {  // the totals of a refused list or log say nothing
      st.records_needed = max(st.records_needed, rec);
      st.slot_bytes_needed = max(st.slot_bytes_needed, bytes);
      if (rec > ws->rec_cap) flags |= CABAC_WS_OVER_RECORDS;
      if (bytes > ws->slot_cap) flags |= CABAC_WS_OVER_SLOTS;
    }
    st.flags |= flags;
    if (flags != 0u) {
      st.n_voided += 1u;
      if (st.first_voided == CABAC_WS_NONE_VOIDED) st.first_voided = st.n_calls;
    }
    st.n_calls += 1u;
    ws->status = st;
    ws->voided = flags != 0u ? 1u : 0u;
    ws->log_flags = 0u;
    voided = flags;
  }
  __syncthreads();
  if (voided == 0u) return;
  if (g.residual_scratch) {  // no block left in the binariser's order: its records pass walks nothing
    const size_t words = g.residual_scratch_bytes / sizeof(uint32_t);
    for (size_t i = threadIdx.x; i < words; i += 1024u) g.residual_scratch[i] = i < kResidualScratchHeader ? 0u : 0xffffffffu;
  }
  for (uint32_t s = threadIdx.x; s < n_sub; s += 1024u) {
    sub_n[s] = 0u;
    sub_cap[s] = 0u;
    rec_base[s] = 0u;
    byte_base[s] = 0u;
    if (g.sub_flag) g.sub_flag[s] = CABAC_RES_OVERFLOW;
  }
}

// the expanded substream: descriptor, block destinations, host records moved to their places.  kGated (a ctx with a fixed
// workspace, cabac_hip_workspace.h): a voided call writes its descriptors — empty: the gate has emptied sub_n, sub_cap and the bases —
// and leaves before anything of the splice list is read
template <bool kGated>
__global__ __launch_bounds__(256) void splice_expand_kernel(const WsState *__restrict__ ws, uint32_t n_sub,
                                                            const cabac_substream_desc *__restrict__ desc,
                                                            const uint16_t *__restrict__ host_records,
                                                            const uint32_t *__restrict__ splice_first,
                                                            const cabac_splice *__restrict__ splices, const uint32_t *__restrict__ pre,
                                                            const uint32_t *__restrict__ sub_n, const uint32_t *__restrict__ sub_cap,
                                                            const uint64_t *__restrict__ rec_base, const uint64_t *__restrict__ byte_base,
                                                            cabac_substream_desc *__restrict__ desc_out, uint64_t *__restrict__ tu_offset,
                                                            uint16_t *__restrict__ records) {
  const uint32_t s = blockIdx.x;
  if (s >= n_sub) return;
  const cabac_substream_desc d = desc[s];
  const uint32_t j0 = splice_first[s], ns = splice_first[s + 1] - j0;
  const uint64_t base = rec_base[s];
  if (threadIdx.x == 0) {
    cabac_substream_desc o = d;
    o.rec_offset = base;
    o.byte_offset = byte_base[s];
    o.n_records = sub_n[s];
    o.byte_capacity = sub_cap[s];
    desc_out[s] = o;
  }
  if (kGated && ws->voided != 0u) return;
  const cabac_splice *sp = splices + j0;
  const uint32_t *p = pre + j0 + s;
  for (uint32_t k = threadIdx.x; k < ns; k += 256u) tu_offset[sp[k].tu] = base + sp[k].at + p[k];
  const uint16_t *src = host_records + d.rec_offset;
  for (uint32_t i = threadIdx.x; i < d.n_records; i += 256u) {
    // the blocks spliced in at or before host record i: the first k splices, k = #(at <= i); `at` is sorted
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sp[mid].at <= i) lo = mid + 1;
      else hi = mid;
    }
    records[base + i + p[lo]] = src[i];
  }
}

// a point (at, splice[i]; splice null: the upper end) of substream s as an index into its expanded string: what the two kernels below say of it
__device__ __forceinline__ uint32_t splice_point_index(uint32_t s, const cabac_substream_desc *__restrict__ desc,
                                                       const uint32_t *__restrict__ splice_first, const cabac_splice *__restrict__ splices,
                                                       const uint32_t *__restrict__ pre, uint32_t at, const uint32_t *__restrict__ splice, uint32_t i) {
  const uint32_t j0 = splice_first[s], ns = splice_first[s + 1] - j0;
  const uint32_t k = min(at, desc[s].n_records);
  const cabac_splice *sp = splices + j0;
  uint32_t lo = 0, hi = ns;  // #{at < k}
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sp[mid].at < k) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t below = lo;
  hi = ns;  // #{at <= k}, from there on
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sp[mid].at <= k) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t m = splice ? min(max(splice[i], below), lo) : lo;
  return k + pre[j0 + s + m];
}

// the hand-over point of every substream (cabac_hip_splice_rows.h) as an index into its expanded string: k host records and m of
// its splices in front, m clipped to [#{at < k}, #{at <= k}] — two bisections of the sorted splices — and the records of those m
// blocks from the running sums of splice_plan_kernel.  One thread per substream; nothing is shared.  kGated: index 0 for every
// substream of a voided call, whose list may be anything
template <bool kGated>
__global__ __launch_bounds__(256) void splice_sync_index_kernel(const WsState *__restrict__ ws, uint32_t n_sub,
                                                                const cabac_substream_desc *__restrict__ desc,
                                                                const uint32_t *__restrict__ splice_first,
                                                                const cabac_splice *__restrict__ splices, const uint32_t *__restrict__ pre,
                                                                const uint32_t *__restrict__ sync_at, const uint32_t *__restrict__ sync_splice,
                                                                uint32_t *__restrict__ sync_rec) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_sub) return;
  if (kGated && ws->voided != 0u) {
    sync_rec[s] = 0u;
    return;
  }
  sync_rec[s] = splice_point_index(s, desc, splice_first, splices, pre, sync_at[s], sync_splice, s);
}

// The same for a LIST of points per substream (cabac_hip_probe.h): probe p of substream s, probe_first[s] <= p < probe_first[s + 1],
// is the pair (probe_at[p], probe_splice[p]).  One thread per probe: a bisection of probe_first for its substream (the last s
// with probe_first[s] <= p — substreams without probes are stepped over), then the two bisections above.
__global__ __launch_bounds__(256) void splice_probe_index_kernel(uint32_t n_sub, uint32_t n_probe,
                                                                 const cabac_substream_desc *__restrict__ desc,
                                                                 const uint32_t *__restrict__ splice_first,
                                                                 const cabac_splice *__restrict__ splices, const uint32_t *__restrict__ pre,
                                                                 const uint32_t *__restrict__ probe_first,
                                                                 const uint32_t *__restrict__ probe_at,
                                                                 const uint32_t *__restrict__ probe_splice, uint32_t *__restrict__ probe_rec) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_probe) return;
  uint32_t lo = 0, hi = n_sub;  // #{s in 1 .. n_sub: probe_first[s] <= p}
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (probe_first[mid + 1u] <= p) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= n_sub) {  // behind probe_first[n_sub]: no substream owns it
    probe_rec[p] = 0u;
    return;
  }
  probe_rec[p] = splice_point_index(lo, desc, splice_first, splices, pre, probe_at[p], probe_splice, p);
}

// BinCounter totals of the expanded substreams (arith_codec.cpp:281-316): per substream 379 context-bin counts, then the
// bypass and the terminate bins
__global__ __launch_bounds__(256) void bin_count_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                        const uint16_t *__restrict__ records, uint32_t *__restrict__ counts) {
  __shared__ uint32_t hist[CABAC_BIN_COUNT_WORDS];
  const uint32_t s = blockIdx.x;
  if (s >= n_sub) return;
  for (uint32_t k = threadIdx.x; k < CABAC_BIN_COUNT_WORDS; k += 256u) hist[k] = 0;
  __syncthreads();
  const cabac_substream_desc d = desc[s];
  const uint16_t *rec = records + d.rec_offset;
  for (uint32_t i = threadIdx.x; i < d.n_records; i += 256u) {
    const uint32_t id = rec[i] & CABAC_REC_ID_MASK;
    if (id < CABAC_NUM_CONTEXTS) atomicAdd(&hist[id], 1u);
    else if (id == CABAC_REC_EP) atomicAdd(&hist[CABAC_NUM_CONTEXTS], 1u);
    else if (id == CABAC_REC_TRM) atomicAdd(&hist[CABAC_NUM_CONTEXTS + 1], 1u);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < CABAC_BIN_COUNT_WORDS; k += 256u) counts[(size_t)s * CABAC_BIN_COUNT_WORDS + k] = hist[k];
}

// descriptor checks the host-pointer entry point leaves to the device (one word per million blocks is cheaper here than a
// host loop): a block whose coefficients would lie outside [0, n_coeff_total) sets *err
__global__ __launch_bounds__(256) void tu_range_check_kernel(uint32_t n_tu, const cabac_tu_desc *__restrict__ tus, uint64_t n_coeff_total,
                                                             uint32_t *__restrict__ err) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_tu) return;
  const cabac_tu_desc d = tus[t];
  if (d.log2_width > 6 || d.log2_height > 6) return;  // flagged by the binariser (CABAC_TU_INFO_BAD_DESC), reads nothing
  const uint64_t n = 1ull << (d.log2_width + d.log2_height);
  if (d.coeff_offset > n_coeff_total || n > n_coeff_total - d.coeff_offset) atomicOr(err, 1u);
}

// any block empty or with a bad descriptor (its splice adds no records; the caller is told)
__global__ __launch_bounds__(256) void tu_info_any_kernel(uint32_t n_tu, const uint32_t *__restrict__ info, uint32_t *__restrict__ flag) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < n_tu && (info[t] & (CABAC_TU_INFO_EMPTY | CABAC_TU_INFO_BAD_DESC))) atomicOr(flag, 1u);
}

hipError_t launch_tu_range_check(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tus, uint64_t n_coeff_total, uint32_t *err) {
  hipError_t e = hipMemsetAsync(err, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if (n_tu) hipLaunchKernelGGL(tu_range_check_kernel, dim3((n_tu + 255u) / 256u), dim3(256), 0, st, n_tu, tus, n_coeff_total, err);
  return hipGetLastError();
}

hipError_t launch_tu_info_any(hipStream_t st, uint32_t n_tu, const uint32_t *info, uint32_t *flag) {
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if (n_tu) hipLaunchKernelGGL(tu_info_any_kernel, dim3((n_tu + 255u) / 256u), dim3(256), 0, st, n_tu, info, flag);
  return hipGetLastError();
}

hipError_t launch_splice_plan(hipStream_t st, uint32_t n_sub, uint32_t n_tu, const cabac_substream_desc *desc,
                              const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_splice,
                              const uint32_t *tu_n_records, uint32_t *pre, uint32_t *sub_n, uint32_t *sub_cap, uint32_t *seen, uint32_t *err,
                              uint64_t *rec_base, uint64_t *byte_base, uint64_t *totals, const uint64_t *n_dev, const WsGate *gate) {
  hipError_t e = hipMemsetAsync(seen, 0, sizeof(uint32_t) * (n_tu ? n_tu : 1u), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(err, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  const dim3 seen_grid((n_tu + 255u) / 256u);
  if (n_sub && n_dev)
    hipLaunchKernelGGL(splice_plan_kernel<true>, dim3(n_sub), dim3(256), 0, st, n_dev, n_sub, n_tu, n_splice, desc, splice_first, splices,
                       tu_n_records, pre, sub_n, sub_cap, seen, err);
  else if (n_sub)
    hipLaunchKernelGGL(splice_plan_kernel<false>, dim3(n_sub), dim3(256), 0, st, nullptr, n_sub, n_tu, n_splice, desc, splice_first, splices,
                       tu_n_records, pre, sub_n, sub_cap, seen, err);
  if (n_tu && n_dev) hipLaunchKernelGGL(splice_seen_kernel<true>, seen_grid, dim3(256), 0, st, n_dev, n_tu, seen, err);
  else if (n_tu) hipLaunchKernelGGL(splice_seen_kernel<false>, seen_grid, dim3(256), 0, st, nullptr, n_tu, seen, err);
  return launch_splice_scan(st, n_sub, sub_n, sub_cap, rec_base, byte_base, err, totals, gate);
}

hipError_t launch_splice_scan(hipStream_t st, uint32_t n_sub, uint32_t *sub_n, uint32_t *sub_cap, uint64_t *rec_base,
                              uint64_t *byte_base, const uint32_t *err, uint64_t *totals, const WsGate *gate) {
  if (gate) hipLaunchKernelGGL(splice_scan_gate_kernel, dim3(1), dim3(1024), 0, st, n_sub, sub_n, sub_cap, rec_base, byte_base, err, totals, *gate);
  else hipLaunchKernelGGL(splice_scan_kernel, dim3(1), dim3(1024), 0, st, n_sub, sub_n, sub_cap, rec_base, byte_base, err, totals);
  return hipGetLastError();
}

hipError_t launch_splice_expand(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *host_records,
                                const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                const uint32_t *sub_n, const uint32_t *sub_cap, const uint64_t *rec_base, const uint64_t *byte_base,
                                cabac_substream_desc *desc_out, uint64_t *tu_offset, uint16_t *records) {
  if (n_sub)
    hipLaunchKernelGGL(splice_expand_kernel<false>, dim3(n_sub), dim3(256), 0, st, nullptr, n_sub, desc, host_records, splice_first, splices,
                       pre, sub_n, sub_cap, rec_base, byte_base, desc_out, tu_offset, records);
  return hipGetLastError();
}

hipError_t launch_splice_expand_gated(hipStream_t st, const WsState *ws, uint32_t n_sub, const cabac_substream_desc *desc,
                                      const uint16_t *host_records, const uint32_t *splice_first, const cabac_splice *splices,
                                      const uint32_t *pre, const uint32_t *sub_n, const uint32_t *sub_cap, const uint64_t *rec_base,
                                      const uint64_t *byte_base, cabac_substream_desc *desc_out, uint64_t *tu_offset, uint16_t *records) {
  if (n_sub)
    hipLaunchKernelGGL(splice_expand_kernel<true>, dim3(n_sub), dim3(256), 0, st, ws, n_sub, desc, host_records, splice_first, splices, pre,
                       sub_n, sub_cap, rec_base, byte_base, desc_out, tu_offset, records);
  return hipGetLastError();
}

hipError_t launch_splice_sync_index(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *splice_first,
                                    const cabac_splice *splices, const uint32_t *pre, const uint32_t *sync_at,
                                    const uint32_t *sync_splice, uint32_t *sync_rec) {
  if (n_sub)
    hipLaunchKernelGGL(splice_sync_index_kernel<false>, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, nullptr, n_sub, desc, splice_first,
                       splices, pre, sync_at, sync_splice, sync_rec);
  return hipGetLastError();
}

hipError_t launch_splice_sync_index_gated(hipStream_t st, const WsState *ws, uint32_t n_sub, const cabac_substream_desc *desc,
                                          const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                          const uint32_t *sync_at, const uint32_t *sync_splice, uint32_t *sync_rec) {
  if (n_sub)
    hipLaunchKernelGGL(splice_sync_index_kernel<true>, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, ws, n_sub, desc, splice_first,
                       splices, pre, sync_at, sync_splice, sync_rec);
  return hipGetLastError();
}

hipError_t launch_splice_probe_index(hipStream_t st, uint32_t n_sub, uint32_t n_probe, const cabac_substream_desc *desc,
                                     const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                     const uint32_t *probe_first, const uint32_t *probe_at, const uint32_t *probe_splice,
                                     uint32_t *probe_rec) {
  if (n_sub && n_probe)
    hipLaunchKernelGGL(splice_probe_index_kernel, dim3((n_probe + 255u) / 256u), dim3(256), 0, st, n_sub, n_probe, desc, splice_first,
                       splices, pre, probe_first, probe_at, probe_splice, probe_rec);
  return hipGetLastError();
}

hipError_t launch_bin_count(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint32_t *counts) {
  if (n_sub) hipLaunchKernelGGL(bin_count_kernel, dim3(n_sub), dim3(256), 0, st, n_sub, desc, records, counts);
  return hipGetLastError();
}

}  // namespace cabac
