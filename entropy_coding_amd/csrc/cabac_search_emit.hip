// The winner log (cabac_hip_search_emit.h): the candidates a search round picked are copied behind one another on the device, and
// at the end every chain's entries are laid out as one record string with splices for the pipeline of cabac_splice.hip.
//
// APPEND, three launches in stream order (stream order is the only synchronisation; no atomics, no LDS staging of data):
//   log_sizes_kernel   one group per 16-lane row: n_rec, n_tu and n_coeff of the picked candidate under the clipping rules of
//                      cabac_hip_search_unit.h, lanes over the candidate's blocks, a row reduction
//   log_scan_kernel    one workgroup: exclusive sums over the groups of entries / records / blocks / coefficients, the capacity
//                      check against the log's cursors, the entries with their per-chain bases, the cursors advanced — or the
//                      overflow flag and nothing else (the pattern of splice_scan_kernel)
//   log_copy_kernel    records, descriptors and positions by a row per group; the COEFFICIENTS — nearly all of the bytes — by
//                      destination bytes: a workgroup takes 4 KiB of the destination (256 aligned 16-byte units, one per thread),
//                      finds the group its first coefficient belongs to by bisection of the groups' sums; every thread bisects on
//                      from there to the group of its own unit and walks that group's blocks to the one that holds it; it moves
//                      its unit with one 16-byte load and store where the unit lies within one block and the source is 16-byte
//                      aligned too, and coefficient by coefficient otherwise (the head and tail of a block, int16_t blocks at odd
//                      offsets, a unit that several tiny blocks share).  A 64 x 64 winner is spread over 4 (int16_t: 2) workgroups, a
//                      hundred 4 x 4 winners share one or two.  Memory bound: every logged byte is read once and written once.
// PLACE, at encode time: log_place_scan_kernel (exclusive sums over the chains' record and block counts: descriptors and
// splice_first) and log_place_move_kernel (a row per entry: its records to their place in the chain's string, its splices).
// On a ctx with a fixed workspace (cabac_hip_workspace.h) the place pass is log_place_scan_fixed_kernel / log_place_move_fixed_kernel:
// the same layout from counters that stay on the device, launched over the log's capacities.
// MARK (cabac_hip_splice_rows.h): log_mark_kernel copies the listed chains' cursors into their hand-over words.
// No MFMA anywhere: there is no arithmetic to speak of.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cabac_hip_search_emit.h"
#include "cabac_kernels.h"

namespace cabac {

namespace {

constexpr uint32_t kRows = 16;         // 16-lane rows per 256-thread workgroup
constexpr uint32_t kUnitBytes = 16;    // what one thread of the coefficient copy moves
constexpr uint32_t kCopyGridMax = 2048;

// blocks / side records of candidate c, clipped as cabac_residual_estimate.hip clips them (est_cand_range, est_side_range)
__device__ __forceinline__ void cand_range(const uint32_t *cand_first, uint32_t n_cand, uint32_t c, uint32_t &first, uint32_t &end) {
  const uint32_t n_tu = cand_first[n_cand];
  first = min(cand_first[c], n_tu);
  end = max(min(cand_first[c + 1u], n_tu), first);
}

__device__ __forceinline__ void side_range(const uint64_t *rec_first, uint32_t n_cand, uint32_t c, uint64_t &first, uint32_t &n) {
  const uint64_t n_all = rec_first[n_cand];
  first = min(rec_first[c], n_all);
  const uint64_t end = max(min(rec_first[c + 1u], n_all), first);
  n = (uint32_t)min(end - first, (uint64_t)0xffffffffu);
}

// coefficients of a block from the second word of its descriptor (log2_width, log2_height: its low bytes); 0 for a bad size
__device__ __forceinline__ uint32_t block_coeffs(uint64_t hi) {
  const uint32_t lw = (uint32_t)hi & 0xffu, lh = (uint32_t)(hi >> 8) & 0xffu;
  return (lw > 6u || lh > 6u) ? 0u : 1u << (lw + lh);
}

__device__ __forceinline__ uint64_t row_sum(uint64_t v) {
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// exclusive scan of N values per thread over a 1024-thread workgroup, continued over tiles through carry[]; one call per tile
template <int N>
__device__ __forceinline__ void scan_tile1024(const uint64_t (&v)[N], uint64_t (&excl)[N], uint64_t (*wave_sum)[16], uint64_t *carry) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t incl[N];
#pragma unroll
  for (int k = 0; k < N; k++) incl[k] = v[k];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      const uint64_t up = __shfl_up(incl[k], d);
      if ((int)lane >= d) incl[k] += up;
    }
  }
  if (lane == 63u) {
#pragma unroll
    for (int k = 0; k < N; k++) wave_sum[k][wave] = incl[k];
  }
  __syncthreads();
  uint64_t base[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    base[k] = carry[k];
    for (uint32_t w = 0; w < wave; w++) base[k] += wave_sum[k][w];
    excl[k] = base[k] + incl[k] - v[k];
  }
  __syncthreads();
  if (tid == 1023u) {
#pragma unroll
    for (int k = 0; k < N; k++) carry[k] = base[k] + incl[k];
  }
  __syncthreads();
}

}  // namespace

size_t search_log_scratch_bytes(uint32_t n_group) { return search_log_scratch(nullptr, n_group).bytes; }

// ---- append (a): sizes ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void log_sizes_kernel(uint32_t n_group, const uint32_t *__restrict__ pick,
                                                        const uint32_t *__restrict__ group_chain, uint32_t n_chain, uint32_t n_cand,
                                                        const uint32_t *__restrict__ cand_first, const cabac_tu_desc *__restrict__ tus,
                                                        const uint64_t *__restrict__ rec_first, SearchLogScratch s) {
  const uint32_t l = threadIdx.x & 15u;
  const uint32_t g = blockIdx.x * kRows + (threadIdx.x >> 4);
  uint32_t chain = 0xffffffffu, first = 0, end = 0, n_rec = 0;
  uint64_t rec0 = 0;
  if (g < n_group) {
    const uint32_t c = pick[g], ch = group_chain[g];  // CABAC_SEARCH_NONE and CABAC_SEARCH_NO_CHAIN fail these comparisons too
    if (c < n_cand && ch < n_chain) {
      chain = ch;
      cand_range(cand_first, n_cand, c, first, end);
      side_range(rec_first, n_cand, c, rec0, n_rec);
    }
  }
  uint64_t n = 0;
  for (uint64_t t = (uint64_t)first + l; t < (uint64_t)end; t += 16u) n += block_coeffs(reinterpret_cast<const uint64_t *>(tus)[2u * t + 1u]);
  n = row_sum(n);
  if (g < n_group && l == 0u) {
    s.chain[g] = chain;
    s.n_rec[g] = n_rec;
    s.n_tu[g] = end - first;
    s.tu_src[g] = first;
    s.rec_src[g] = rec0;
    s.n_coeff[g] = n;
  }
}

// ---- append (b): scan, capacity, entries, cursors ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void log_scan_kernel(uint32_t n_group, SearchLogScratch s, SearchLogArrays log) {
  __shared__ uint64_t wave_sum[4][16];
  __shared__ uint64_t carry[4];
  __shared__ uint32_t chain_over, ok;
  __shared__ uint64_t base[4];
  const uint32_t tid = threadIdx.x;
  if (tid == 0u) {
    carry[0] = carry[1] = carry[2] = carry[3] = 0;
    chain_over = 0;
  }
  __syncthreads();
  for (uint32_t tile = 0; tile < n_group; tile += 1024u) {
    const uint32_t g = tile + tid;
    uint64_t v[4] = {0, 0, 0, 0}, excl[4];
    if (g < n_group) {
      const uint32_t ch = s.chain[g];
      if (ch != 0xffffffffu) {
        v[0] = 1;
        v[1] = s.n_rec[g];
        v[2] = s.n_tu[g];
        v[3] = s.n_coeff[g];
        if ((uint64_t)log.chain_rec[ch] + v[1] > 0xffffffffull) chain_over = 1u;  // every writer writes the same value
      }
    }
    scan_tile1024<4>(v, excl, wave_sum, carry);
    if (g < n_group) {  // relative to what the log holds; the bases are added below once the call is known to fit
      s.entry[g] = (uint32_t)excl[0];
      s.rec_dst[g] = excl[1];
      s.tu_dst[g] = (uint32_t)excl[2];
      s.co_dst[g] = excl[3];
    }
  }
  if (tid == 0u) {
    const cabac_search_log_counters cnt = *log.counters;
    uint32_t over = 0;
    if (cnt.n_entry + carry[0] > log.entry_cap) over |= CABAC_SEARCH_LOG_OVER_ENTRIES;
    if (cnt.n_record + carry[1] > log.record_cap) over |= CABAC_SEARCH_LOG_OVER_RECORDS;
    if (cnt.n_tu + carry[2] > log.tu_cap) over |= CABAC_SEARCH_LOG_OVER_BLOCKS;
    if (cnt.n_coeff + carry[3] > log.coeff_cap) over |= CABAC_SEARCH_LOG_OVER_COEFFS;
    if (chain_over) over |= CABAC_SEARCH_LOG_OVER_CHAIN_RECORDS;
    ok = over ? 0u : 1u;
    base[0] = cnt.n_entry;
    base[1] = cnt.n_record;
    base[2] = cnt.n_tu;
    base[3] = cnt.n_coeff;
    s.co_dst[n_group] = carry[3];
    s.hdr[0] = ok;
    s.hdr[1] = cnt.n_coeff;
    s.hdr[2] = carry[3];
    if (over) {
      log.counters->flags = cnt.flags | CABAC_SEARCH_LOG_OVERFLOW | over;
    } else {
      log.counters->n_entry = cnt.n_entry + carry[0];
      log.counters->n_record = cnt.n_record + carry[1];
      log.counters->n_tu = cnt.n_tu + carry[2];
      log.counters->n_coeff = cnt.n_coeff + carry[3];
    }
  }
  __syncthreads();
  if (!ok) return;
  for (uint32_t g = tid; g < n_group; g += 1024u) {
    const uint32_t ch = s.chain[g];
    if (ch == 0xffffffffu) continue;
    const uint32_t n_rec = s.n_rec[g], n_tu = s.n_tu[g];
    const uint64_t rec_dst = base[1] + s.rec_dst[g];
    const uint32_t tu_dst = (uint32_t)(base[2] + s.tu_dst[g]);
    const uint32_t chain_rec = log.chain_rec[ch], chain_tu = log.chain_tu[ch];  // one appending group per chain and call
    cabac_search_log_entry e;
    e.rec_first = rec_dst;
    e.chain = ch;
    e.n_rec = n_rec;
    e.n_tu = n_tu;
    e.tu_first = tu_dst;
    e.chain_rec_first = chain_rec;
    e.chain_tu_first = chain_tu;
    log.entries[base[0] + s.entry[g]] = e;
    log.chain_rec[ch] = chain_rec + n_rec;
    log.chain_tu[ch] = chain_tu + n_tu;
    s.rec_dst[g] = rec_dst;
    s.tu_dst[g] = tu_dst;
  }
}

// ---- append (c): copy -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void log_copy_kernel(uint32_t n_group, const cabac_tu_desc *__restrict__ tus, const T *__restrict__ coeff,
                                                       const uint16_t *__restrict__ records, const uint32_t *__restrict__ tu_at,
                                                       SearchLogScratch s, SearchLogArrays log) {
  if (s.hdr[0] == 0ull) return;  // the call did not fit: nothing of it is appended
  const uint64_t co_base = s.hdr[1], co_total = s.hdr[2];
  const uint32_t tid = threadIdx.x, l = tid & 15u;
  T *const dst_coeff = static_cast<T *>(log.coeff);

  // records, descriptors, positions: a row per group
  for (uint64_t g = (uint64_t)blockIdx.x * kRows + (tid >> 4); g < n_group; g += (uint64_t)gridDim.x * kRows) {
    if (s.chain[g] == 0xffffffffu) continue;
    const uint32_t n_rec = s.n_rec[g], n_tu = s.n_tu[g];
    const uint64_t tu_src = s.tu_src[g], tu_dst = s.tu_dst[g], rec_src = s.rec_src[g], rec_dst = s.rec_dst[g];
    uint64_t co_at = co_base + s.co_dst[g];  // row-uniform: where the next tile of 16 blocks starts in the log's coefficients
    uint32_t at_prev = 0;                    // row-uniform: the effective position of the block in front of the tile
    for (uint32_t tile = 0; tile < n_tu; tile += 16u) {
      const uint32_t i = tile + l;
      const bool valid = i < n_tu;
      uint64_t d_hi = 0;  // the descriptor's second word: sizes, channel, flags — kept as it is
      uint32_t n = 0, at = 0;
      if (valid) {
        d_hi = reinterpret_cast<const uint64_t *>(tus)[2u * (tu_src + i) + 1u];
        n = block_coeffs(d_hi);
        at = tu_at ? tu_at[tu_src + i] : 0xffffffffu;
      }
      uint32_t incl = n;  // at most 16 * 4096
      for (int dd = 1; dd < 16; dd <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, dd, 16), um = (uint32_t)__shfl_up((int)at, dd, 16);
        if ((int)l >= dd) {
          incl += up;
          at = max(at, um);
        }
      }
      at = max(at, at_prev);
      if (valid) {
        *reinterpret_cast<ulonglong2 *>(log.tu + tu_dst + i) = make_ulonglong2(co_at + incl - n, d_hi);  // coeff_offset rebased
        log.tu_at[tu_dst + i] = min(at, n_rec);
      }
      co_at += (uint32_t)__shfl((int)incl, 15, 16);
      at_prev = (uint32_t)__shfl((int)at, 15, 16);
    }
    for (uint64_t i = l; i < n_rec; i += 16u) log.records[rec_dst + i] = records[rec_src + i];
  }

  // coefficients: by destination bytes.  Unit u = the aligned 16 bytes [16 u, 16 u + 16) counted from the aligned address at or
  // below the call's first coefficient; `lead` coefficients of unit 0 lie in front of the call (they are not touched).
  constexpr uint32_t kPer = kUnitBytes / sizeof(T);
  const uint32_t lead = (uint32_t)(co_base & (kPer - 1u));
  const uint64_t n_unit = co_total ? (co_total + lead + kPer - 1u) / kPer : 0u, n_chunk = (n_unit + 255u) / 256u;
  for (uint64_t k = blockIdx.x; k < n_chunk; k += gridDim.x) {
    // coefficients [c0, ..) of the call are the chunk's, [e0, e1) this thread's (empty for a thread behind the end)
    const uint64_t cv0 = k * 256u * kPer;
    const uint64_t c0 = max(cv0, (uint64_t)lead) - lead;
    const uint64_t v0 = cv0 + (uint64_t)tid * kPer;
    const uint64_t e0 = min(max(v0, (uint64_t)lead) - lead, co_total), e1 = min(v0 + kPer - lead, co_total);
    // the group that holds coefficient c0, for the whole workgroup (uniform loads): co_dst[lo] <= c0 < co_dst[hi] throughout
    // (co_dst[0] = 0, co_dst[n_group] = co_total > c0) ...
    uint32_t lo = 0, hi = n_group;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (s.co_dst[mid] <= c0) lo = mid;
      else hi = mid;
    }
    if (e0 >= e1) continue;
    // ... and from there the group that holds e0, for this thread: the lanes search side by side, so the cost of a chunk does not
    // grow with the number of winners that share it
    hi = n_group;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (s.co_dst[mid] <= e0) lo = mid;
      else hi = mid;
    }
    uint32_t g = lo, i = 0, n_tu = s.n_tu[g];
    uint64_t b0 = s.co_dst[g], tu_src = s.tu_src[g];
    for (uint64_t pos = e0; pos < e1;) {
      // the block that holds pos: the blocks of g from i on, then those of the groups behind it (pos < co_total: there is one)
      const uint64_t *w;
      uint32_t n;
      for (;;) {
        if (i == n_tu) {
          g++;
          i = 0;
          n_tu = s.n_tu[g];
          tu_src = s.tu_src[g];
          b0 = s.co_dst[g];
          continue;
        }
        w = reinterpret_cast<const uint64_t *>(tus + tu_src + i);
        n = block_coeffs(w[1]);
        if (pos < b0 + n) break;
        b0 += n;
        i++;
      }
      const uint64_t m1 = min(e1, b0 + n);
      const T *src = coeff + w[0] + (pos - b0);
      T *dst = dst_coeff + co_base + pos;
      if (m1 - pos == kPer && (reinterpret_cast<uintptr_t>(src) & (kUnitBytes - 1u)) == 0u) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);  // dst is a whole aligned unit then
      } else {
        for (uint32_t j = 0; j < (uint32_t)(m1 - pos); j++) dst[j] = src[j];
      }
      pos = m1;
    }
  }
}

// ---- place ------------------------------------------------------------------------------------------------------------------
// one workgroup: where every chain's record string and splice list start; desc_out[k] = {rec_base, 0, n_records, 0, qp, init_id}
__global__ __launch_bounds__(1024) void log_place_scan_kernel(uint32_t n_chain, const cabac_substream_desc *__restrict__ desc,
                                                              const uint32_t *__restrict__ chain_rec, const uint32_t *__restrict__ chain_tu,
                                                              uint64_t n_tu_total, cabac_substream_desc *__restrict__ desc_out,
                                                              uint32_t *__restrict__ splice_first) {
  __shared__ uint64_t wave_sum[2][16];
  __shared__ uint64_t carry[2];
  const uint32_t tid = threadIdx.x;
  if (tid == 0u) carry[0] = carry[1] = 0;
  __syncthreads();
  for (uint32_t tile = 0; tile < n_chain; tile += 1024u) {
    const uint32_t k = tile + tid;
    uint64_t v[2] = {0, 0}, excl[2];
    if (k < n_chain) {
      v[0] = chain_rec[k];
      v[1] = chain_tu[k];
    }
    scan_tile1024<2>(v, excl, wave_sum, carry);
    if (k < n_chain) {
      cabac_substream_desc o;
      o.rec_offset = excl[0];
      o.byte_offset = 0;
      o.n_records = (uint32_t)v[0];
      o.byte_capacity = 0;
      o.qp = desc[k].qp;
      o.init_id = desc[k].init_id;
      desc_out[k] = o;
      splice_first[k] = (uint32_t)min(excl[1], n_tu_total);
    }
  }
  if (tid == 0u) splice_first[n_chain] = (uint32_t)min(carry[1], n_tu_total);
}

// a row per entry: its records behind those of its chain's earlier entries, its blocks' splices behind theirs.  An entry that does
// not lie within what its chain counts (two groups named one chain in one call) is left out: the splice list is then incomplete
// and the pipeline refuses it.
__global__ __launch_bounds__(256) void log_place_move_kernel(uint32_t n_entry, SearchLogArrays log, uint64_t n_record_total,
                                                             uint64_t n_tu_total, const cabac_substream_desc *__restrict__ desc_out,
                                                             const uint32_t *__restrict__ splice_first, uint16_t *__restrict__ records,
                                                             cabac_splice *__restrict__ splices) {
  const uint32_t l = threadIdx.x & 15u;
  const uint32_t i = blockIdx.x * kRows + (threadIdx.x >> 4);
  if (i >= n_entry) return;
  const cabac_search_log_entry e = log.entries[i];
  if (e.chain >= log.n_chain) return;
  if ((uint64_t)e.chain_rec_first + e.n_rec > log.chain_rec[e.chain] || (uint64_t)e.chain_tu_first + e.n_tu > log.chain_tu[e.chain] ||
      e.rec_first + e.n_rec > n_record_total || (uint64_t)e.tu_first + e.n_tu > n_tu_total)
    return;
  const uint64_t rec_to = desc_out[e.chain].rec_offset + e.chain_rec_first;
  for (uint64_t k = l; k < e.n_rec; k += 16u) records[rec_to + k] = log.records[e.rec_first + k];
  const uint64_t sp_to = (uint64_t)splice_first[e.chain] + e.chain_tu_first;
  for (uint32_t k = l; k < e.n_tu; k += 16u) {
    cabac_splice sp;
    sp.at = e.chain_rec_first + log.tu_at[e.tu_first + k];
    sp.tu = e.tu_first + k;
    splices[sp_to + k] = sp;
  }
}

// ---- place, sized from the log's capacities (cabac_hip_workspace.h) -------------------------------------------------------------
// The counters stay on the device.  log_place_scan_fixed_kernel takes them (a log that overflowed or whose counters exceed its
// capacities counts as empty and leaves its flags for the gate), log_place_move_fixed_kernel runs a row per entry the log could
// hold and gives the binariser tu_cap descriptors: the logged ones, then ones it rejects.  The splice list is the logged blocks'
// alone: the splice kernels take their number from ws->log_tu.
__global__ __launch_bounds__(1024) void log_place_scan_fixed_kernel(SearchLogArrays log, WsState *__restrict__ ws,
                                                                    const cabac_substream_desc *__restrict__ desc,
                                                                    cabac_substream_desc *__restrict__ desc_out,
                                                                    uint32_t *__restrict__ splice_first, cabac_splice *__restrict__ splices) {
  __shared__ uint64_t wave_sum[2][16];
  __shared__ uint64_t carry[2];
  const uint32_t tid = threadIdx.x, n_chain = log.n_chain;
  const cabac_search_log_counters cnt = *log.counters;
  uint32_t flags = (cnt.flags & CABAC_SEARCH_LOG_OVERFLOW) ? CABAC_WS_LOG_OVERFLOW : 0u;
  if (cnt.n_entry > log.entry_cap || cnt.n_record > log.record_cap || cnt.n_tu > log.tu_cap || cnt.n_coeff > log.coeff_cap)
    flags |= CABAC_WS_LOG_DAMAGED;
  const uint64_t n_tu_total = flags ? 0u : cnt.n_tu;
  if (tid == 0u) {
    carry[0] = carry[1] = 0;
    ws->log_entry = flags ? 0u : cnt.n_entry;
    ws->log_record = flags ? 0u : cnt.n_record;
    ws->log_tu = n_tu_total;
    ws->log_flags = flags;
  }
  __syncthreads();
  for (uint32_t tile = 0; tile < n_chain; tile += 1024u) {
    const uint32_t k = tile + tid;
    uint64_t v[2] = {0, 0}, excl[2];
    if (k < n_chain && flags == 0u) {
      v[0] = log.chain_rec[k];
      v[1] = log.chain_tu[k];
    }
    scan_tile1024<2>(v, excl, wave_sum, carry);
    if (k < n_chain) {
      cabac_substream_desc o;
      o.rec_offset = min(excl[0], log.record_cap);  // a chain count the log cannot hold: the move leaves its entries out
      o.byte_offset = 0;
      o.n_records = (uint32_t)min(v[0], log.record_cap - o.rec_offset);
      o.byte_capacity = 0;
      o.qp = desc[k].qp;
      o.init_id = desc[k].init_id;
      desc_out[k] = o;
      splice_first[k] = (uint32_t)min(excl[1], n_tu_total);
    }
  }
  if (tid == 0u) splice_first[n_chain] = (uint32_t)min(carry[1], n_tu_total);
  // a splice of a logged block that no entry fills names no block: the pipeline refuses the list (those behind are never read)
  cabac_splice none;
  none.at = none.tu = 0xffffffffu;
  for (uint64_t t = tid; t < n_tu_total; t += 1024u) splices[t] = none;
}

__global__ __launch_bounds__(256) void log_place_move_fixed_kernel(SearchLogArrays log, const WsState *__restrict__ ws,
                                                                   const cabac_substream_desc *__restrict__ desc_out,
                                                                   const uint32_t *__restrict__ splice_first, uint16_t *__restrict__ records,
                                                                   cabac_splice *__restrict__ splices, cabac_tu_desc *__restrict__ tus_out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // a descriptor per thread: a copy (the log is not written), or a rejected one
  if (t < log.tu_cap) {
    cabac_tu_desc d{};
    d.log2_width = d.log2_height = 7;
    if (t < ws->log_tu) d = log.tu[t];
    tus_out[t] = d;
  }
  const uint32_t l = threadIdx.x & 15u;
  const uint32_t i = blockIdx.x * kRows + (threadIdx.x >> 4);
  if (i >= ws->log_entry) return;
  const uint64_t n_record_total = ws->log_record, n_tu_total = ws->log_tu;
  const cabac_search_log_entry e = log.entries[i];
  if (e.chain >= log.n_chain) return;
  if ((uint64_t)e.chain_rec_first + e.n_rec > desc_out[e.chain].n_records || (uint64_t)e.chain_tu_first + e.n_tu > log.chain_tu[e.chain] ||
      e.rec_first + e.n_rec > n_record_total || (uint64_t)e.tu_first + e.n_tu > n_tu_total)
    return;
  const uint64_t rec_to = desc_out[e.chain].rec_offset + e.chain_rec_first;
  for (uint64_t k = l; k < e.n_rec; k += 16u) records[rec_to + k] = log.records[e.rec_first + k];
  const uint64_t sp_to = (uint64_t)splice_first[e.chain] + e.chain_tu_first;
  if (sp_to + e.n_tu > n_tu_total) return;  // chain counts that do not add up: the list stays incomplete and is refused
  for (uint32_t k = l; k < e.n_tu; k += 16u) {
    cabac_splice sp;
    sp.at = e.chain_rec_first + log.tu_at[e.tu_first + k];
    sp.tu = e.tu_first + k;
    splices[sp_to + k] = sp;
  }
}

// ---- mark (cabac_hip_splice_rows.h) --------------------------------------------------------------------------------------------
// the hand-over point of every listed chain: its cursors as they stand in stream order (a dropped append left them unchanged)
__global__ __launch_bounds__(256) void log_mark_kernel(uint32_t n, const uint32_t *__restrict__ chain, SearchLogArrays log) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t ch = chain[i];
  if (ch >= log.n_chain) return;  // 0xffffffff too
  log.mark_rec[ch] = log.chain_rec[ch];
  log.mark_tu[ch] = log.chain_tu[ch];
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
hipError_t launch_search_log_reset(hipStream_t st, const SearchLogArrays &log) {
  hipError_t e = hipMemsetAsync(log.counters, 0, sizeof(cabac_search_log_counters), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(log.chain_rec, 0, sizeof(uint32_t) * log.n_chain, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(log.chain_tu, 0, sizeof(uint32_t) * log.n_chain, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(log.mark_rec, 0xff, sizeof(uint32_t) * log.n_chain, st);  // every mark: the end of the chain
  if (e != hipSuccess) return e;
  return hipMemsetAsync(log.mark_tu, 0xff, sizeof(uint32_t) * log.n_chain, st);
}

hipError_t launch_search_log_mark(hipStream_t st, const SearchLogArrays &log, uint32_t n, const uint32_t *chain) {
  if (n) hipLaunchKernelGGL(log_mark_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, chain, log);
  return hipGetLastError();
}

hipError_t launch_search_log_append(hipStream_t st, const SearchLogArrays &log, uint32_t n_group, const uint32_t *pick,
                                    const uint32_t *group_chain, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                    const void *coeff, int coeff_bytes, const uint64_t *rec_first, const uint16_t *records,
                                    const uint32_t *tu_at, void *scratch) {
  if (n_group == 0) return hipSuccess;
  const SearchLogScratch s = search_log_scratch(scratch, n_group);
  const uint32_t rows = (n_group + kRows - 1u) / kRows;
  hipLaunchKernelGGL(log_sizes_kernel, dim3(rows), dim3(256), 0, st, n_group, pick, group_chain, log.n_chain, n_cand, cand_first, tus,
                     rec_first, s);
  hipLaunchKernelGGL(log_scan_kernel, dim3(1), dim3(1024), 0, st, n_group, s, log);
  // enough workgroups for the rows and for the coefficients the log has room for; both loops stride over the grid
  const uint64_t chunks = (log.coeff_cap * (uint64_t)coeff_bytes + 4095u) / 4096u + 1u;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(rows, chunks), kCopyGridMax);
  if (coeff_bytes == 2)
    hipLaunchKernelGGL(log_copy_kernel<int16_t>, dim3(grid), dim3(256), 0, st, n_group, tus, static_cast<const int16_t *>(coeff), records,
                       tu_at, s, log);
  else
    hipLaunchKernelGGL(log_copy_kernel<int32_t>, dim3(grid), dim3(256), 0, st, n_group, tus, static_cast<const int32_t *>(coeff), records,
                       tu_at, s, log);
  return hipGetLastError();
}

hipError_t launch_search_log_place(hipStream_t st, const SearchLogArrays &log, const cabac_substream_desc *desc, uint32_t n_entry,
                                   uint64_t n_record, uint32_t n_tu, cabac_substream_desc *desc_out, uint32_t *splice_first,
                                   uint16_t *records, cabac_splice *splices) {
  if (n_tu) {  // a splice nobody fills names no block: the pipeline refuses the list
    hipError_t e = hipMemsetAsync(splices, 0xff, sizeof(cabac_splice) * (size_t)n_tu, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(log_place_scan_kernel, dim3(1), dim3(1024), 0, st, log.n_chain, desc, log.chain_rec, log.chain_tu, (uint64_t)n_tu,
                     desc_out, splice_first);
  if (n_entry)
    hipLaunchKernelGGL(log_place_move_kernel, dim3((n_entry + kRows - 1u) / kRows), dim3(256), 0, st, n_entry, log, n_record, (uint64_t)n_tu,
                       desc_out, splice_first, records, splices);
  return hipGetLastError();
}

hipError_t launch_search_log_place_fixed(hipStream_t st, const SearchLogArrays &log, WsState *ws, const cabac_substream_desc *desc,
                                         cabac_substream_desc *desc_out, uint32_t *splice_first, uint16_t *records,
                                         cabac_splice *splices, cabac_tu_desc *tus_out) {
  hipLaunchKernelGGL(log_place_scan_fixed_kernel, dim3(1), dim3(1024), 0, st, log, ws, desc, desc_out, splice_first, splices);
  const uint32_t grid = std::max((log.entry_cap + kRows - 1u) / kRows, (log.tu_cap + 255u) / 256u);  // rows of entries; descriptors
  if (grid)
    hipLaunchKernelGGL(log_place_move_fixed_kernel, dim3(grid), dim3(256), 0, st, log, ws, desc_out, splice_first, records, splices, tus_out);
  return hipGetLastError();
}

}  // namespace cabac
