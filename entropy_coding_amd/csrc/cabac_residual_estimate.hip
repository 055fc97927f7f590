// Fused residual estimator: transform-block coefficients -> fractional bits, without bin records.
// What CABACWriter::residual_coding (cabac_writer.cpp:2424-2525) costs on a BitEstimator_Std (arith_codec.cpp:603-711)
// whose contexts were assigned from another coder's (contexts.hpp:254): the rate-distortion search's
//   getCABACEstimator()->residual_coding(tu, compID, cuCtx);  getEstFracBits()
// for a batch of candidates.  The result is DEFINED as the composition of the two existing device paths — the records
// cabac_hip_residual_device produces (cabac_residual.hip), costed by cabac_hip_estimate_from_device (estimate_kernel,
// cabac_kernels_v4.hip) — and computed without them: the walk below is the binariser's (same geometry, same carried
// budget of context-coded bins, same dependent-quantisation popcounts, same template reads), but where the binariser
// computes a write offset and stores a record, this kernel looks the bin's cost up and updates the context.
//
// Layout: one CANDIDATE (a run of blocks costed in order, contexts carried from block to block) per 16-lane DPP row,
// four per wave, sixteen per 256-thread workgroup; lane = scan position inside the coefficient group, one iteration per
// group in coding order.  Per row in LDS: the context store (380 words: 379 packed contexts + a pad word inactive lanes
// write to).  Per wave in LDS: 1024 match words (which lanes of a row hold which context, as quad_resolve's).
//
// Order.  The estimator has no low / range chain: the total is a plain sum, and the only ordered thing is each context's
// own state.  The reference codes pass 1 of a group position-major (sig, gt1, par, gt2 of position 15, then of 14, ...),
// but the four flags draw from disjoint context ranges (Ctx::SigFlag[ch, ch+2, ch+4], Ctx::ParFlag[ch], Ctx::GtxFlag[ch],
// Ctx::GtxFlag[ch+2]; context_modelling.cpp:41-45, context_modelling.hpp:71-244) — as do the last-position prefixes, the
// group flags, transform_skip_flag and the flags of the transform-skip walk among themselves — so a group is costed
// PLANE BY PLANE: the 16 sig bins in one step, then the gt1 / par / gt2 bins in another, each in position order per
// context.  Inside a plane a context repeats often; a lane takes the row's same-context mask and applies its
// predecessors' bins (which it knows from a ballot) to the state in registers — no hand-over between lanes.  gt1, par and
// gt2 of a position share the context offset, so one match serves all three and their predecessor walks run together.
// Bypass bins (escape code words, signs) add their length << 15.
//
// Reads 4 (2) B per coefficient plus template re-reads that hit L1 / L2, and the touched part of the start context set
// per candidate (L2); writes 8 B per candidate (+ 12 B per block when the per-block outputs are asked for).  No MFMA.
//
// The exporting variant (kExport, cabac_hip_search.h) is the same walk over a list of candidates, which at its end unpacks
// the row's context store into the set the candidate leaves (1.9 KB: 379 x 4 B states + 379 rate bytes): what a search
// round commits for the candidate it picked.  The estimator's own entry points instantiate the kernel without it.
//
// The variant with side records (kSide, cabac_hip_search_unit.h) costs a candidate that is a record string with blocks
// spliced in: in front of every block, and once more behind the last one, a row costs its own side records up to the
// block's position, 16 per step with lane = record — a context-coded record through the same plane step as a block's
// flags, a bypass bin 1 << 15, a terminate bin its constant, and an align record rounds the row's running total (blocks
// included) up to a whole bit, formed in order only in a step that holds one.  Any of the 379 contexts can be named, so
// this variant brings all of them in and exports all of them from the store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_device.h"
#include "cabac_hip.h"
#include "cabac_kernels.h"
#include "cabac_scan.h"

namespace cabac {

namespace {

constexpr uint32_t kEstRows = 16;          // candidates per workgroup (256 threads)
constexpr uint32_t kEstCtxStride = 380;    // 379 contexts + the pad word
constexpr uint32_t kEstMatchWords = 1024;  // per wave: 16 bits per row and context id, two rows per word
constexpr uint32_t kEstClasses = 16;       // candidates by log2 of their group count
// scratch layout (uint32): [0..15] candidates per class, [16..31] scatter cursors, [32 .. 32 + n) the order, [32 + n .. 32 + 2n) classes
constexpr uint32_t kEstHeader = 32;

__constant__ uint32_t c_est_frac_bits[512] = {CABAC_FRAC_BITS_TABLE_VALUES};

__device__ __forceinline__ uint64_t est_row_sum64(uint64_t v) {  // sum over the 16 lanes of a row, in every lane
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

struct EstExport {        // what the exporting variant of the kernel needs on top (all null / unused otherwise)
  const uint32_t *index;    // item -> candidate (null: the identity)
  const uint32_t *out_set;  // per item: the set to write, 0xffffffff = none
  uint32_t *out_state;
  uint8_t *out_rate;
};

struct EstSide {           // what the variant with side records needs on top (unused otherwise)
  const uint64_t *rec_first;  // candidate -> its run of side records (n_cand + 1 entries)
  const uint16_t *records;
  const uint32_t *tu_at;      // block -> the index in its candidate's run it is inserted in front of (null: behind the run)
  uint32_t *flags;            // per candidate: CABAC_RES_BAD_RECORD or 0 (may be null)
};

struct EstRow {          // what a plane step needs of its row
  uint32_t *ctx;         // the row's context store (LDS)
  uint32_t *match;       // the row pair's match words (LDS)
  const uint32_t *frac;  // m_binFracBits (LDS)
  uint32_t l, row_shift, match_shift;
};

// update(bin) on the packed word (ctx2_update) with the shifts and the addend of the context derived once
struct EstRates {
  uint32_t r0, r1, add;
  __device__ __forceinline__ explicit EstRates(uint32_t st) {
    r0 = (st & 3u) + 2u;
    r1 = ((st >> 2) & 7u) + 5u;
    add = ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16);
  }
  __device__ __forceinline__ uint32_t update(uint32_t st, uint32_t bin) const {
    const uint32_t d = (((st & kMask0) >> r0) & kMask0) | ((((st >> 16) >> r1) & kMask1) << 16);
    return st - d + (bin ? add : 0u);
  }
};

// the lanes of the row that are `on` with the same id (this lane included); 0 for a lane that is off
__device__ __forceinline__ uint32_t est_match(const EstRow &r, bool on, uint32_t id) {
  uint32_t *word = r.match + (on ? id : (uint32_t)kNumCtx);
  atomicOr(word, 1u << (r.match_shift + r.l));
  asm volatile("" ::: "memory");  // one wave: LDS executes its instructions in order
  const uint32_t same = (*word >> r.match_shift) & 0xffffu;
  asm volatile("" ::: "memory");
  *word = 0u;
  return on ? same : 0u;
}

// the lanes of `same` coded before lane l / whether none is coded after it
template <bool kDown>
__device__ __forceinline__ uint32_t est_before(uint32_t same, uint32_t l) {
  return kDown ? same & (0xfffeu << l) & 0xffffu : same & ((1u << l) - 1u);
}
template <bool kDown>
__device__ __forceinline__ bool est_is_last(uint32_t same, uint32_t l) {
  return kDown ? (same & ((1u << l) - 1u)) == 0u : (same >> (l + 1u)) == 0u;
}
template <bool kDown>
__device__ __forceinline__ uint32_t est_oldest(uint32_t todo) {
  return kDown ? 31u - (uint32_t)__builtin_clz(todo) : (uint32_t)__builtin_ctz(todo);
}

// One plane: up to 16 context-coded bins of a row, one per lane, in coding order (kDown: lane 15 first — the regular walk's
// reverse scan; else lane 0 first).  Returns the lane's cost (estFracBitsUpdate, contexts.cpp:922-925) and leaves the
// contexts updated.  Called by all lanes of the wave together.
template <bool kDown>
__device__ __forceinline__ uint32_t est_plane(const EstRow &r, bool on, uint32_t id, uint32_t bin) {
  const uint32_t same = est_match(r, on, id);
  const uint32_t bins = row_bits(on && bin != 0u, r.row_shift);
  const uint32_t slot = on ? id : (uint32_t)kNumCtx;
  uint32_t st = r.ctx[slot];
  const EstRates rt(st);
  uint32_t todo = est_before<kDown>(same, r.l);
  while (__ballot(todo != 0u) != 0ull) {
    if (todo != 0u) {
      const uint32_t which = est_oldest<kDown>(todo);
      st = rt.update(st, (bins >> which) & 1u);
      todo &= ~(1u << which);
    }
  }
  const uint32_t cost = on ? r.frac[2u * ctx2_q8(st) + bin] : 0u;
  if (on && est_is_last<kDown>(same, r.l)) r.ctx[id] = rt.update(st, bin);
  return cost;
}

// The greater-than-1, parity and greater-than-2 flags of a group (cabac_writer.cpp:2789-2803) in one step: the three
// contexts of a position are base + aofs with the same aofs, a position with a gt1 bin 1 has the other two, so the lanes
// sharing the parity / gt2 context are those sharing the gt1 context that have |level| > 1.
__device__ __forceinline__ uint32_t est_gtx_planes(const EstRow &r, bool on, uint32_t aofs, uint32_t gt1_base, uint32_t par_base,
                                                   uint32_t gt2_base, uint32_t a) {
  const bool big = on && a > 1u;
  const uint32_t par_bin = (a - 2u) & 1u, gt2_bin = (a - 2u) >> 1 ? 1u : 0u;
  const uint32_t same = est_match(r, on, gt1_base + aofs);
  const uint32_t m_big = row_bits(big, r.row_shift), m_par = row_bits(big && par_bin != 0u, r.row_shift),
                 m_gt2 = row_bits(big && gt2_bin != 0u, r.row_shift);
  const uint32_t slot = on ? aofs : 0u;
  uint32_t st1 = r.ctx[on ? gt1_base + aofs : (uint32_t)kNumCtx], stp = r.ctx[par_base + slot], st2 = r.ctx[gt2_base + slot];
  const EstRates rt1(st1), rtp(stp), rt2(st2);
  uint32_t todo = est_before<true>(same, r.l);
  while (__ballot(todo != 0u) != 0ull) {
    if (todo != 0u) {
      const uint32_t which = est_oldest<true>(todo);
      const uint32_t b1 = (m_big >> which) & 1u;
      st1 = rt1.update(st1, b1);
      if (b1) {
        stp = rtp.update(stp, (m_par >> which) & 1u);
        st2 = rt2.update(st2, (m_gt2 >> which) & 1u);
      }
      todo &= ~(1u << which);
    }
  }
  uint32_t cost = 0;
  if (on) {
    cost = r.frac[2u * ctx2_q8(st1) + (big ? 1u : 0u)];
    if (est_is_last<true>(same, r.l)) r.ctx[gt1_base + aofs] = rt1.update(st1, big ? 1u : 0u);
  }
  if (big) {
    cost += r.frac[2u * ctx2_q8(stp) + par_bin] + r.frac[2u * ctx2_q8(st2) + gt2_bin];
    if (est_is_last<true>(same & m_big, r.l)) {
      r.ctx[par_base + aofs] = rtp.update(stp, par_bin);
      r.ctx[gt2_base + aofs] = rt2.update(st2, gt2_bin);
    }
  }
  return cost;
}

// number of coefficient groups of a block's coded region (0 for a descriptor the kernel rejects)
__device__ __forceinline__ uint32_t est_groups(uint32_t lw, uint32_t lh) {
  if (lw > 6u || lh > 6u) return 0u;
  uint32_t cgw_l2, cgh_l2;
  group_shape(lw, lh, cgw_l2, cgh_l2);
  return 1u << (((lw < 5u ? lw : 5u) - cgw_l2) + ((lh < 5u ? lh : 5u) - cgh_l2));
}

// blocks [first, end) of candidate c, clipped to the n_tu = cand_first[n_cand] blocks there are; a run that goes backwards is empty
__device__ __forceinline__ void est_cand_range(const uint32_t *cand_first, uint32_t n_cand, uint32_t c, uint32_t &first, uint32_t &end) {
  const uint32_t n_tu = cand_first[n_cand];
  first = min(cand_first[c], n_tu);
  end = min(cand_first[c + 1u], n_tu);
  end = max(end, first);
}

// side records [first, first + n) of candidate c, clipped to the rec_first[n_cand] records there are as est_cand_range clips
// blocks; a run longer than 2^32 - 1 records (positions are uint32) is cut there
__device__ __forceinline__ void est_side_range(const uint64_t *rec_first, uint32_t n_cand, uint32_t c, uint64_t &first, uint32_t &n) {
  const uint64_t n_all = rec_first[n_cand];
  first = min(rec_first[c], n_all);
  const uint64_t end = max(min(rec_first[c + 1u], n_all), first);
  n = (uint32_t)min(end - first, (uint64_t)0xffffffffu);
}

}  // namespace

// Ordering pre-pass (the idea of class_hist / class_scatter, cabac_residual.hip): the rows of a wave run as long as the
// longest of them, so candidates are handed out by the log2 of their total group count, largest first.
// `index` (may be null): the pass orders the n_item candidates index[0 .. n_item) instead of candidates 0 .. n_cand - 1 (then
// n_item == n_cand); an entry that names no candidate (>= n_cand) has no blocks.  `rec_first` (may be null): the candidates' side
// records; a step of 16 of them weighs as much as a coefficient group.
__global__ __launch_bounds__(256) void est_class_hist(uint32_t n_item, uint32_t n_cand, const uint32_t *__restrict__ index,
                                                       const uint32_t *__restrict__ cand_first,
                                                       const cabac_tu_desc *__restrict__ tus, const uint64_t *__restrict__ rec_first,
                                                       uint32_t *__restrict__ scratch) {
  __shared__ uint32_t h[kEstClasses];
  if (threadIdx.x < kEstClasses) h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < n_item) {
    uint32_t first = 0, end = 0, groups = 0;
    const uint32_t cand = index ? index[c] : c;
    if (cand < n_cand) est_cand_range(cand_first, n_cand, cand, first, end);
    for (uint32_t t = first; t < end; t++) {
      const uint64_t hi = reinterpret_cast<const uint64_t *>(tus)[2u * (uint64_t)t + 1u];  // log2_width, log2_height: its low bytes
      groups += est_groups((uint32_t)hi & 0xffu, (uint32_t)(hi >> 8) & 0xffu);
    }
    if (rec_first && cand < n_cand) {
      uint64_t rec0;
      uint32_t n_rec;
      est_side_range(rec_first, n_cand, cand, rec0, n_rec);
      groups += (uint32_t)min(((uint64_t)n_rec + 15ull) >> 4, (uint64_t)(0xffffffffu - groups));
    }
    const uint32_t cls = groups ? min(32u - (uint32_t)__builtin_clz(groups), kEstClasses - 1u) : 0u;
    scratch[kEstHeader + n_item + c] = cls;
    atomicAdd(&h[cls], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kEstClasses && h[threadIdx.x]) atomicAdd(&scratch[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void est_class_scatter(uint32_t n_cand, uint32_t *__restrict__ scratch) {
  __shared__ uint32_t cnt[kEstClasses], start[kEstClasses];
  if (threadIdx.x < kEstClasses) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  uint32_t cls = 0, rank = 0;
  if (c < n_cand) {
    cls = scratch[kEstHeader + n_cand + c];
    rank = atomicAdd(&cnt[cls], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kEstClasses && cnt[threadIdx.x]) {
    uint32_t base = 0;
    for (uint32_t k = kEstClasses; k-- > threadIdx.x + 1u;) base += scratch[k];
    start[threadIdx.x] = base + atomicAdd(&scratch[kEstClasses + threadIdx.x], cnt[threadIdx.x]);
  }
  __syncthreads();
  if (c < n_cand) scratch[kEstHeader + start[cls] + rank] = c;
}

// kExport: the variant that also writes the context set a candidate leaves (cabac_hip_search.h).  It walks the n_item
// ITEMS of ex: item i is candidate ex.index[i] (i itself without an index; an entry >= n_cand is skipped) and writes its
// final contexts as set ex.out_set[i] of ex.out_state / ex.out_rate, which may be the start arrays: every read of the start
// set that feeds the walk happens before the __syncthreads() below, every store after the walk.  So the start arrays are not
// __restrict__ here.  Without kExport n_item == n_cand, ex is not read and the code is the one the estimator always ran.
// kSide (with kExport only): the candidates carry side records (sd, see the top of the file); ex.out_set may then be null (no
// set is written).  Without kSide sd is not read.
template <class C, bool kExport, bool kSide>
__global__ __launch_bounds__(256) void residual_estimate_kernel(uint32_t n_item, uint32_t n_cand, const uint32_t *__restrict__ cand_first,
                                                                 const cabac_tu_desc *__restrict__ tus, const C *__restrict__ coeff_all,
                                                                 const uint32_t *start_state, const uint8_t *start_rate,
                                                                 const uint32_t *__restrict__ start_set,
                                                                 const uint32_t *__restrict__ order, uint64_t *__restrict__ frac_bits,
                                                                 uint64_t *__restrict__ tu_frac_bits, uint32_t *__restrict__ tu_info,
                                                                 EstExport ex, EstSide sd) {
  static_assert(kExport || !kSide, "side records come with the exporting variant");
  __shared__ uint32_t ctx_all[kEstRows * kEstCtxStride];
  __shared__ uint32_t frac[512];
  __shared__ uint32_t match_all[4 * kEstMatchWords];
  const uint32_t lane = threadIdx.x & 63u, l = lane & 15u, row_shift = lane & 48u, wave = threadIdx.x >> 6, row = lane >> 4;
  for (uint32_t k = threadIdx.x; k < 4u * kEstMatchWords; k += 256u) match_all[k] = 0u;
  for (uint32_t k = threadIdx.x; k < 512u; k += 256u) frac[k] = c_est_frac_bits[k];

  const uint32_t slot = blockIdx.x * kEstRows + (threadIdx.x >> 4);
  const uint32_t item = slot < n_item ? order[slot] : 0xffffffffu;
  const uint32_t cand = (kExport && ex.index && item < n_item) ? ex.index[item] : item;
  const bool has_cand = item < n_item && cand < n_cand;
  uint32_t t = 0, t_end = 0;
  if (has_cand) est_cand_range(cand_first, n_cand, cand, t, t_end);

  EstRow r;
  r.ctx = ctx_all + (threadIdx.x >> 4) * kEstCtxStride;
  r.match = match_all + wave * kEstMatchWords + ((row >> 1) << 9);
  r.frac = frac;
  r.l = l;
  r.row_shift = row_shift;
  r.match_shift = (row & 1u) << 4;
  // Contexts assigned from another coder's (contexts.hpp:254): set start_set[cand], in the format of cabac_hip_ctx_init_device
  // (m_state[0] | m_state[1] << 16, m_rate = 16 * rate0 + rate1).  Only what residual coding can touch is brought in:
  // SigCoeffGroup .. LastY (86..291), TransformSkipFlag (310, 311) and the transform-skip residual sets (357..378).
  if (l == 0u) r.ctx[kNumCtx] = 0u;
  if (has_cand && (kExport || t < t_end)) {
    const uint64_t set = (uint64_t)start_set[cand] * (uint64_t)kNumCtx;
    auto bring = [&](uint32_t k) {
      const uint32_t st = start_state[set + k], rt = start_rate[set + k];
      r.ctx[k] = (st & kMask0) | (st & 0xffff0000u) | (((rt >> 4) - 2u) & 3u) | ((((rt & 15u) - 5u) & 7u) << 2);
    };
    if constexpr (kSide) {  // a side record can name any context
      for (uint32_t k = l; k < (uint32_t)kNumCtx; k += 16u) bring(k);
    } else {
      for (uint32_t k = 86u + l; k < 292u; k += 16u) bring(k);
      if (l < 2u) bring(310u + l);
      for (uint32_t k = 357u + l; k < (uint32_t)kNumCtx; k += 16u) bring(k);
    }
  }
  // the row's side records: rec[0 .. n_rec), costed up to rec_pos; rec_next holds lane l's record of the next step (rec_pos + l),
  // loaded a step ahead — across a block's walk too
  const uint16_t *rec = nullptr;
  uint32_t n_rec = 0, rec_pos = 0, rec_next = 0;
  uint64_t side_acc = 0;  // this lane's share of the side records' cost since the row's total was last formed
  bool side_bad = false;
  if constexpr (kSide) {
    if (has_cand) {
      uint64_t rec0;
      est_side_range(sd.rec_first, n_cand, cand, rec0, n_rec);
      rec = sd.records + rec0;
      if (l < n_rec) rec_next = rec[l];
    }
  }
  __syncthreads();

  uint64_t cand_total = 0;  // row-uniform
  while (__ballot(t < t_end || (kSide && rec_pos < n_rec)) != 0ull) {
    const bool blk = t < t_end;
    if constexpr (kSide) {
      // ---- the side records in front of this block (behind the last one: all that are left), 16 per step -----------
      uint32_t seg_end = n_rec;
      if (blk && sd.tu_at) seg_end = min(max(sd.tu_at[t], rec_pos), n_rec);
      while (__ballot(rec_pos < seg_end) != 0ull) {
        const uint32_t n_here = min(seg_end - rec_pos, 16u);
        const bool active = l < n_here;
        const uint32_t rr = rec_next;
        rec_pos += n_here;
        rec_next = (l < n_rec - rec_pos) ? rec[rec_pos + l] : 0u;
        const uint32_t id = rr & CABAC_REC_ID_MASK, bin = rr >> 15;
        uint32_t cost = est_plane<false>(r, active && id < (uint32_t)kNumCtx, id, bin);
        if (active && id == CABAC_REC_EP) cost = 1u << 15;                  // estFracBitsEP, contexts.cpp:880-882
        if (active && id == CABAC_REC_TRM) cost = bin ? 0x3bfbbu : 0x0010cu;  // estFracBitsTrm, contexts.cpp:931-933
        const bool aln = active && id == CABAC_REC_ALIGN;
        side_bad = side_bad || (active && id >= (uint32_t)kNumCtx && id < CABAC_REC_ALIGN);
        if (__builtin_expect(__ballot(aln) != 0ull, 0)) {  // align(), arith_codec.cpp:679-684: the total in order, as estimate_kernel
          uint64_t total = cand_total + est_row_sum64(side_acc);
          for (int k = 0; k < 16; k++) {
            total += (uint32_t)__shfl((int)cost, (int)(row * 16u + (uint32_t)k));
            if (__shfl((int)aln, (int)(row * 16u + (uint32_t)k))) total = (total + 0x7fffull) & ~0x7fffull;
          }
          cand_total = total;
          side_acc = 0;
        } else {
          side_acc += cost;
        }
      }
      if (__ballot(blk) == 0ull) continue;  // the iteration behind the last block of every row
    }
    bool live = blk;
    // ---- geometry (row-uniform), as residual_rows --------------------------------------------------
    uint32_t lw = 0, lh = 0, chroma = 0, flags = 0, max_log2 = 15;
    const C *coeff = coeff_all;
    if (live) {
      const cabac_tu_desc d = tus[t];
      lw = d.log2_width;
      lh = d.log2_height;
      chroma = d.channel;
      flags = d.flags;
      max_log2 = d.max_log2_tr_range ? d.max_log2_tr_range : 15u;
      coeff = coeff_all + d.coeff_offset;
    }
    const bool bad = live && (lw > 6u || lh > 6u || chroma > 1u || max_log2 > 20u ||
                              ((flags & CABAC_TU_TRANSFORM_SKIP) && (lw > 5u || lh > 5u)));  // TS blocks are at most 32 x 32
    if (bad) lw = lh = chroma = 0;
    live = live && !bad;
    const bool ts_blk = live && (flags & CABAC_TU_TRANSFORM_SKIP);
    const uint32_t w = 1u << lw, h = 1u << lh;
    uint32_t cgw_l2, cgh_l2;
    group_shape(lw, lh, cgw_l2, cgh_l2);
    const uint32_t cg_l2 = cgw_l2 + cgh_l2, cg_size = 1u << cg_l2;
    const uint32_t we = w < 32u ? w : 32u, he = h < 32u ? h : 32u;
    const uint32_t lwg = (31u - (uint32_t)__builtin_clz(we)) - cgw_l2, lhg = (31u - (uint32_t)__builtin_clz(he)) - cgh_l2;
    const uint32_t wg = 1u << lwg, hg = 1u << lhg, n_cg = live ? wg * hg : 0u;
    const uint32_t in_cg = c_diag.in_cg[cgw_l2][cgh_l2][l & (cg_size - 1u)];
    const uint32_t ix = in_cg & 15u, iy = in_cg >> 4;
    const uint8_t *grid = c_diag.grid[lwg][lhg];
    const bool lane_in_cg = l < cg_size;
    auto coef_at = [&](uint32_t x, uint32_t y) -> int32_t { return (int32_t)coeff[(y << lw) + x]; };  // within the coded region only

    // SBT / MTS zero-out (CABAC_TU_SBT_ZERO_OUT): a 32-wide (32-tall) luma block is coded as if only its left (upper) 16
    // columns (rows) existed
    const bool zo = live && !ts_blk && (flags & CABAC_TU_SBT_ZERO_OUT) && chroma == 0u && w <= 32u && h <= 32u;
    const uint32_t zo_w = (zo && w == 32u) ? 16u : we, zo_h = (zo && h == 32u) ? 16u : he;
    auto zeroed_out = [&](uint32_t gpos) { return (((gpos & 15u) << cgw_l2) >= zo_w) || (((gpos >> 4) << cgh_l2) >= zo_h); };

    // ---- sweep 1: which groups hold a coefficient, and the last significant position ----------------------
    int last = -1;
    uint64_t coded = 0;    // by scan index of the group
    uint64_t sig_map = 0;  // by raster position in the group grid: bit gy * wg + gx
    {
      int top = (int)n_cg - 1;
      top = max(top, __shfl_xor(top, 16));
      top = max(top, __shfl_xor(top, 32));
      top = __builtin_amdgcn_readfirstlane(top);
      for (int k = top; k >= 0; k--) {
        const bool on = k < (int)n_cg;
        int32_t c = 0;
        uint32_t gpos = 0;
        if (on) gpos = grid[k];
        const bool out_of_play = on && zeroed_out(gpos);
        if (on && !out_of_play && lane_in_cg) c = coef_at(((gpos & 15u) << cgw_l2) + ix, ((gpos >> 4) << cgh_l2) + iy);
        const uint32_t nz = row_bits(c != 0, row_shift);
        if (nz) {
          if (last < 0) last = (int)(((uint32_t)k << cg_l2) + (31u - (uint32_t)__builtin_clz(nz)));
          coded |= 1ull << k;
          sig_map |= 1ull << ((gpos >> 4) * wg + (gpos & 15u));
        }
      }
    }
    const bool empty = live && last < 0;
    live = live && !empty;
    uint32_t info = live ? (uint32_t)last : (bad ? CABAC_TU_INFO_BAD_DESC : empty ? CABAC_TU_INFO_EMPTY : 0u);
    const bool is_ts = ts_blk && live, is_reg = live && !ts_blk;
    uint64_t acc = 0;  // this lane's share of the block's cost

    // ---- transform_skip_flag (lane 15) and the prefix of the last position's x (lanes 0 ..), then of its y; the suffixes
    // are bypass bins (last_sig_coeff, cabac_writer.cpp:2639-2720) ----------------------------------------------------
    {
      uint32_t nx = 0, ny = 0, gix = 0, giy = 0, off_x = 0, off_y = 0, sh_x = 0, sh_y = 0;
      if (is_reg) {
        const uint32_t lcg = (uint32_t)last >> cg_l2;
        const uint32_t lgp = grid[lcg];
        const uint32_t lin = c_diag.in_cg[cgw_l2][cgh_l2][(uint32_t)last & (cg_size - 1u)];
        const uint32_t px = ((lgp & 15u) << cgw_l2) + (lin & 15u), py = ((lgp >> 4) << cgh_l2) + (lin >> 4);
        const uint32_t luma_off_x = lw < 3u ? 0u : lw == 3u ? 3u : lw == 4u ? 6u : lw == 5u ? 10u : 15u;
        const uint32_t luma_off_y = lh < 3u ? 0u : lh == 3u ? 3u : lh == 4u ? 6u : lh == 5u ? 10u : 15u;
        off_x = chroma ? 0u : luma_off_x;
        off_y = chroma ? 0u : luma_off_y;
        sh_x = chroma ? min(w >> 3, 2u) : (lw + 1u) >> 2;
        sh_y = chroma ? min(h >> 3, 2u) : (lh + 1u) >> 2;
        gix = group_idx(px);
        giy = group_idx(py);
        nx = gix + (gix < group_idx(zo_w - 1u) ? 1u : 0u);
        ny = giy + (giy < group_idx(zo_h - 1u) ? 1u : 0u);
        const uint32_t sx = gix > 3u ? (gix - 2u) >> 1 : 0u, sy = giy > 3u ? (giy - 2u) >> 1 : 0u;
        if (l == 0u) acc += (uint64_t)(sx + sy) << 15;
      }
      const bool ts_flag = live && (flags & CABAC_TU_TS_FLAG) && l == 15u;
      const bool on_x = l < nx;  // nx <= 10
      acc += est_plane<false>(r, on_x || ts_flag, ts_flag ? CABAC_CTX_TRANSFORM_SKIP_FLAG(chroma) : CABAC_CTX_LAST_X(chroma) + off_x + (l >> sh_x),
                              ts_flag ? (is_ts ? 1u : 0u) : (l < gix ? 1u : 0u));
      if (__ballot(l < ny) != 0ull) acc += est_plane<false>(r, l < ny, CABAC_CTX_LAST_Y(chroma) + off_y + (l >> sh_y), l < giy ? 1u : 0u);
    }

    // ---- sweep 2: the coefficient groups in coding order (residual_coding_subblock, cabac_writer.cpp:2722-2872) -----
    const bool dq = is_reg && (flags & CABAC_TU_DEP_QUANT);
    int budget = (int)((zo_w * zo_h * 28u) >> 4);  // cabac_writer.cpp:2485-2489 (the area after the zero-out)
    uint32_t state = 0;
    const int last_cg = live ? (last >> cg_l2) : -1;
    uint64_t todo = is_reg ? ((coded | 1ull) & ((2ull << last_cg) - 1ull)) : 0ull;  // the groups still to walk, by scan index
    int prev_cg = last_cg + 1;
    const uint32_t luma = chroma ^ 1u;
    const uint32_t gt1_base = 214u + 21u * chroma, par_base = 150u + 21u * chroma, gt2_base = 182u + 21u * chroma;  // GtxFlag(2 + ch), ParFlag(ch), GtxFlag(ch)

    while (__ballot(todo != 0ull) != 0ull) {
      const bool row_on = todo != 0ull;
      const int cg = row_on ? 63 - __builtin_clzll(todo) : 0;
      todo &= ~(1ull << cg);
      // coded_sub_block_flag (cabac_writer.cpp:2733-2743) of the empty groups passed over (bin 0; the zeroed-out ones among
      // them have none), then of this group (bin 1): one context set, in this order
      const uint32_t gap = row_on ? (uint32_t)(prev_cg - 1 - cg) : 0u;
      const bool own_flag = row_on && cg != last_cg && cg != 0;
      const uint32_t n_flags = gap + (own_flag ? 1u : 0u);
      for (uint32_t base = 0; __ballot(base < n_flags) != 0ull; base += 16u) {
        const uint32_t j = base + l;
        const bool in = j < n_flags, own = in && j == gap;
        const uint32_t sp = in ? grid[own ? cg : prev_cg - 1 - (int)j] : 0u;
        const bool keep = in && (own || !zeroed_out(sp));
        const uint32_t sx_ = sp & 15u, sy_ = sp >> 4, sb = sy_ * wg + sx_;
        const uint32_t right = sx_ + 1u < wg ? (uint32_t)(sig_map >> (sb + 1u)) & 1u : 0u;
        const uint32_t below = sy_ + 1u < hg ? (uint32_t)(sig_map >> (sb + wg)) & 1u : 0u;
        acc += est_plane<false>(r, keep, CABAC_CTX_SIG_COEFF_GROUP(chroma) + (right | below), own ? 1u : 0u);
      }
      prev_cg = row_on ? cg : prev_cg;
      const uint32_t gpos = row_on ? grid[cg] : 0u;
      const uint32_t gx = gpos & 15u, gy = gpos >> 4;
      const bool coded_group = (coded >> cg) & 1ull;
      if (row_on && chroma == 0u && coded_group && (gx > 3u || gy > 3u)) info |= CABAC_TU_INFO_MTS_VIOLATION;
      const int lo = cg << cg_l2;
      const int first = cg == last_cg ? last : lo + (int)cg_size - 1;
      const int infer = cg == last_cg ? last : (cg != 0 ? lo : -1);
      const int pos = lo + (int)l;
      const bool act = row_on && lane_in_cg && pos <= first;
      const uint32_t x = (gx << cgw_l2) + ix, y = (gy << cgh_l2) + iy, diag = x + y;

      int32_t c = 0;
      if (act) c = coef_at(x, y);
      const uint32_t a = (uint32_t)(c < 0 ? -c : c);
      const bool nzero = c != 0;
      const uint32_t m_nz = row_bits(nzero, row_shift);

      // template of the position (sigCtxIdAbs / templateAbsSum, context_modelling.hpp:71-117, :152-176): five neighbours to
      // the right and below, absent ones count as zero; loads from clamped addresses, an absent neighbour zeroed afterwards
      int sum_abs = 0, sum_clip = 0, n_tmpl = 0;
      if (act) {
        const bool x1 = x + 1u < we, x2 = x + 2u < we, y1 = y + 1u < he, y2 = y + 2u < he;
        const uint32_t xa = x + (x1 ? 1u : 0u), xb = x + (x2 ? 2u : 0u), ya = y + (y1 ? 1u : 0u), yb = y + (y2 ? 2u : 0u);
        const int32_t v0 = coef_at(xa, y), v1 = coef_at(xb, y), v2 = coef_at(xa, ya), v3 = coef_at(x, ya), v4 = coef_at(x, yb);
        auto add = [&](int32_t v, bool present) {
          int av = v < 0 ? -v : v;
          av = present ? av : 0;
          sum_abs += av;
          sum_clip += min(av, 4 + (av & 1));
          n_tmpl += av != 0;
        };
        add(v0, x1);
        add(v1, x2);
        add(v2, x1 && y1);
        add(v3, y1);
        add(v4, y2);
      }

      // which bins exist, and how far the context-bin budget reaches
      const uint32_t above_mask = ~0u << (l + 1u);  // positions coded before this one
      const bool sig_coded = act && !(pos == infer && (m_nz & above_mask) == 0u);
      const uint32_t m_sig = row_bits(sig_coded, row_shift);
      const uint32_t m_gt1 = row_bits(a > 1u, row_shift);
      const uint32_t spent_before = (uint32_t)__builtin_popcount(m_sig & above_mask) + (uint32_t)__builtin_popcount(m_nz & above_mask) +
                                    2u * (uint32_t)__builtin_popcount(m_gt1 & above_mask);
      const bool ctx_mode = act && (budget - (int)spent_before >= 4);
      const uint32_t m_ctx = row_bits(ctx_mode, row_shift);
      const uint32_t n_ctx_bins = (uint32_t)__builtin_popcount(m_sig & m_ctx) + (uint32_t)__builtin_popcount(m_nz & m_ctx) +
                                  2u * (uint32_t)__builtin_popcount(m_gt1 & m_ctx);

      // dependent-quantisation state on entry to each position: two masked popcounts of the group's parity bits (see
      // residual_rows)
      uint32_t my_state = 0;
      {
        const uint32_t m_par = row_bits(dq && act && (a & 1u), row_shift);
        const uint32_t top = (uint32_t)(first - lo), tt = top - l;
        const uint32_t s1 = state >> 1, s0 = state & 1u;
        const uint32_t e1 = (uint32_t)__builtin_popcount((m_par >> (l + 1u)) & 0x5555u) & 1u;
        const uint32_t e0 = (uint32_t)__builtin_popcount((m_par >> (l + 2u)) & 0x5555u) & 1u;
        my_state = ((e1 ^ ((tt & 1u) ? s0 : s1)) << 1) | (e0 ^ ((tt & 1u) ? s1 : s0));
        if (row_on) {  // state after the top + 1 steps of this group
          const uint32_t p1 = (uint32_t)__builtin_popcount(m_par & 0x5555u) & 1u, p0 = (uint32_t)__builtin_popcount(m_par & 0xAAAAu) & 1u;
          const uint32_t n = top + 1u;
          state = ((p1 ^ ((n & 1u) ? s0 : s1)) << 1) | (p0 ^ ((n & 1u) ? s1 : s0));
        }
        if (!dq) my_state = 0;
      }

      // pass 2 (remainder of a context-coded level) or pass 3 (whole level in bypass mode): one escape code per position
      uint32_t ep_value = 0, ep_rice = 0;
      bool has_ep = false;
      if (ctx_mode) {
        has_ep = a >= 4u;
        ep_value = (a - 4u) >> 1;
        ep_rice = rice_of(sum_abs, 4);
      } else if (act) {
        has_ep = true;
        ep_rice = rice_of(sum_abs, 0);
        const uint32_t pos0 = (my_state < 2u ? 1u : 2u) << ep_rice;
        ep_value = a == 0u ? pos0 : (a <= pos0 ? a - 1u : a);
      }
      uint32_t ep_bins = 0;
      if (has_ep) {
        const EpCode ep = rem_abs_code(ep_value, ep_rice, max_log2);
        ep_bins = ep.len1 + ep.len2;
      }
      // signs (cabac_writer.cpp:2860-2871): one bypass bin per non-zero level, the hidden one excepted
      bool sign = nzero;
      if (m_nz && (flags & CABAC_TU_SIGN_HIDING)) {
        const uint32_t hi_nz = 31u - (uint32_t)__builtin_clz(m_nz), lo_nz = (uint32_t)__builtin_ctz(m_nz);
        if (hi_nz - lo_nz >= 4u && l == lo_nz) sign = false;
      }
      acc += (uint64_t)(ep_bins + (sign ? 1u : 0u)) << 15;

      // the context-coded flags, plane by plane
      const uint32_t ofs = min((uint32_t)(sum_clip + 1) >> 1, 3u) + 4u * ((uint32_t)(diag < 2u) + (luma & (uint32_t)(diag < 5u)));
      const uint32_t set = chroma + 2u * (my_state - (my_state > 1u ? 1u : my_state));  // SigFlag[chType + 2 * max(0, state - 1)]
      const uint32_t sig_base = (uint32_t)(0x8E827A6E665Aull >> (8u * set)) & 0xffu;    // 90, 102, 110, 122, 130, 142
      // ctxOffsetAbs, context_modelling.hpp:131-143
      const uint32_t steps = (uint32_t)(diag == 0u) + luma * ((uint32_t)(diag < 3u) + (uint32_t)(diag < 10u));
      const uint32_t aofs = (pos != last ? 1u : 0u) * ((uint32_t)min(sum_clip - n_tmpl, 4) + 1u + 5u * steps);
      if (__ballot(ctx_mode && sig_coded) != 0ull) acc += est_plane<true>(r, ctx_mode && sig_coded, sig_base + ofs, nzero ? 1u : 0u);
      if (__ballot(ctx_mode && nzero) != 0ull) acc += est_gtx_planes(r, ctx_mode && nzero, aofs, gt1_base, par_base, gt2_base, a);
      if (row_on) budget -= (int)n_ctx_bins;
    }

    // ---- transform-skip blocks: residual_codingTS / residual_coding_subblockTS (cabac_writer.cpp:2874-3046) ----------
    // Forward scan order; sig, sign, greater-than-1 and parity of pass 1, the four greater-than flags of pass 2 and the
    // group flag draw from disjoint contexts, so each is a plane of its own
    if (__ballot(is_ts) != 0ull) {
      const bool bdpcm = (flags & CABAC_TU_BDPCM) != 0u;
      int tbudget = (int)((w * h * 7u) >> 2);
      uint32_t top = is_ts ? n_cg : 0u;
      top = max(top, (uint32_t)__shfl_xor((int)top, 16));
      top = max(top, (uint32_t)__shfl_xor((int)top, 32));
      top = (uint32_t)__builtin_amdgcn_readfirstlane((int)top);
      const uint32_t below_mask = (1u << l) - 1u;
      for (uint32_t cg = 0; cg < top; cg++) {
        const bool row_on = is_ts && cg < n_cg;
        const uint32_t gpos = row_on ? grid[cg] : 0u;
        const uint32_t gx = gpos & 15u, gy = gpos >> 4, gbit = gy * wg + gx;
        const bool coded_group = (coded >> cg) & 1ull;
        const bool others = (coded & ((1ull << cg) - 1ull)) != 0ull;  // a significant group before this one
        const bool has_flag = row_on && (cg != n_cg - 1u || others);  // cabac_writer.cpp:2933
        if (__ballot(has_flag) != 0ull) {
          const uint32_t left = gx > 0u ? (uint32_t)(sig_map >> (gbit - 1u)) & 1u : 0u;
          const uint32_t above = gy > 0u ? (uint32_t)(sig_map >> (gbit - wg)) & 1u : 0u;
          acc += est_plane<false>(r, has_flag && l == 0u, CABAC_CTX_TS_SIG_COEFF_GROUP + left + above, coded_group ? 1u : 0u);
        }
        const bool walk = row_on && (coded_group || !has_flag);
        if (__ballot(walk) == 0ull) continue;
        const bool act = walk && lane_in_cg;
        const uint32_t x = (gx << cgw_l2) + ix, y = (gy << cgh_l2) + iy;
        int32_t c = 0, vl = 0, va = 0;
        if (act) {
          c = coef_at(x, y);
          vl = coef_at(x > 0u ? x - 1u : x, y);
          va = coef_at(x, y > 0u ? y - 1u : y);
          vl = x > 0u ? vl : 0;
          va = y > 0u ? va : 0;
        }
        const uint32_t a = (uint32_t)(c < 0 ? -c : c);
        const bool nzero = c != 0;
        const uint32_t n_nb = (vl != 0 ? 1u : 0u) + (va != 0 ? 1u : 0u);
        uint32_t mod = a;  // deriveModCoeff, context_modelling.hpp:344-364
        if (!bdpcm && a != 0u) {
          const uint32_t pred = max((uint32_t)(vl < 0 ? -vl : vl), (uint32_t)(va < 0 ? -va : va));
          mod = a == pred ? 1u : (a < pred ? a + 1u : a);
        }
        // pass 1
        const uint32_t m_nz = row_bits(nzero, row_shift);
        const bool sig_coded = act && !(l == cg_size - 1u && (m_nz & below_mask) == 0u);
        const uint32_t m_sig = row_bits(sig_coded, row_shift);
        const uint32_t m_g1 = row_bits(nzero && mod > 1u, row_shift);
        const uint32_t spent1 = (uint32_t)__builtin_popcount(m_sig & below_mask) + 2u * (uint32_t)__builtin_popcount(m_nz & below_mask) +
                                (uint32_t)__builtin_popcount(m_g1 & below_mask);
        const bool pass1 = act && (tbudget - (int)spent1 >= 4);
        const uint32_t m_p1 = row_bits(pass1, row_shift);
        const uint32_t n1 = (uint32_t)__builtin_popcount(m_sig & m_p1) + 2u * (uint32_t)__builtin_popcount(m_nz & m_p1) +
                            (uint32_t)__builtin_popcount(m_g1 & m_p1);
        const int last1 = m_p1 ? 31 - __builtin_clz(m_p1) : -1;
        // pass 2
        const uint32_t cost2 = mod >= 2u ? min(4u, mod >> 1) : 0u;
        const uint32_t m_c0 = row_bits(act && (cost2 & 1u), row_shift), m_c1 = row_bits(act && (cost2 & 2u), row_shift),
                       m_c2 = row_bits(act && (cost2 & 4u), row_shift);
        const uint32_t spent2 = (uint32_t)__builtin_popcount(m_c0 & below_mask) + 2u * (uint32_t)__builtin_popcount(m_c1 & below_mask) +
                                4u * (uint32_t)__builtin_popcount(m_c2 & below_mask);
        const bool pass2 = act && (tbudget - (int)n1 - (int)spent2 >= 4);
        const uint32_t m_p2 = row_bits(pass2, row_shift);
        const uint32_t n2 = (uint32_t)__builtin_popcount(m_c0 & m_p2) + 2u * (uint32_t)__builtin_popcount(m_c1 & m_p2) +
                            4u * (uint32_t)__builtin_popcount(m_c2 & m_p2);
        const int last2 = m_p2 ? 31 - __builtin_clz(m_p2) : -1;
        // pass 3
        const uint32_t cut = (int)l <= last2 ? 10u : ((int)l <= last1 ? 2u : 0u);
        const uint32_t lvl = cut ? mod : a;
        const bool has_rem = act && lvl >= cut;
        const bool ep_sign = has_rem && lvl != 0u && (int)l > last1;
        uint32_t n3 = ep_sign ? 1u : 0u;
        if (has_rem) {
          const EpCode ep = rem_abs_code((int)l <= last1 ? (lvl - cut) >> 1 : lvl, 1u, max_log2);
          n3 += ep.len1 + ep.len2;
        }
        acc += (uint64_t)n3 << 15;

        const bool p1_nz = pass1 && nzero;
        if (__ballot(pass1 && sig_coded) != 0ull) acc += est_plane<false>(r, pass1 && sig_coded, CABAC_CTX_TS_SIG_FLAG + n_nb, nzero ? 1u : 0u);
        if (__ballot(p1_nz) != 0ull) {
          const int sl = (vl > 0) - (vl < 0), sa = (va > 0) - (va < 0);  // signCtxIdAbsTS, context_modelling.hpp:293-317
          uint32_t sctx = ((sl == 0 && sa == 0) || sl * sa < 0) ? 0u : (sl >= 0 && sa >= 0) ? 1u : 2u;
          sctx += bdpcm ? 3u : 0u;
          acc += est_plane<false>(r, p1_nz, CABAC_CTX_TS_RESIDUAL_SIGN + sctx, c < 0 ? 1u : 0u);
          acc += est_plane<false>(r, p1_nz, CABAC_CTX_TS_LRG1_FLAG + (bdpcm ? 3u : n_nb), mod > 1u ? 1u : 0u);
          if (__ballot(p1_nz && mod > 1u) != 0ull) acc += est_plane<false>(r, p1_nz && mod > 1u, CABAC_CTX_TS_PAR_FLAG, (mod - 2u) & 1u);
        }
        for (uint32_t k = 1; k <= 4u; k++)  // greater-than-(2k+1) flags, contexts TsGtxFlag(1..4)
          if (__ballot(pass2 && k <= cost2) != 0ull)
            acc += est_plane<false>(r, pass2 && k <= cost2, CABAC_CTX_TS_GTX_FLAG + k, mod >= 2u * k + 2u ? 1u : 0u);
        if (walk) tbudget -= (int)(n1 + n2);
      }
    }

    const uint64_t share = est_row_sum64(acc);
    if (blk && l == 0u) {
      if (tu_frac_bits) tu_frac_bits[t] = share;
      if (tu_info) tu_info[t] = info;
    }
    cand_total += blk ? share : 0ull;
    t += blk ? 1u : 0u;
  }
  if constexpr (kSide) {
    cand_total += est_row_sum64(side_acc);
    const bool bad_rec = row_bits(side_bad, row_shift) != 0u;
    if (bad_rec) cand_total = ~0ull;
    if (has_cand && l == 0u && sd.flags) sd.flags[cand] = bad_rec ? CABAC_RES_BAD_RECORD : 0u;
  }
  if (has_cand && l == 0u && (!kExport || frac_bits)) frac_bits[cand] = cand_total;

  // ---- the contexts the candidate leaves: the row's store unpacked into the format it was brought in from, and what
  // residual coding cannot touch copied from the start set (the row's own lanes wrote the store: one wave, LDS in order)
  if constexpr (kExport) {
    const uint32_t oset = (has_cand && (!kSide || ex.out_set)) ? ex.out_set[item] : 0xffffffffu;
    if (oset != 0xffffffffu) {
      const uint64_t src = (uint64_t)start_set[cand] * (uint64_t)kNumCtx, dst = (uint64_t)oset * (uint64_t)kNumCtx;
      for (uint32_t k = l; k < (uint32_t)kNumCtx; k += 16u) {
        const bool held = kSide || (k >= 86u && k < 292u) || k == 310u || k == 311u || k >= 357u;
        uint32_t st, rt;
        if (held) {
          const uint32_t w = r.ctx[k];
          st = w & (kMask0 | 0xffff0000u);
          rt = (((w & 3u) + 2u) << 4) | (((w >> 2) & 7u) + 5u);
        } else {
          st = start_state[src + k];
          rt = start_rate[src + k];
        }
        ex.out_state[dst + k] = st;
        ex.out_rate[dst + k] = (uint8_t)rt;
      }
    }
  }
}

size_t residual_estimate_scratch_bytes(uint32_t n_cand) { return sizeof(uint32_t) * (kEstHeader + 2u * (size_t)n_cand); }

namespace {

template <bool kExport, bool kSide = false>
hipError_t launch_estimate_items(hipStream_t st, uint32_t n_item, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                 const void *coeff, int coeff_bytes, const uint32_t *start_state, const uint8_t *start_rate,
                                 const uint32_t *start_set, uint64_t *frac_bits, uint64_t *tu_frac_bits, uint32_t *tu_info,
                                 void *scratch, const EstExport &ex, const EstSide &sd = EstSide{nullptr, nullptr, nullptr, nullptr}) {
  if (n_item == 0) return hipSuccess;
  if (coeff_bytes != 4 && coeff_bytes != 2) return hipErrorInvalidValue;
  uint32_t *s32 = static_cast<uint32_t *>(scratch);
  hipError_t e = hipMemsetAsync(s32, 0, sizeof(uint32_t) * kEstHeader, st);
  if (e != hipSuccess) return e;
  const dim3 sort_grid((n_item + 255u) / 256u), grid((n_item + kEstRows - 1u) / kEstRows);
  hipLaunchKernelGGL(est_class_hist, sort_grid, dim3(256), 0, st, n_item, n_cand, ex.index, cand_first, tus,
                     kSide ? sd.rec_first : nullptr, s32);
  hipLaunchKernelGGL(est_class_scatter, sort_grid, dim3(256), 0, st, n_item, s32);
  const uint32_t *order = s32 + kEstHeader;
  if (coeff_bytes == 2)
    hipLaunchKernelGGL((residual_estimate_kernel<int16_t, kExport, kSide>), grid, dim3(256), 0, st, n_item, n_cand, cand_first, tus,
                       static_cast<const int16_t *>(coeff), start_state, start_rate, start_set, order, frac_bits, tu_frac_bits, tu_info,
                       ex, sd);
  else
    hipLaunchKernelGGL((residual_estimate_kernel<int32_t, kExport, kSide>), grid, dim3(256), 0, st, n_item, n_cand, cand_first, tus,
                       static_cast<const int32_t *>(coeff), start_state, start_rate, start_set, order, frac_bits, tu_frac_bits, tu_info,
                       ex, sd);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_residual_estimate(hipStream_t st, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                    const void *coeff, int coeff_bytes, const uint32_t *start_state, const uint8_t *start_rate,
                                    const uint32_t *start_set, uint64_t *frac_bits, uint64_t *tu_frac_bits, uint32_t *tu_info,
                                    void *scratch) {
  return launch_estimate_items<false>(st, n_cand, n_cand, cand_first, tus, coeff, coeff_bytes, start_state, start_rate, start_set,
                                      frac_bits, tu_frac_bits, tu_info, scratch, EstExport{nullptr, nullptr, nullptr, nullptr});
}

hipError_t launch_residual_estimate_export(hipStream_t st, uint32_t n_item, const uint32_t *index, uint32_t n_cand,
                                           const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                           const uint32_t *start_state, const uint8_t *start_rate, const uint32_t *start_set,
                                           const uint32_t *out_set, uint32_t *out_state, uint8_t *out_rate, uint64_t *frac_bits,
                                           uint64_t *tu_frac_bits, uint32_t *tu_info, void *scratch) {
  return launch_estimate_items<true>(st, n_item, n_cand, cand_first, tus, coeff, coeff_bytes, start_state, start_rate, start_set,
                                     frac_bits, tu_frac_bits, tu_info, scratch, EstExport{index, out_set, out_state, out_rate});
}

hipError_t launch_unit_estimate(hipStream_t st, uint32_t n_item, const uint32_t *index, uint32_t n_cand, const uint32_t *cand_first,
                                const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, const uint32_t *start_state,
                                const uint8_t *start_rate, const uint32_t *start_set, const uint64_t *rec_first,
                                const uint16_t *records, const uint32_t *tu_at, const uint32_t *out_set, uint32_t *out_state,
                                uint8_t *out_rate, uint64_t *frac_bits, uint64_t *tu_frac_bits, uint32_t *tu_info, uint32_t *flags,
                                void *scratch) {
  return launch_estimate_items<true, true>(st, n_item, n_cand, cand_first, tus, coeff, coeff_bytes, start_state, start_rate, start_set,
                                           frac_bits, tu_frac_bits, tu_info, scratch, EstExport{index, out_set, out_state, out_rate},
                                           EstSide{rec_first, records, tu_at, flags});
}

}  // namespace cabac
