// The lane-parallel half of the v4 "quad" kernels (cabac_kernels_v4.hip, where the layout is described): the DPP and mask
// helpers, phase (a) of a 16-bin step (quad_resolve, quad_phase_a, quad_phase_fields), its LDS tables, and the context store of a
// row from Ctx::init or a context set.  Shared by the kernel files that walk bin records four substreams to a wave.
#ifndef CABAC_QUAD_H
#define CABAC_QUAD_H
#include <type_traits>

#include "cabac_device.h"
#include "cabac_kernels.h"

namespace cabac {

constexpr uint32_t kQuadSubs = 4;        // substreams (rows) per wave
constexpr uint32_t kQuadCtxStride = 380; // LDS words per row context store (379 + pad)

template <int I>
__device__ __forceinline__ uint32_t row_bcast(uint32_t v) {
  // lane I of every 16-lane row -> all lanes of that row (DPP_ROW_NEWBCAST0 = 0x150, gfx90a+)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + I, 0xf, 0xf, true);  // bound_ctrl: no old-value init
}

// lane I of every group of L lanes -> all lanes of that group: L = 16 the DPP row broadcast above, L = 4 a DPP quad
// permutation (quad_perm:[I,I,I,I])
template <int L, int I>
__device__ __forceinline__ uint32_t group_bcast(uint32_t v) {
  if constexpr (L == 64) {  // one substream per wave: a scalar — handed back in a vector register, so that the chain stays the
    uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)v, I);  // vector code of the other geometries (as scalar code it is longer)
    asm volatile("" : "+v"(r));
    return r;
  }
  else if constexpr (L == 16) return row_bcast<I>(v);
  else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, I | (I << 2) | (I << 4) | (I << 6), 0xf, 0xf, true);
}

// Lanes (of `lanes`) that hold the same BITS-bit key as this lane.  One ballot per key bit; each lane keeps
// the lanes that agree with it on that bit: m &= ~(ballot ^ mybit), with the lane's bit spread to a 0 / ~0
// word so that the whole round is four vector instructions (bfe, cmp, 2 x bitop3) and no scalar one.
template <int BITS>
__device__ __forceinline__ uint64_t match_any_bits(uint32_t key, uint64_t lanes) {
  uint32_t mlo = (uint32_t)lanes, mhi = (uint32_t)(lanes >> 32);
#pragma unroll
  for (int b = 0; b < BITS; b++) {
    const uint32_t mine = (uint32_t)((int32_t)(key << (31 - b)) >> 31);
    const uint64_t bal = __ballot(mine != 0);
    mlo &= ~((uint32_t)bal ^ mine);
    mhi &= ~((uint32_t)(bal >> 32) ^ mine);
  }
  return ((uint64_t)mhi << 32) | mlo;
}

// 0 / ~0 from one bit of x
template <int BIT>
__device__ __forceinline__ uint32_t bit_mask(uint32_t x) {
  return (uint32_t)((int32_t)(x << (31 - BIT)) >> 31);
}
// (a & m) | (b & ~m)  — v_bfi_b32
__device__ __forceinline__ uint32_t sel(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }
__device__ __forceinline__ uint32_t neg_mask(uint32_t x) { return (uint32_t)((int32_t)x >> 31); }  // ~0 if bit 31 set

// sixteen consecutive LDS words into registers, four at a time (16-byte reads)
__device__ __forceinline__ void lds_read4(const uint32_t *p, int q, uint32_t (&dst)[16]) {
  const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
  dst[4 * q] = v.x;
  dst[4 * q + 1] = v.y;
  dst[4 * q + 2] = v.z;
  dst[4 * q + 3] = v.w;
}

// Phase (a) of one 16-bin step for the four rows: the context state each bin sees, resolved in parallel
// (see v3), the LDS context store brought up to date, and the bin's chain fields packed into one word:
//   bits 4..0 k | bits 8..5 2c | bit 9 LPS path | bit 10 bypass | bit 11 bypass bin 1 | bit 12 align
struct QuadRecord {  // one bin record of a 16-bin step, with the context state it sees
  uint32_t id, bin, st;
  uint32_t ctxm, epm, trmm, alnm;  // 0 / ~0: what kind of record it is (all zero: none — past the end of the substream)
  uint32_t kind;                   // quad_resolve<.., kKindTab>: the kind word of the id's table row, in place of epm, trmm, alnm
};

// Written with 0 / ~0 masks throughout (round 2): as booleans the record kinds became lane masks in SGPRs, and the
// s_and_b64 / s_and_saveexec that combined them each waited ~55 cycles for a vector compare — six to eight times per
// step in the context wave, which every encoder since v5 waits for.
constexpr uint32_t kMatchWords = 1024;  // per wave: which lanes of a row hold which record id, 16 bits per row and id, two rows per word
// `match` (optional, LDS, all zero between calls): the lanes of a row with the same id found through LDS instead of with nine
// ballots — every lane ORs its bit into the word of its id, reads the word back and clears it: three LDS instructions and
// one round trip instead of 36 vector instructions that write scalar registers (measured alone, tools/ubench_ctx.hip:
// the nine-round match-any is 160 of quad_phase_a's 350 ns)
// `rates` (kRateTab, LDS, 512 entries): the packed shift amounts and addends of the two estimators of every context, looked
// up instead of derived from the state word's rate bits with ten vector instructions (they depend on the context only:
// the fourth row of the init table; the estimator, which may start from given rates, derives them)
// `kinds` (kKindTab, LDS, kKindRows rows of 16 bytes, quad_kind_tab_init; it takes the place of `rates`): what a record id
// means, looked up with the rates in one 16-byte read instead of derived from the id with compares and masks for every bin
// — {rate shifts, rate addends, ctxm, kind word}.  An inactive lane reads the row behind the 512 ids, which is all zero
// ("nothing"), so nothing here asks again whether the lane is active; and the match bitmap has kMatchWordsCtx words per
// wave: a word per context and pair of rows, and one that every other record shares (only contexts use the answer).
constexpr uint32_t kKindNone = 512;             // the row of an inactive lane
constexpr uint32_t kKindRows = 513;
constexpr uint32_t kMatchWordsCtx = 768;        // 2 x (379 contexts + the shared word), rounded up
enum : uint32_t {                               // the kind word
  kKindC2Mask = 0x3ffu,                         // bits 9..0: 2 * constant term of the LPS width: 8 context, 4 terminate, 512 align, 0 otherwise
  kKindEpBit = 10,                              // a bypass bin
  kKindBadBit = 11,                             // no record id
  kKindLpsBit = 12,                             // context or terminate: a bin off the MPS (a terminate bin 1) takes the LPS path
  kKindAlignBit = 13,                           // align: the LPS path whatever the bin
  kKindLp9Shift = 16,                           // bits 24..16: 0x1ff for context, terminate and bypass — what such a bin may add to low
};
template <uint32_t kLowestSpecial = CABAC_REC_ALIGN, bool kLds = false, bool kRateTab = false, bool kKindTab = false>  // ids from kLowestSpecial up to 0x1FF are not "bad" (the estimator has two more)
__device__ __forceinline__ QuadRecord quad_resolve(uint32_t r, bool active, uint32_t lane, uint32_t row, uint32_t *rctx,
                                                   uint32_t &bad, uint32_t *match = nullptr, const uint2 *rates = nullptr,
                                                   const uint4 *kinds = nullptr) {
  static_assert(!kKindTab || (kLds && !kRateTab && kLowestSpecial == CABAC_REC_ALIGN), "the kind table: the encoder's ids, with the LDS match");
  QuadRecord q;
  uint32_t actm = active ? ~0u : 0u;
  if constexpr (!kKindTab) asm volatile("" : "+v"(actm));   // opaque: hipcc otherwise turns the mask arithmetic below back into lane-mask booleans
  const uint32_t id = kKindTab ? (active ? r & CABAC_REC_ID_MASK : kKindNone) : sel(actm, r & CABAC_REC_ID_MASK, CABAC_REC_ID_MASK);
  const uint32_t bin = (r >> 15) & 1u;
  uint4 kind = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (kKindTab) kind = kinds[id];
  const uint32_t ctxm = kKindTab ? kind.z : neg_mask(id - (uint32_t)kNumCtx);     // id < 379 (an inactive lane's id is 0x1FF)
  const uint32_t epm = actm & neg_mask((id ^ CABAC_REC_EP) - 1u);                 // (these three: not with kKindTab, where kind.w says it)
  const uint32_t trmm = actm & neg_mask((id ^ CABAC_REC_TRM) - 1u);
  const uint32_t alnm = actm & neg_mask((id ^ CABAC_REC_ALIGN) - 1u);
  if constexpr (kKindTab) bad |= kind.w & (1u << kKindBadBit);
  else bad |= actm & ~ctxm & neg_mask(id - kLowestSpecial) & 1u;
  const uint32_t j = lane & 15u;
  uint32_t same;
  if (kLds) {   // (a template parameter, not `match != nullptr`: an LDS address may be 0, so that test survives to run time)
    uint32_t *word = match + ((row >> 1) << 9) + id;
    if constexpr (kKindTab) word = match + (row >> 1) * (kMatchWordsCtx / 2u) + min(id, (uint32_t)kNumCtx);
    const uint32_t shift = ((row & 1u) << 4);
    atomicOr(word, 1u << (shift + j));
    asm volatile("" ::: "memory");                 // one wave: LDS executes its instructions in order
    same = (*word >> shift) & 0xffffu;             // (not through a volatile pointer: that becomes a system-scope flat load)
    asm volatile("" ::: "memory");
    *word = 0u;
  } else {
    same = (uint32_t)(match_any_bits<9>(id, 0xffffull << (16u * row)) >> (16u * row)) & 0xffffu;
  }
  const uint32_t binmask = (uint32_t)(__ballot(bin != 0) >> (16u * row)) & 0xffffu;  // the bins of this row
  const uint32_t before = same & ((1u << j) - 1u);      // earlier bins of the same context in this step
  const uint32_t lastm = neg_mask(((same >> j) ^ 1u) - 1u);  // no later one
  const uint32_t stored = rctx[min(id, (uint32_t)kNumCtx)];  // unconditional load (slot kNumCtx: the row's pad word)
  uint32_t st = stored & ctxm;
  // The state this bin sees is the stored one updated by those earlier bins, oldest first.  Their values are
  // known (encoder), so every lane walks its own `before` set — no hand-over between lanes, hence no LDS
  // round trip per repetition of a context.  update(), contexts.cpp:903-913, on both 15-bit estimators at
  // once with packed 16-bit math as in the decoder (the rates of a context never change).
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  u16x2 rate2, add2;
  if (kKindTab) {
    rate2 = __builtin_bit_cast(u16x2, kind.x);
    add2 = __builtin_bit_cast(u16x2, kind.y);
  } else if (kRateTab) {
    const uint2 ra = rates[id];
    rate2 = __builtin_bit_cast(u16x2, ra.x);
    add2 = __builtin_bit_cast(u16x2, ra.y);
  } else {
    const uint32_t r0 = (st & 3u) + 2u, r1 = ((st >> 2) & 7u) + 5u;
    rate2 = __builtin_bit_cast(u16x2, r0 | (r1 << 16));
    add2 = __builtin_bit_cast(u16x2, ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16));
  }
  const u16x2 mask2 = __builtin_bit_cast(u16x2, (kMask1 << 16) | kMask0);
  auto updated = [&](uint32_t s, uint32_t b) {
    const u16x2 s2 = __builtin_bit_cast(u16x2, s);
    const u16x2 b2 = __builtin_bit_cast(u16x2, b | (b << 16));
    return __builtin_bit_cast(uint32_t, (u16x2)(add2 * b2 + (s2 - ((s2 >> rate2) & mask2))));
  };
  uint32_t todo = before & ctxm;
  // How many repetitions the wave needs is asked right here (three ballots on todo with its lowest one / two bits
  // removed), long before the answers are branched on: a round is ten vector instructions for all lanes, and most
  // steps need none or one.
  const uint32_t after1 = todo & (todo - 1u), after2 = after1 & (after1 - 1u);
  uint64_t any1 = __ballot(todo != 0u), any2 = __ballot(after1 != 0u), more = __ballot(after2 != 0u);
  asm volatile("" : "+s"(any1), "+s"(any2), "+s"(more));
  auto one_round = [&]() {
    const uint32_t valid = (uint32_t)((int32_t)(0u - todo) >> 31);
    const uint32_t which = (uint32_t)__builtin_ctz(todo | 0x10000u);
    const uint32_t b = (binmask >> which) & 1u;
    st = sel(valid, updated(st, b), st);
    todo &= todo - 1u;
  };
  if (any1 != 0) {
    one_round();
    if (any2 != 0) {
      one_round();
      if (__builtin_expect(more != 0, 0)) {
        for (int round = 2; round < 16; round++) {
          one_round();
          if (__ballot(todo != 0) == 0) break;
        }
      }
    }
  }
  // others write the pad word (with kKindTab: min(id, kNumCtx) is the pad word already for all that is no context)
  if constexpr (kKindTab) rctx[((same >> j) & 0xffffu) == 1u ? min(id, (uint32_t)kNumCtx) : (uint32_t)kNumCtx] = updated(st, bin);
  else rctx[sel(ctxm & lastm, id, (uint32_t)kNumCtx)] = updated(st, bin);
  q.id = id;
  q.bin = bin;
  q.st = st;
  q.ctxm = ctxm;
  q.epm = epm;
  q.trmm = trmm;
  q.alnm = alnm;
  q.kind = kind.w;
  return q;
}

template <bool kLds = false>
__device__ __forceinline__ uint32_t quad_phase_a(uint32_t r, bool active, uint32_t lane, uint32_t row, uint32_t *rctx,
                                                 uint32_t &bad, uint32_t *match = nullptr, const uint2 *rates = nullptr) {
  const QuadRecord q = quad_resolve<CABAC_REC_ALIGN, kLds, kLds>(r, active, lane, row, rctx, bad, match, rates);
  const uint32_t bin = q.bin;
  const uint32_t q8 = ctx2_q8(q.st);
  const uint32_t mps = q8 >> 7;
  // inactive lanes: a no-op step (t = 0, no shift); the kinds exclude each other
  return ((ctx2_k(q8) | (8u << 5) | ((bin ^ mps) << 9)) & q.ctxm) |
         (((4u << 5) | (bin << 9)) & q.trmm) |          // terminate == LPS width 2 (arith_codec.cpp:460-478)
         (((1u << 10) | (bin << 11)) & q.epm) |
         ((1u << 12) & q.alnm);
}

// The same as separate words for the lane-serial encoder (v7), which parks them in LDS field by field: no packing here and
// no unpacking there.
struct QuadFields {
  uint32_t k, c2, lpsm, lp9, ep;
};
template <bool kLds = false, bool kKindTab = false>
__device__ __forceinline__ QuadFields quad_phase_fields(uint32_t r, bool active, uint32_t lane, uint32_t row, uint32_t *rctx,
                                                        uint32_t &bad, uint32_t *match = nullptr, const uint2 *rates = nullptr,
                                                        const uint4 *kinds = nullptr) {
  const QuadRecord q = quad_resolve<CABAC_REC_ALIGN, kLds, kLds && !kKindTab, kKindTab>(r, active, lane, row, rctx, bad, match, rates, kinds);
  const uint32_t sum = (q.st & kMask0) + (q.st >> 16);            // state(), contexts.cpp:939-950
  const uint32_t sx = (uint32_t)((int32_t)(sum << 16) >> 31);     // 0 / ~0: the MPS
  const uint32_t binm = 0u - q.bin;                               // 0 / ~0: the bin
  QuadFields f;
  if constexpr (kKindTab) {
    // the same fields from the kind word.  Only a context has a state (q.st is 0 otherwise, so sum and sx are): off_mps is
    // the bin itself for every other record, and k needs no mask
    const uint32_t off_mps = binm ^ sx;                           // 0 / ~0: the bin is not the MPS
    f.k = ((sum >> 10) ^ sx) & 31u;
    f.c2 = q.kind & kKindC2Mask;
    f.lpsm = (off_mps & bit_mask<kKindLpsBit>(q.kind)) | bit_mask<kKindAlignBit>(q.kind);
    f.lp9 = off_mps & (q.kind >> kKindLp9Shift);
    f.ep = (q.kind >> kKindEpBit) & 1u;
    return f;
  }
  f.k = ((sum >> 10) ^ sx) & 31u & q.ctxm;
  // terminate == LPS width 2 (arith_codec.cpp:460-478).  align() == an LPS of width 256 (k = 0, c2 = 512: t = 256, the
  // chain takes t, clz(256) - 23 = 0 shifts, range = 256) that adds nothing to low (lp9 = 0, ep = 0): the chain and the
  // low wave need no case of their own for it
  f.c2 = (8u & q.ctxm) | (4u & q.trmm) | (512u & q.alnm);
  const uint32_t lpsm = ((binm ^ sx) & q.ctxm) | (binm & q.trmm); // the LPS path: bin != MPS, or a terminate bin 1
  f.lp9 = (lpsm | (binm & q.epm)) & 0x1ffu;                       // the bin adds its MPS sub-range to low: LPS, or a bypass bin 1
  f.lpsm = lpsm | q.alnm;                                         // (after lp9: an align record's stays 0)
  f.ep = q.epm & 1u;
  return f;
}

// the table quad_resolve<.., kRateTab> reads: per record id {shift0 | shift1 << 16, add0 | add1 << 16} (0 for ids that are no context)
__device__ __forceinline__ void quad_rate_tab_init(uint2 *tab, uint32_t tid, uint32_t n_threads) {
  for (uint32_t id = tid; id < 512u; id += n_threads) {
    uint2 v = make_uint2(0u, 0u);
    if (id < (uint32_t)kNumCtx) {
      const uint32_t rates = ctx2_init(0, c_init_tables[id], c_init_tables[3 * kNumCtx + id]) & 31u;
      const uint32_t r0 = (rates & 3u) + 2u, r1 = ((rates >> 2) & 7u) + 5u;
      v.x = r0 | (r1 << 16);
      v.y = ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16);
    }
    tab[id] = v;
  }
}

// the table quad_resolve<.., kKindTab> reads: the same two rate words, the context mask and the kind word (above) per record
// id, and the all-zero row of an inactive lane behind them
__device__ __forceinline__ void quad_kind_tab_init(uint4 *tab, uint32_t tid, uint32_t n_threads) {
  for (uint32_t id = tid; id < kKindRows; id += n_threads) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (id < (uint32_t)kNumCtx) {
      const uint32_t rates = ctx2_init(0, c_init_tables[id], c_init_tables[3 * kNumCtx + id]) & 31u;
      const uint32_t r0 = (rates & 3u) + 2u, r1 = ((rates >> 2) & 7u) + 5u;
      v.x = r0 | (r1 << 16);
      v.y = ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16);
      v.z = ~0u;
      v.w = 8u | (1u << kKindLpsBit) | (0x1ffu << kKindLp9Shift);
    } else if (id == CABAC_REC_TRM) {
      v.w = 4u | (1u << kKindLpsBit) | (0x1ffu << kKindLp9Shift);
    } else if (id == CABAC_REC_EP) {
      v.w = (1u << kKindEpBit) | (0x1ffu << kKindLp9Shift);
    } else if (id == CABAC_REC_ALIGN) {
      v.w = 512u | (1u << kKindAlignBit);
    } else if (id < kKindNone) {
      v.w = 1u << kKindBadBit;
    }
    tab[id] = v;
  }
}

__device__ __forceinline__ void quad_ctx_init(uint32_t *rctx, int qp_in, uint32_t iid, uint32_t j) {
  const int qp = qp_in < 0 ? 0 : (qp_in > 63 ? 63 : qp_in);
  for (uint32_t k = j; k < (uint32_t)kNumCtx; k += 16)
    rctx[k] = ctx2_init(qp, c_init_tables[iid * kNumCtx + k], c_init_tables[3 * kNumCtx + k]);
}

// ---- context sets (cabac_hip_ctx_sets.h) ------------------------------------------------------------------------
// The codec kernels take the sets as a trailing parameter PACK: empty for the instantiations the plain entry points
// launch — the signature, the kernel arguments and the code are then the ones from before the sets — and one CtxSets for
// the sets calls.  Everything about sets is in the overloads below; the empty ones say "no set, never bad".
constexpr uint32_t kNoSet = 0xffffffffu;
struct QuadSetUse {
  uint32_t start, out;  // kNoSet: Ctx::init / nothing written
  bool bad;             // an index >= n_sets: the substream codes nothing (CABAC_RES_BAD_SET)
};
__device__ __forceinline__ QuadSetUse quad_set_use(uint32_t, bool) { return QuadSetUse{kNoSet, kNoSet, false}; }
__device__ __forceinline__ QuadSetUse quad_set_use(uint32_t sub, bool in_batch, const CtxSets &cs) {
  QuadSetUse u;
  u.start = (in_batch && cs.start_set != nullptr) ? cs.start_set[sub] : kNoSet;
  u.out = (in_batch && cs.out_set != nullptr) ? cs.out_set[sub] : kNoSet;
  u.bad = (u.start != kNoSet && u.start >= cs.n_sets) || (u.out != kNoSet && u.out >= cs.n_sets);  // once per substream
  return u;
}
// the row's context store from its start set, lanes j, j + L, ...: the loop of estimate_kernel.  kRates: with the window
// sizes in the low five bits (the encoders' packed word); the decoder keeps those bits zero
template <bool kRates>
__device__ __forceinline__ void quad_ctx_load(uint32_t *rctx, int qp_in, uint32_t iid, uint32_t j, uint32_t L, const QuadSetUse &u,
                                              const CtxSets &cs) {
  if (u.start == kNoSet || u.bad) {
    const int qp = qp_in < 0 ? 0 : (qp_in > 63 ? 63 : qp_in);
    for (uint32_t k = j; k < (uint32_t)kNumCtx; k += L) {
      const uint32_t packed = ctx2_init(qp, c_init_tables[iid * kNumCtx + k], c_init_tables[3 * kNumCtx + k]);
      rctx[k] = kRates ? packed : packed & ~31u;
    }
  } else {
    const uint64_t at = (uint64_t)u.start * (uint64_t)kNumCtx;
    for (uint32_t k = j; k < (uint32_t)kNumCtx; k += L) {
      const uint32_t st = cs.state[at + k];
      uint32_t w = (st & kMask0) | (st & 0xffff0000u);
      if (kRates) {
        const uint32_t rt = cs.rate[at + k];
        w |= (((rt >> 4) - 2u) & 3u) | ((((rt & 15u) - 5u) & 7u) << 2);
      }
      rctx[k] = w;
    }
  }
}
// the contexts the row has now as its out set: all 379 states, and as rates the window sizes of the context (the fourth row of
// the init table; every set this library writes holds them).  The caller has made the row's stores visible to its lanes.
__device__ __forceinline__ void quad_ctx_export(const uint32_t *, uint32_t, uint32_t, const QuadSetUse &) {}
__device__ __forceinline__ void quad_ctx_export(const uint32_t *rctx, uint32_t j, uint32_t L, const QuadSetUse &u, const CtxSets &cs) {
  if (u.out == kNoSet || u.bad) return;
  const uint64_t at = (uint64_t)u.out * (uint64_t)kNumCtx;
  for (uint32_t k = j; k < (uint32_t)kNumCtx; k += L) {
    const uint32_t r = ctx_init_rates(c_init_tables[3 * kNumCtx + k]);
    cs.out_state[at + k] = rctx[k] & ~31u;
    cs.out_rate[at + k] = (uint8_t)(16u * (r & 0xffu) + (r >> 8));  // m_rate
  }
}
// a substream with a bad set index: results[sub] = {0, CABAC_RES_BAD_SET}
__device__ __forceinline__ void quad_bad_set_result(cabac_substream_result *results, uint32_t sub, bool first_lane, const QuadSetUse &u) {
  if (u.bad && first_lane) {
    cabac_substream_result res;
    res.n_bits = 0u;
    res.flags = 0x40u;  // CABAC_RES_BAD_SET
    results[sub] = res;
  }
}

// ---- the coder state of the pieces calls (cabac_hip_pieces.h) -----------------------------------------------------
// The pieces calls instantiate the in-wave kernels with one CtxPieces in the trailing pack: the sets overloads above take its
// base, the functions below the coder state; the kernels call them under `if constexpr`, so that the other instantiations compile
// to the code they had.  A state is data from memory: quad_piece_use checks every condition
// the header lists before the kernel looks at any of its values.
template <class... Sets>
constexpr bool kQuadPieces = (std::is_base_of_v<CtxPieces, Sets> || ...);

struct QuadPieceUse {
  bool code;        // the row codes its records
  bool refuse;      // CABAC_RES_BAD_STATE: nothing is written but the result
  uint32_t sticky;  // the flags the state came with (and CABAC_RES_BAD_SET of this piece): not zero — the state is copied
  // encode: low, range, pend, buf, nbuf, pos.  decode: range, value, fresh (the value is the first 16 bits of the stream), bits
  uint32_t low, range, pend, buf, nbuf, pos, value, fresh, bits;
};
template <bool kEnc>
__device__ __forceinline__ QuadPieceUse quad_piece_use(uint32_t sub, bool in_batch, bool bad_set, uint32_t cap, const CtxPieces &cp) {
  QuadPieceUse u{};
  u.range = 510u;  // start(), arith_codec.cpp:329-337 / :60-66
  u.fresh = 1u;
  uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (in_batch && cp.coder_in != nullptr) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(cp.coder_in + sub);
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = p[k];
  }
  const uint32_t kind = w[0];
  u.refuse = in_batch && !bad_set && kind != CABAC_CODER_FRESH && kind != (kEnc ? CABAC_CODER_ENC : CABAC_CODER_DEC);
  u.sticky = u.refuse ? 0u : (w[1] | (bad_set ? 0x40u : 0u));  // CABAC_RES_BAD_SET
  if (in_batch && !u.refuse && u.sticky == 0u && kind != CABAC_CODER_FRESH) {
    u.fresh = 0u;
    u.bits = w[2];
    if (kEnc) {
      u.low = w[4];
      u.range = w[5] & 0xffffu;
      u.pend = w[5] >> 16;
      u.buf = w[6];
      u.nbuf = w[7];
      u.pos = w[3];
      const uint64_t held = 8ull * u.pos + 16ull * u.nbuf + u.pend;          // what getNumWrittenBits() answers
      u.refuse = u.range < 256u || u.range > 510u || u.pend > 15u || u.low >= (1u << (10u + (u.pend & 15u))) || (u.pos & 1u) != 0u ||
                 held != (uint64_t)u.bits || (uint64_t)u.pos + 2ull * u.nbuf > (uint64_t)cap;
    } else {
      u.range = w[4];
      u.value = w[5];
      const uint32_t mark = w[6];  // 1: behind a terminate bin 1, where value may stand at or above the scaled range
      u.refuse = mark > 1u || u.range < 256u || u.range > 510u + mark || u.value >= ((u.range + 2u * mark) << 7);
    }
  }
  u.code = in_batch && !u.refuse && u.sticky == 0u;
  if (!u.code) {  // a refused state's values reach nothing: the row idles as a fresh, empty one
    u.low = u.pend = u.buf = u.nbuf = u.pos = u.value = u.bits = 0u;
    u.range = 510u;
    u.fresh = 1u;
  }
  return u;
}
// What a row that does not code leaves: {0, CABAC_RES_BAD_STATE} and nothing else, or {0, flags} and a copy of the state (read
// again here: in place it is this row's own, and nobody else writes it).  first_lane: lane 0 of a row inside the batch.
__device__ __forceinline__ void quad_piece_pass(cabac_substream_result *results, uint32_t sub, bool first_lane, const QuadPieceUse &u,
                                                const CtxPieces &cp) {
  if (!first_lane || u.code) return;
  cabac_substream_result res;
  res.n_bits = 0u;
  res.flags = u.refuse ? 0x80u : u.sticky;  // CABAC_RES_BAD_STATE
  results[sub] = res;
  if (u.refuse || cp.coder_out == nullptr) return;
  uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (cp.coder_in != nullptr) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(cp.coder_in + sub);
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = p[k];
  }
  w[1] = u.sticky;
  uint32_t *q = reinterpret_cast<uint32_t *>(cp.coder_out + sub);
#pragma unroll
  for (int k = 0; k < 8; k++) q[k] = w[k];
}
// the state behind a coded piece, from the row's first lane (plain vector stores)
__device__ __forceinline__ void quad_piece_store(const CtxPieces &cp, uint32_t sub, uint32_t kind, uint32_t flags, uint32_t bits,
                                                 uint32_t bytes_final, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  if (cp.coder_out == nullptr) return;
  uint32_t *q = reinterpret_cast<uint32_t *>(cp.coder_out + sub);
  q[0] = kind;
  q[1] = flags;
  q[2] = bits;
  q[3] = bytes_final;
  q[4] = p0;
  q[5] = p1;
  q[6] = p2;
  q[7] = p3;
}
template <class T, class... Rest>
__device__ __forceinline__ const T &quad_pack_first(const T &first, const Rest &...) { return first; }

// ---- probe points (cabac_hip_probe.h) ---------------------------------------------------------------------------
// A row's cursor into its list: the next probe, the end of the list, and the clipped position of that next probe in a register
// (0xffffffff: none left) — a step with no probe in it costs one compare against it.
struct QuadProbeCursor {
  uint32_t next, end, at;
  uint32_t ahead;  // per lane: the clipped position of probe next + j (0xffffffff behind the list), loaded a drain ahead
};
__device__ __forceinline__ uint32_t quad_probe_load(const ProbeList &pl, const QuadProbeCursor &pc, uint32_t n, uint32_t j) {
  const uint32_t p = pc.next + j;
  return p < pc.end ? min(pl.at[p], n) : 0xffffffffu;
}
__device__ __forceinline__ QuadProbeCursor quad_probe_begin(const ProbeList &pl, uint32_t sub, bool in_batch, uint32_t n, uint32_t lane) {
  QuadProbeCursor pc;
  pc.next = in_batch ? pl.first[sub] : 0u;
  pc.end = in_batch ? pl.first[sub + 1u] : 0u;
  pc.ahead = quad_probe_load(pl, pc, n, lane & 15u);
  pc.at = (uint32_t)__shfl((int)pc.ahead, (int)(lane & 48u));
  return pc;
}
__device__ __forceinline__ uint32_t quad_lane_get(uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)src); }
__device__ __forceinline__ uint64_t quad_lane_get(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src);
  return ((uint64_t)hi << 32) | lo;
}
// The row's probes at positions up to `upto`, the end of the step just walked (0: in front of the first step, where `mine` is 0).
// `mine` is the running total after this lane's own record of the step, so the total after the first pos records sits in lane
// (pos - 1) & 15 of the row.  Lane j takes probe next + j, whose position it holds already (`ahead`): each value comes over from
// the lane that holds it with a shuffle (no LDS traffic) and is stored from the lane that asked.  The next sixteen positions are
// then loaded for the drain to come, and the position of the next probe — what every step compares against — comes over from the
// lane that held it, so no step waits for that load.  The wave loops while a row had all sixteen taken: forty probes at one
// position are three trips.  A row with none to take passes through with nothing stored.  Positions that go backwards (the device
// forms do not see them) get the value of some lane of the row: unspecified, in bounds.
template <class T>
__device__ __forceinline__ void quad_probe_drain(const ProbeList &pl, QuadProbeCursor &pc, uint32_t n, uint32_t upto, T mine,
                                                 uint32_t lane, T *__restrict__ out) {
  const uint32_t row = lane >> 4, j = lane & 15u;
  for (;;) {
    const uint32_t pos = pc.ahead;
    T v = quad_lane_get(mine, (lane & 48u) | ((pos - 1u) & 15u));
    if (pos == 0u) v = 0;
    const uint32_t hits = (uint32_t)(__ballot(pos <= upto) >> (16u * row)) & 0xffffu;
    const uint32_t lead = (uint32_t)__builtin_ctz(~hits);  // the probes in front of the first one that is not due (at most 16)
    if (j < lead) out[pc.next + j] = v;
    pc.next += lead;
    pc.at = (uint32_t)__shfl((int)pos, (int)((lane & 48u) | (lead & 15u)));  // (a row with all sixteen taken comes round again)
    pc.ahead = quad_probe_load(pl, pc, n, j);
    if (__ballot(lead == 16u) == 0) break;
  }
}

}  // namespace cabac
#endif
