// Residual parser (decoder side): bytes -> transform-block coefficients, every context derived
// on the device from the coefficients decoded so far.  Restates
//   CABACReader::residual_coding             entropy_codec/cabac_reader.cpp:2647-2735
//   CABACReader::ts_flag                     cabac_reader.cpp:2737-2752
//   CABACReader::last_sig_coeff              cabac_reader.cpp:2865-2938
//   CABACReader::residual_coding_subblock    cabac_reader.cpp:2946-3128
//   CABACReader::residual_codingTS / residual_coding_subblockTS   cabac_reader.cpp:3130-3339
//   CoeffCodingContext                       common/context_modelling.hpp:71-244, :268-384, context_modelling.cpp:7-106
//   BinDecoderBase / TBinDecoder             entropy_codec/arith_codec.cpp:60-78, :100-197, :242-277
//
// The walk is serial by nature: the context of a bin is chosen from the values of the bins before it.  What can be had
// is a short instruction stream per bin and the other waves of the SIMD to fill its gaps, so: ONE substream per wave
// with uniform control flow (real scalar branches, no exec regions), four waves per workgroup dealt to the CU's four
// SIMDs, ~7 KB of LDS per wave (16 waves per CU).  Inside the wave the lanes hold what the serial walk keeps looking up:
//   * lane i of the first 16 lanes is scan position i of the current coefficient group: its level, its position in the
//     block, and the running five-sample template sums of its position (sum of |level|, the clipped sum, the count of
//     non-zero neighbours).  A decoded level is added to exactly the lanes whose template contains its position (one
//     masked add from a per-shape bit table), so the context of the next position is ONE v_readlane away instead of five
//     dependent LDS reads;
//   * the input is held 256 bytes at a time, one byte-swapped dword per lane, the next 256 bytes already loaded: the
//     arithmetic decoder's refill is a v_readlane, no memory access near the chain;
//   * signs, the sign-hiding parity rule and the write-out of a group are lane-parallel (ballots and popcounts).
// The arithmetic decoder keeps (value, look-ahead) in a 64-bit window as the quad decoder does (cabac_kernels_v4.hip):
// value in bits 62..47, refilled 16 bits at a time while fewer than 32 look-ahead bits are valid — a check per syntax
// element (a position's four flags shift at most 24 bits), not per bin.  Its arithmetic is branch-free vector code on
// wave-uniform values (the context state comes out of LDS, i.e. out of a VGPR); only the decoded bin crosses to the
// scalar side, once per bin.  Runs of bypass bins (Rice prefixes / suffixes, sign patterns, last-position suffixes) are
// decoded up to 15 at a time with one division: n bypass bins are the n-bit quotient of the value by the range
// (arith_codec.cpp:100-151 decodes them one by one and eight at a time, to the same effect).
//
// Algorithmic bytes: B_in read, 4 B per coded coefficient written, 16 B per block descriptor: HBM traffic is a few
// percent of the roof; the limit is the serial chain (instruction issue), as for the bin decoder.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "cabac_device.h"
#include "cabac_hip.h"
#include "cabac_hip_parse_elements.h"
#include "cabac_hip_parse_plan.h"
#include "cabac_kernels.h"
#include "cabac_quad.h"
#include "cabac_scan.h"

namespace cabac {

#ifdef CABAC_PARSE_PROFILE  // build with CABAC_EXTRA_FLAGS=-DCABAC_PARSE_PROFILE: where wave 0 of workgroup 0 spends its cycles
__device__ unsigned long long g_parse_prof[16];
__device__ unsigned long long g_parse_wave[3 * 8192];  // per substream: start, end (memtime), HW_ID | XCC_ID << 32
#define PP_TICK(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define PP_ADD(slot, t0, t1) \
  if (blockIdx.x == 0 && threadIdx.x == 0) g_parse_prof[slot] += (t1) - (t0)
#else
#define PP_TICK(var)
#define PP_ADD(slot, t0, t1)
#endif

namespace {

// The parser only ever touches the residual-coding contexts: SigCoeffGroup .. LastY (ids 86..291), TransformSkipFlag
// (310, 311) and the transform-skip sets (357..378): 230 slots of 16 bytes {state, shifts, adds, -} per wave.
constexpr uint32_t kCtxSlots = 232;
constexpr uint32_t kBlkWords = 1024;   // coded region of a block, pitch = its coded width
__host__ __device__ constexpr uint32_t slot_of(uint32_t id) { return id < 292u ? id - 86u : id < 312u ? id - 310u + 206u : id - 357u + 208u; }
__device__ __forceinline__ uint32_t id_of_slot(uint32_t s) { return s < 206u ? s + 86u : s < 208u ? s - 206u + 310u : s - 208u + 357u; }
// D: the decoder type of the walk.  The side-walking instantiation (unit parse, below) keeps all 379 contexts and uses the id as
// the slot; either way a block's slots are compile-time arithmetic on the ids.
#define SL_A(id) (D::kIdSlots ? (id) : (id) - 86u)                    /* ids 86..291 */
#define SL_TS(id) (D::kIdSlots ? (id) : (id) - 357u + 208u)           /* ids 357..378 */
#define SL_TS_FLAG(ch) (D::kIdSlots ? 310u + (ch) : 206u + (ch))
constexpr uint32_t kSideCtxSlots = 380;  // the side walk's store: slot = ctxId, 0..378

// Per coefficient-group shape: which scan positions of the group lie in the five-sample template of each position
// (context_modelling.hpp:71-117: right, right+1, below-right, below, below+1), and for transform-skip blocks the
// in-group index of the left / upper neighbour (0xFF: outside the group).
struct ShapeLut {
  uint16_t in_template[5][5][16];  // bit q: position q's sample is in the template of this position
  uint8_t left[5][5][16], above[5][5][16];
};

constexpr ShapeLut make_shapes() {
  ShapeLut t{};
  for (int a = 0; a < 5; a++)
    for (int b = 0; a + b < 5; b++) {
      uint8_t pos[16] = {};
      fill_diag(pos, 1 << a, 1 << b);
      const int n = 1 << (a + b);
      for (int i = 0; i < n; i++) {
        const int x = pos[i] & 15, y = pos[i] >> 4;
        uint16_t m = 0;
        uint8_t l = 0xff, u = 0xff;
        for (int q = 0; q < n; q++) {
          const int dx = (pos[q] & 15) - x, dy = (pos[q] >> 4) - y;
          if ((dx == 1 && dy == 0) || (dx == 2 && dy == 0) || (dx == 1 && dy == 1) || (dx == 0 && dy == 1) || (dx == 0 && dy == 2))
            m = (uint16_t)(m | (1u << q));
          if (dx == -1 && dy == 0) l = (uint8_t)q;
          if (dx == 0 && dy == -1) u = (uint8_t)q;
        }
        t.in_template[a][b][i] = m;
        t.left[a][b][i] = l;
        t.above[a][b][i] = u;
      }
    }
  return t;
}

__constant__ ShapeLut c_shapes = make_shapes();

// the tables the walk indexes with lane-varying or data-dependent indices, copied to LDS once per workgroup
struct LdsTables {
  uint8_t grid[4][4][64];
  uint8_t in_cg[5][5][16];
  uint16_t in_template[5][5][16];
  uint8_t left[5][5][16], above[5][5][16];
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// ---------------------------------------------------------------------------------------------------------------
// arithmetic decoder

template <bool kS, bool kIds = false>
struct PDecT {
  // kS: this wave keeps the decoder on the SCALAR unit (see pd_bin); kIds: the context store is indexed by ctxId (SL_A)
  static constexpr bool kScalar = kS;
  static constexpr bool kIdSlots = kIds;
  uint32_t hi, lo;   // window (wave-uniform, kept in vector registers): value in bits 62..47
  uint32_t range;    //   "
  int32_t look;      //   "   valid look-ahead bits below bit 47
  uint32_t rp;       // scalar: byte offset of the next unread 16-bit unit
  uint32_t in_cur, in_nxt;  // per lane: dword `lane` of the 256-byte block that holds rp / of the block after it, byte-swapped
  const uint8_t *src_safe;
  uint32_t cap, last_dword, lane;
};

template <class D>
__device__ __forceinline__ uint32_t pd_load_block(const D &d, uint32_t blk) {
  const uint32_t off = blk * 256u + 4u * d.lane;
  const uint32_t w = *reinterpret_cast<const uint32_t *>(d.src_safe + min(off, d.last_dword));
  return off < d.cap ? __builtin_bswap32(w) : 0u;  // past the end of the substream the window is fed zeros
}

// Append 16-bit units while fewer than 32 look-ahead bits are valid (at most two: look >= 0 here).  Afterwards 32 bits
// can be consumed before the next check.
template <class D>
__device__ __forceinline__ void pd_check(D &d) {
  int32_t look = (int32_t)rfl((uint32_t)d.look);
  while (__builtin_expect(look < 32, 0)) {
    const uint32_t dw = rl(d.in_cur, (d.rp >> 2) & 63u);
    const uint32_t unit = (d.rp & 2u) ? (dw & 0xffffu) : (dw >> 16);
    const uint64_t add = (uint64_t)unit << (31 - look);
    d.hi |= (uint32_t)(add >> 32);
    d.lo |= (uint32_t)add;
    look += 16;
    d.rp += 2u;
    if ((d.rp & 255u) == 0u) {
      d.in_cur = d.in_nxt;
      d.in_nxt = pd_load_block(d, (d.rp >> 8) + 1u);
    }
  }
  d.look = look;
}

// decodeBin, arith_codec.cpp:242-277, with BinProbModel_Std::getLPS / update (contexts.cpp:903-913, :939-954).
// ctx[slot] = {s0 | s1 << 16 (rate bits cleared), shift0 | shift1 << 16, add0 | add1 << 16, -}.  Branch-free: the one
// data-dependent decision of the walk is taken on the returned bin.  The walk is bound by instruction issue, so this is
// written for count: 31 vector instructions, two LDS accesses and the one v_readfirstlane.
template <class D>
__device__ __forceinline__ uint32_t pd_bin(D &d, uint4 *ctx, uint32_t slot) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const uint4 e = ctx[slot];
  // A SIMD has a vector and a scalar pipe that run side by side — for DIFFERENT waves (tools/ubench_mix.hip: four waves of
  // vector code 7.9 ns per instruction and wave, four of scalar code 7.1, two and two 4.2).  The decision arithmetic of a bin
  // is the same ~20 instructions on wave-uniform values either way, so every other wave of a workgroup runs it on the
  // scalar pipe: the state word crosses over first (one v_readfirstlane) and hipcc, seeing uniform values, picks s_
  // instructions; the other waves keep it in vector registers and only the decoded bin crosses.
  const uint32_t st = D::kScalar ? rfl(e.x) : e.x;
  const uint32_t sum = (st & 0xffffu) + (st >> 16);
  const uint32_t sx = (uint32_t)((int32_t)(sum << 16) >> 31);  // 0 / ~0 from the MPS bit
  const uint32_t k = ((sum >> 10) ^ sx) & 31u;
  const uint32_t t = (__umul24(d.range >> 5, k) + 8u) >> 1;     // ((range >> 5) * k >> 1) + 4
  const uint32_t rm = d.range - t;
  uint32_t ev;                                                  // value - scaledRange
  if (D::kScalar) ev = d.hi - (rm << 22);
  else asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(ev) : "v"(rm), "v"(0xffc00000u), "v"(d.hi));  // rm * -2^22 + value: one instruction
  // renormalisation, one rule for both paths: the chosen sub-range shifted up to [256, 511] — LPS by getRenormBitsLPS =
  // clz(t) - 23; MPS by one bit iff rm < 256, which is clz(rm) - 23 because rm >= 128 (an LPS width is at most 15.5 / 32
  // of the range plus 4)
  uint32_t bin, x;
  if (D::kScalar) {
    const bool mps = (int32_t)ev < 0;
    bin = (mps ? sx : ~sx) & 1u;
    x = mps ? rm : t;
  } else {
    uint32_t ngem;  // ~0: value < scaledRange (MPS).  Through asm: as (int)ev >> 31 hipcc turns every use back into v_cmp + v_cndmask pairs
    asm("v_ashrrev_i32 %0, 31, %1" : "=v"(ngem) : "v"(ev));
    bin = ~(ngem ^ sx) & 1u;
    x = (rm & ngem) | (t & ~ngem);
  }
  const uint32_t nsh = (uint32_t)__builtin_clz(x) - 23u;
  d.hi = min(d.hi, ev);   // ev wraps above 2^31 exactly when value < scaledRange
  d.range = x << nsh;
  const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << nsh;
  d.hi = (uint32_t)(v >> 32);
  d.lo = (uint32_t)v;
  d.look -= (int32_t)nsh;
  // update(bin) on both 15-bit estimators at once (vector pipe in both kinds of wave: there is no packed scalar math)
  const u16x2 st2 = __builtin_bit_cast(u16x2, e.x);
  const u16x2 dlt2 = (st2 >> __builtin_bit_cast(u16x2, e.y)) & __builtin_bit_cast(u16x2, (kMask1 << 16) | kMask0);
  const uint32_t rest = __builtin_bit_cast(uint32_t, (u16x2)(st2 - dlt2));
  uint32_t upd;
  if (D::kScalar) asm("v_pk_mad_u16 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(upd) : "v"(e.z), "s"(bin), "v"(rest));
  else asm("v_pk_mad_u16 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(upd) : "v"(e.z), "v"(bin), "v"(rest));
  ctx[slot].x = upd;
  return D::kScalar ? bin : rfl(bin);
}

// decodeBinEP, arith_codec.cpp:100-114: the doubling of value is folded into the comparison (against scaledRange / 2)
template <class D>
__device__ __forceinline__ uint32_t pd_ep(D &d) {
  const uint32_t ev = d.hi - (d.range << 21);
  const uint32_t ngem = (uint32_t)((int32_t)ev >> 31);
  d.hi = (d.hi & ngem) | (ev & ~ngem);
  const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << 1;
  d.hi = (uint32_t)(v >> 32);
  d.lo = (uint32_t)v;
  d.look -= 1;
  return rfl(~ngem & 1u);
}

// The next n (1..15) bypass bins as one number, MSB first, WITHOUT consuming them: they are the quotient of the value
// extended by n stream bits by the scaled range (what n rounds of decodeBinEP compute bit by bit).  look >= n.
template <class D>
__device__ __forceinline__ uint32_t pd_ep_peek(const D &d, uint32_t n) {
  // value (16 bits) and n more bits, over 128 * range: floor(floor(V / 128) / range), V / 128 < 2^24 exactly a float
  const uint32_t a = d.hi >> (22u - n);
  const float fr = (float)d.range;
  uint32_t q = (uint32_t)((float)a * __builtin_amdgcn_rcpf(fr));
  int32_t r = (int32_t)(a - q * d.range);
  if (r < 0) q -= 1u;
  else if (r >= (int32_t)d.range) q += 1u;
  return rfl(q);
}

// consume k of the bins just peeked (bins = their values, MSB first)
template <class D>
__device__ __forceinline__ void pd_ep_take(D &d, uint32_t bins, uint32_t k) {
  const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << k;
  d.hi = (uint32_t)(v >> 32) - ((bins * d.range) << 22);
  d.lo = (uint32_t)v;
  d.look -= (int32_t)k;
}

// decodeBinsEP(n), n <= 32 (arith_codec.cpp:116-151)
template <class D>
__device__ __forceinline__ uint32_t pd_bins_ep(D &d, uint32_t n) {
  uint32_t out = 0;
  while (n != 0u) {
    const uint32_t k = n < 15u ? n : 15u;
    pd_check(d);
    const uint32_t b = pd_ep_peek(d, k);
    pd_ep_take(d, b, k);
    out = (out << k) | b;
    n -= k;
  }
  return out;
}

// decodeRemAbsEP with cutoff 5 (arith_codec.cpp:153-179): unary prefix of at most 32 - maxLog2 ones, then the suffix
template <class D>
__device__ __forceinline__ uint32_t pd_rem_abs(D &d, uint32_t rice, uint32_t max_log2) {
  const uint32_t cutoff = 5u, max_prefix = 32u - max_log2;
  uint32_t prefix = 0;
  for (;;) {
    pd_check(d);
    const uint32_t want = min(15u, max_prefix - prefix);
    if (want == 0u) break;
    const uint32_t b = pd_ep_peek(d, want);
    const uint32_t ones = (uint32_t)__builtin_clz(~(b << (32u - want)));  // leading ones of the `want` bins (want < 32)
    if (ones < want) {
      pd_ep_take(d, b >> (want - ones - 1u), ones + 1u);  // the ones and the terminating zero
      prefix += ones;
      break;
    }
    pd_ep_take(d, b, want);
    prefix += want;
  }
  uint32_t length = rice, offset;
  if (prefix < cutoff) {
    offset = prefix << rice;
  } else {
    offset = ((1u << (prefix - cutoff)) + cutoff - 1u) << rice;
    length += prefix == max_prefix ? max_log2 - rice : prefix - cutoff;
  }
  return offset + pd_bins_ep(d, length);
}

// ---- the element walk's code words (cabac_hip_parse_elements.h) -----------------------------------------------------------
// A run of bypass ones: up to max_ones bins are read while they are 1; a 0 in front of the limit is consumed with them.  Returns
// the ones (== max_ones: no 0 was read).  15 bins per look-ahead check, as the prefix of pd_rem_abs.
template <class D>
__device__ __forceinline__ uint32_t pd_ep_ones(D &d, uint32_t max_ones) {
  uint32_t n = 0;
  for (;;) {
    const uint32_t want = min(15u, max_ones - n);
    if (want == 0u) break;
    pd_check(d);
    const uint32_t b = pd_ep_peek(d, want);
    const uint32_t ones = (uint32_t)__builtin_clz(~(b << (32u - want)));  // leading ones of the `want` bins (want < 32)
    if (ones < want) {
      pd_ep_take(d, b >> (want - ones - 1u), ones + 1u);  // the ones and the terminating zero
      n += ones;
      break;
    }
    pd_ep_take(d, b, want);
    n += want;
  }
  return n;
}

// decodeRemAbsEP with the cutoff as a parameter (arith_codec.cpp:153-179); maxLog2 15..20, cutoff <= 32 - maxLog2, rice <= 14:
// the suffix is at most max(maxLog2, 14 + 16) = 30 bins
template <class D>
__device__ __forceinline__ uint32_t pd_rem_abs_cut(D &d, uint32_t rice, uint32_t cutoff, uint32_t max_log2) {
  const uint32_t max_prefix = 32u - max_log2;
  const uint32_t prefix = pd_ep_ones(d, max_prefix);
  uint32_t length = rice, offset;
  if (prefix < cutoff) {
    offset = prefix << rice;
  } else {
    offset = ((1u << (prefix - cutoff)) + cutoff - 1u) << rice;
    length += prefix == max_prefix ? max_log2 - rice : prefix - cutoff;
  }
  return offset + pd_bins_ep(d, length);
}

// decodeBinTrm, arith_codec.cpp:181-197: decoding goes on whatever the bin is
template <class D>
__device__ __forceinline__ uint32_t pd_trm(D &d) {
  const uint32_t range = rfl(d.range) - 2u;
  const uint32_t bin = rfl(d.hi) >= (range << 22) ? 1u : 0u;
  d.range = range;
  if (!bin && range < 256u) {
    const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << 1;
    d.hi = (uint32_t)(v >> 32);
    d.lo = (uint32_t)v;
    d.look -= 1;
    d.range = range << 1;
  }
  return bin;
}

// ---------------------------------------------------------------------------------------------------------------
struct BlockGeom {  // scalars of the block being parsed
  uint32_t lw, lh, chroma, fl, max_log2;
  uint32_t we, he, lwe;                       // coded region (rom.cpp:218-226) and its pitch
  uint32_t cgw_l2, cgh_l2, cg_l2, cg_size;    // coefficient group (g_log2SbbSize, rom.cpp:41-50)
  uint32_t lwg, lhg, wg, hg;                  // group grid
};

__device__ __forceinline__ void geom_init(BlockGeom &g, uint32_t lw, uint32_t lh) {
  g.lw = lw;
  g.lh = lh;
  const uint32_t w = 1u << lw, h = 1u << lh;
  g.we = w < 32u ? w : 32u;
  g.he = h < 32u ? h : 32u;
  g.lwe = lw < 5u ? lw : 5u;
  if (lw == 0u) { g.cgw_l2 = 0u; g.cgh_l2 = lh < 4u ? lh : 4u; }
  else if (lh == 0u) { g.cgw_l2 = lw < 4u ? lw : 4u; g.cgh_l2 = 0u; }
  else if (lw == 1u) { g.cgw_l2 = 1u; g.cgh_l2 = lh <= 2u ? 1u : 3u; }
  else if (lh == 1u) { g.cgh_l2 = 1u; g.cgw_l2 = lw <= 2u ? 1u : 3u; }
  else { g.cgw_l2 = 2u; g.cgh_l2 = 2u; }
  g.cg_l2 = g.cgw_l2 + g.cgh_l2;
  g.cg_size = 1u << g.cg_l2;
  g.lwg = g.lwe - g.cgw_l2;
  g.lhg = (lh < 5u ? lh : 5u) - g.cgh_l2;
  g.wg = 1u << g.lwg;
  g.hg = 1u << g.lhg;
}

// |value| of the block sample at (xx, yy), 0 outside the coded region
__device__ __forceinline__ uint32_t blk_abs(const int32_t *blk, const BlockGeom &g, uint32_t xx, uint32_t yy) {
  const bool in = xx < g.we && yy < g.he;
  const int32_t v = blk[in ? (yy << g.lwe) + xx : 0u];
  return in ? (uint32_t)(v < 0 ? -v : v) : 0u;
}
__device__ __forceinline__ int32_t blk_val(const int32_t *blk, const BlockGeom &g, int32_t xx, int32_t yy) {
  const bool in = xx >= 0 && yy >= 0;
  const int32_t v = blk[in ? ((uint32_t)yy << g.lwe) + (uint32_t)xx : 0u];
  return in ? v : 0;
}

// SigFlag context sets by (state > 1 ? state - 1 : 0) * 2 + chroma: 90, 102, 110, 122, 130, 142
__device__ __forceinline__ uint32_t sig_set_base(uint32_t set) { return (uint32_t)((0x8E827A6E665Aull >> (8u * set)) & 0xffu); }

// ---- regular residual coding: one block (after ts_flag) -----------------------------------------------------------
// kZo: the block is coded with the SBT / MTS zero-out.  A variant of its own, because its three extra scalars (the reduced
// extents and the flag) are live across the whole walk: compiled into the common walk they push it over the scalar register
// file and hipcc moves uniform values of the chain to vector registers (static count 1 842 -> 2 340 vector instructions,
// 5.91 -> 6.13 ms on the bench's tiles, none of which uses the zero-out).
template <class D, bool kZo>
__device__ __forceinline__ uint32_t parse_regular(D &d, uint4 *ctx, int32_t *blk, const LdsTables &tab, const BlockGeom &g,
                                                  uint32_t lane) {
  const uint32_t chroma = g.chroma, j = lane & 15u;
  PP_TICK(p0);
  // ---- last significant position (cabac_reader.cpp:2865-2938)
  const uint32_t luma_off_x = g.lw < 3u ? 0u : g.lw == 3u ? 3u : g.lw == 4u ? 6u : g.lw == 5u ? 10u : 15u;
  const uint32_t luma_off_y = g.lh < 3u ? 0u : g.lh == 3u ? 3u : g.lh == 4u ? 6u : g.lh == 5u ? 10u : 15u;
  const uint32_t off_x = chroma ? 0u : luma_off_x, off_y = chroma ? 0u : luma_off_y;
  const uint32_t sh_x = chroma ? min((1u << g.lw) >> 3, 2u) : (g.lw + 1u) >> 2, sh_y = chroma ? min((1u << g.lh) >> 3, 2u) : (g.lh + 1u) >> 2;
  // SBT / MTS zero-out (CABAC_TU_SBT_ZERO_OUT; cabac_reader.cpp:2880-2891, :2718-2727, unit.cpp:465-479)
  const uint32_t zo_w = (kZo && g.lw == 5u) ? 16u : g.we, zo_h = (kZo && g.lh == 5u) ? 16u : g.he;
  const uint32_t max_x = group_idx(zo_w - 1u), max_y = group_idx(zo_h - 1u);
  uint32_t px = 0, py = 0;
  for (; px < max_x; px++) {
    pd_check(d);
    if (!pd_bin(d, ctx, SL_A(CABAC_CTX_LAST_X(chroma)) + off_x + (px >> sh_x))) break;
  }
  for (; py < max_y; py++) {
    pd_check(d);
    if (!pd_bin(d, ctx, SL_A(CABAC_CTX_LAST_Y(chroma)) + off_y + (py >> sh_y))) break;
  }
  if (px > 3u) px = min_in_group(px) + pd_bins_ep(d, (px - 2u) >> 1);
  if (py > 3u) py = min_in_group(py) + pd_bins_ep(d, (py - 2u) >> 1);
  px = min(px, g.we - 1u);  // a corrupt stream must not lead outside the block
  py = min(py, g.he - 1u);
  // its scan position: the group and the place in the group, found by the lanes
  const uint32_t ip = tab.in_cg[g.cgw_l2][g.cgh_l2][j];
  const uint32_t ix = ip & 15u, iy = ip >> 4;
  const uint32_t gl = tab.grid[g.lwg][g.lhg][lane];
  const uint32_t want_g = (px >> g.cgw_l2) | ((py >> g.cgh_l2) << 4);
  const uint32_t want_i = (px & ((1u << g.cgw_l2) - 1u)) | ((py & ((1u << g.cgh_l2) - 1u)) << 4);
  const uint64_t mg = __ballot(gl == want_g && lane < g.wg * g.hg), mi = __ballot(ip == want_i && lane < g.cg_size);
  const uint32_t last_cg = mg ? (uint32_t)__builtin_ctzll(mg) : 0u, last_i = mi ? (uint32_t)__builtin_ctzll(mi) : 0u;
  uint32_t info = (last_cg << g.cg_l2) + last_i;

  const uint32_t in_tmpl = tab.in_template[g.cgw_l2][g.cgh_l2][j];
  // dependent-quantisation state (cabac_reader.cpp:2699-2700: table 32040): kept as sq = 8 * state, the bit offset of the
  // state's SigFlag context slot in a lane's packed word; the transition table holds the next sq for (state, parity)
  const uint64_t trans8 = (g.fl & CABAC_TU_DEP_QUANT) ? 0x0818180800101000ull : 0ull;  // byte [2 * state + parity] = 8 * next state: 0,2 | 2,0 | 1,3 | 3,1
  // SigFlag slots by state (sets: state 0, 1 -> 0; 2 -> 1; 3 -> 2; luma sets 0, 2, 4 / chroma 1, 3, 5), packed one byte each
  const uint32_t sb0 = SL_A(CABAC_CTX_SIG_FLAG(0)), sb1 = SL_A(CABAC_CTX_SIG_FLAG(1)), sb2 = SL_A(CABAC_CTX_SIG_FLAG(2)),
                 sb3 = SL_A(CABAC_CTX_SIG_FLAG(3)), sb4 = SL_A(CABAC_CTX_SIG_FLAG(4)), sb5 = SL_A(CABAC_CTX_SIG_FLAG(5));
  const uint32_t sig_bases = chroma ? (sb1 | sb1 << 8 | sb3 << 16 | sb5 << 24) : (sb0 | sb0 << 8 | sb2 << 16 | sb4 << 24);
  const uint32_t gt1_base = SL_A(CABAC_CTX_GTX_FLAG(2u + chroma)), par_base = SL_A(CABAC_CTX_PAR_FLAG(chroma)),
                 gt2_base = SL_A(CABAC_CTX_GTX_FLAG(chroma));
  uint32_t sq = 0;
  int32_t budget = (int32_t)((zo_w * zo_h * 28u) >> 4);
  uint64_t sig_map = 0;
  PP_TICK(p1);
  PP_ADD(1, p0, p1);
  const uint32_t pitch = 1u << g.lwe;
  for (int32_t cg = (int32_t)last_cg; cg >= 0; cg--) {
    PP_TICK(c0);
    const uint32_t gp = rl(gl, (uint32_t)cg), gx = gp & 15u, gy = gp >> 4, gbit = gy * g.wg + gx;
    if (kZo && ((gx << g.cgw_l2) >= zo_w || (gy << g.cgh_l2) >= zo_h)) continue;  // zeroed out: nothing is coded for this group
    bool sig = cg == (int32_t)last_cg || cg == 0;
    if (!sig) {  // coded_sub_block_flag (cabac_reader.cpp:2965-2975)
      const uint32_t right = gx + 1u < g.wg ? (uint32_t)(sig_map >> (gbit + 1u)) & 1u : 0u;
      const uint32_t below = gy + 1u < g.hg ? (uint32_t)(sig_map >> (gbit + g.wg)) & 1u : 0u;
      pd_check(d);
      sig = pd_bin(d, ctx, SL_A(CABAC_CTX_SIG_COEFF_GROUP(chroma)) + (right | below)) != 0u;
    }
    PP_TICK(c1);
    PP_ADD(2, c0, c1);
    if (!sig) continue;
    sig_map |= 1ull << gbit;
    if (!chroma && (gx > 3u || gy > 3u)) info |= CABAC_TU_INFO_MTS_VIOLATION;  // cabac_reader.cpp:2729-2732
    // This lane's position and what its contexts need (context_modelling.hpp:71-143): the template over the groups
    // decoded before (samples of this group still read as zero) — sc the clipped sum, dd = sc minus the count of non-zero
    // neighbours, t_abs the plain sum — and the diagonal class offsets.
    const uint32_t x = (gx << g.cgw_l2) + ix, y = (gy << g.cgh_l2) + iy, diag = x + y;
    uint32_t t_abs, sc, dd, sig_cls, abs_cls1;
    {
      const uint32_t at = (y << g.lwe) + x;
      const bool x1 = x + 1u < g.we, x2 = x + 2u < g.we, y1 = y + 1u < g.he, y2 = y + 2u < g.he;
      auto mag = [&](bool in, uint32_t idx) {  // unconditional read from a clamped address: no exec region per sample
        const uint32_t m = in ? ~0u : 0u;
        const int32_t v = blk[idx & m];
        return (uint32_t)(v < 0 ? -v : v) & m;
      };
      const uint32_t a0 = mag(x1, at + 1u), a1 = mag(x2, at + 2u), a2 = mag(x1 && y1, at + pitch + 1u), a3 = mag(y1, at + pitch),
                     a4 = mag(y2, at + 2u * pitch);
      t_abs = a0 + a1 + a2 + a3 + a4;
      auto clip = [](uint32_t a) { return min(a, 4u + (a & 1u)); };
      sc = clip(a0) + clip(a1) + clip(a2) + clip(a3) + clip(a4);
      dd = sc - ((uint32_t)(a0 != 0u) + (uint32_t)(a1 != 0u) + (uint32_t)(a2 != 0u) + (uint32_t)(a3 != 0u) + (uint32_t)(a4 != 0u));
      sig_cls = diag < 2u ? 4u : 0u;
      if (!chroma) sig_cls += diag < 5u ? 4u : 0u;
      abs_cls1 = 1u;
      if (diag == 0u) abs_cls1 += chroma ? 5u : 15u;
      else if (!chroma) abs_cls1 += diag < 3u ? 10u : diag < 10u ? 5u : 0u;
    }
    // per lane, kept up to date by the lanes themselves: the SigFlag slot of this position for each state (one byte each)
    // and the offset of its gt1 / parity / gt2 contexts — the serial walk reads them with one v_readlane each
    auto sig_slots = [&]() {
      const uint32_t o = min((sc + 1u) >> 1, 3u) + sig_cls;
      return sig_bases + __builtin_amdgcn_perm(o, o, 0u);  // the offset in all four bytes
    };
    uint32_t sig4 = sig_slots(), aofs_v = min(dd, 4u) + abs_cls1;
    const bool is_last_cg = cg == (int32_t)last_cg;
    const int32_t first_i = is_last_cg ? (int32_t)last_i : (int32_t)g.cg_size - 1;
    uint32_t nz_mask = 0, g2_mask = 0, lev = 0;
    int32_t i = first_i;
    PP_TICK(c2);
    PP_ADD(3, c1, c2);
    // ---- pass 1: sig / gt1 / parity / gt2 while the budget of context-coded bins lasts (cabac_reader.cpp:3007-3063)
    // The first position of the group's walk is special (the last significant position of the block: significant by
    // definition, context offset 0) and so is its last (significance inferred when nothing before it was significant and
    // the group flag was coded): both are peeled off the loop's common path by `special`.
    // kInfer: the significance of this position is not coded if nothing before it in the group was significant
    // (:3011-3013); kLast: the block's last significant position — significant by definition, context offset 0.
    auto position = [&](auto infer, auto at_last) {
      pd_check(d);
      uint32_t sf = 1u;
      if (!(infer.value && nz_mask == 0u)) {
        sf = pd_bin(d, ctx, (rl(sig4, (uint32_t)i) >> sq) & 0xffu);
        budget--;
      }
      uint32_t par2 = 0;  // 2 * parity of the level
      if (sf) {
        const uint32_t aofs = at_last.value ? 0u : rl(aofs_v, (uint32_t)i);
        uint32_t level = 1u;
        budget--;
        if (pd_bin(d, ctx, gt1_base + aofs)) {
          const uint32_t par = pd_bin(d, ctx, par_base + aofs);
          const uint32_t g2 = pd_bin(d, ctx, gt2_base + aofs);
          budget -= 2;
          level = 2u + par + (g2 << 1);
          g2_mask |= g2 << i;
        }
        par2 = (level & 1u) << 1;
        nz_mask |= 1u << i;
        lev = j == (uint32_t)i ? level : lev;
        // into the templates that hold this position, and their context offsets again
        const uint32_t hit = 0u - ((in_tmpl >> i) & 1u);
        sc += hit & level;
        dd += hit & (level - 1u);
        t_abs += hit & level;
        sig4 = sig_slots();
        aofs_v = min(dd, 4u) + abs_cls1;
      }
      sq = (uint32_t)(trans8 >> (2u * sq + 4u * par2)) & 0xffu;
      i--;
    };
    typedef std::integral_constant<bool, true> yes_t;
    typedef std::integral_constant<bool, false> no_t;
    if (is_last_cg) {
      if (budget >= 4) position(yes_t(), yes_t());  // the last significant position itself
      while (i >= 0 && budget >= 4) position(no_t(), no_t());
    } else {
      const int32_t stop = cg != 0 ? 1 : 0;          // position 0 of a group other than the DC group may be inferred
      while (i >= stop && budget >= 4) position(no_t(), no_t());
      if (i == 0 && budget >= 4) position(yes_t(), no_t());
    }
    const int32_t bypass_i = i;  // positions bypass_i .. 0 are coded without contexts
    PP_TICK(c3);
    PP_ADD(4, c2, c3);
#ifdef CABAC_PARSE_PROFILE
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      g_parse_prof[10] += (unsigned)(first_i - i);                 // positions visited in pass 1
      g_parse_prof[11] += 1;                                       // coded groups
    }
#endif
    // ---- pass 2: remainders of the context-coded levels (:3065-3077)
    for (uint32_t m = g2_mask; m != 0u;) {
      const uint32_t q = 31u - (uint32_t)__builtin_clz(m);
      m &= ~(1u << q);
      const uint32_t rem2 = pd_rem_abs(d, rice_of((int)rl(t_abs, q), 4), g.max_log2) << 1;
      lev += j == q ? rem2 : 0u;
      t_abs += (0u - ((in_tmpl >> q) & 1u)) & rem2;
    }
    // ---- pass 3: whole levels in bypass mode (:3079-3098)
    for (int32_t q = bypass_i; q >= 0; q--) {
      const uint32_t rice = rice_of((int)rl(t_abs, (uint32_t)q), 0);
      const uint32_t pos0 = (sq < 16u ? 1u : 2u) << rice;
      const uint32_t rem = pd_rem_abs(d, rice, g.max_log2);
      const uint32_t v = rem == pos0 ? 0u : (rem < pos0 ? rem + 1u : rem);
      sq = (uint32_t)(trans8 >> (2u * sq + 8u * (v & 1u))) & 0xffu;
      if (v) {
        nz_mask |= 1u << q;
        lev = j == (uint32_t)q ? v : lev;
        t_abs += (0u - ((in_tmpl >> q) & 1u)) & v;
      }
    }
    PP_TICK(c4);
    PP_ADD(5, c3, c4);
    // ---- signs; with sign-data hiding the lowest position's sign is the parity of the level sum (:3100-3126)
    const uint32_t n_nz = (uint32_t)__builtin_popcount(nz_mask);
    const int32_t first_nz = nz_mask ? (int32_t)__builtin_ctz(nz_mask) : first_i;
    const int32_t last_nz = nz_mask ? 31 - (int32_t)__builtin_clz(nz_mask) : -1;
    const bool hide = (g.fl & CABAC_TU_SIGN_HIDING) && last_nz - first_nz >= 4;
    const uint32_t n_signs = hide ? n_nz - 1u : n_nz;
    const uint32_t pattern = pd_bins_ep(d, n_signs);
    {
      const bool mine = lane < g.cg_size && ((nz_mask >> j) & 1u);
      const uint32_t odd = (uint32_t)__builtin_popcountll(__ballot(mine && (lev & 1u))) & 1u;
      const uint32_t k = (uint32_t)__builtin_popcount(nz_mask >> (j + 1u));  // non-zero positions decoded before this one
      const uint32_t neg = k < n_signs ? (pattern >> (n_signs - 1u - k)) & 1u : odd;
      if (mine) blk[(y << g.lwe) + x] = neg ? -(int32_t)lev : (int32_t)lev;
    }
    PP_TICK(c5);
    PP_ADD(6, c4, c5);
  }
  return info;
}

// ---- transform-skip residual coding: one block (cabac_reader.cpp:3130-3339) ------------------------------------------
template <class D>
__device__ __forceinline__ void parse_ts(D &d, uint4 *ctx, int32_t *blk, const LdsTables &tab, const BlockGeom &g, uint32_t lane) {
  const uint32_t j = lane & 15u;
  const bool bdpcm = (g.fl & CABAC_TU_BDPCM) != 0u;
  const uint32_t ip = tab.in_cg[g.cgw_l2][g.cgh_l2][j];
  const uint32_t ix = ip & 15u, iy = ip >> 4;
  const uint32_t gl = tab.grid[g.lwg][g.lhg][lane];
  const uint32_t idx_l = tab.left[g.cgw_l2][g.cgh_l2][j], idx_a = tab.above[g.cgw_l2][g.cgh_l2][j];
  const uint32_t n_cg = g.wg * g.hg;
  int32_t budget = (int32_t)((g.we * g.he * 7u) >> 2);
  uint64_t sig_map = 0;
  for (uint32_t cg = 0; cg < n_cg; cg++) {
    const uint32_t gp = rl(gl, cg), gx = gp & 15u, gy = gp >> 4, gbit = gy * g.wg + gx;
    bool sig = cg == n_cg - 1u && sig_map == 0ull;
    if (!sig) {
      const uint32_t left = gx > 0u ? (uint32_t)(sig_map >> (gbit - 1u)) & 1u : 0u;
      const uint32_t above = gy > 0u ? (uint32_t)(sig_map >> (gbit - g.wg)) & 1u : 0u;
      pd_check(d);
      sig = pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_SIG_COEFF_GROUP) + left + above) != 0u;
    }
    if (!sig) continue;
    sig_map |= 1ull << gbit;
    // lane = forward scan position in the group; its left / upper samples as they stand (decoded groups: final values)
    const int32_t x = (int32_t)((gx << g.cgw_l2) + ix), y = (int32_t)((gy << g.cgh_l2) + iy);
    int32_t nb_l = blk_val(blk, g, x - 1, y), nb_a = blk_val(blk, g, x, y - 1), val = 0;
    uint32_t nz_mask = 0, sign_pattern = 0, n_nz = 0;
    int32_t last1 = -1, last2 = -1;
    const int32_t hi_i = (int32_t)g.cg_size - 1;
    auto put = [&](uint32_t i, int32_t v) {  // position i of the group becomes v: its own lane and the lanes beside / below it
      val = j == i ? v : val;
      nb_l = idx_l == i ? v : nb_l;
      nb_a = idx_a == i ? v : nb_a;
    };
    for (int32_t i = 0; i <= hi_i && budget >= 4; i++) {  // pass 1: sig, sign, greater-1, parity (:3222-3271)
      pd_check(d);
      const int32_t left = (int32_t)rl((uint32_t)nb_l, (uint32_t)i), above = (int32_t)rl((uint32_t)nb_a, (uint32_t)i);
      const uint32_t n_nb = (uint32_t)(left != 0) + (uint32_t)(above != 0);
      uint32_t sf = (n_nz == 0u && i == hi_i) ? 1u : 0u;
      if (!sf) {
        sf = pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_SIG_FLAG) + n_nb);
        budget--;
      }
      if (sf) {
        const int32_t sl = (left > 0) - (left < 0), sa = (above > 0) - (above < 0);
        uint32_t sctx = ((sl == 0 && sa == 0) || sl * sa < 0) ? 0u : (sl >= 0 && sa >= 0) ? 1u : 2u;
        if (bdpcm) sctx += 3u;
        const uint32_t sign = pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_RESIDUAL_SIGN) + sctx);
        const uint32_t g1 = pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_LRG1_FLAG) + (bdpcm ? 3u : n_nb));
        budget -= 2;
        uint32_t par = 0;
        if (g1) {
          par = pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_PAR_FLAG));
          budget--;
        }
        sign_pattern |= sign << n_nz;
        n_nz++;
        nz_mask |= 1u << i;
        const int32_t m = (int32_t)(1u + par + g1);
        put((uint32_t)i, sign ? -m : m);
      }
      last1 = i;
    }
    for (int32_t i = 0; i <= hi_i && budget >= 4; i++) {  // pass 2: greater-than-3/5/7/9 flags (:3276-3297)
      int32_t c = (int32_t)rl((uint32_t)val, (uint32_t)i);
      c = c < 0 ? -c : c;
      for (int32_t cut = 2; cut <= 8; cut += 2)
        if (c >= cut) {
          pd_check(d);
          c += (int32_t)(pd_bin(d, ctx, SL_TS(CABAC_CTX_TS_GTX_FLAG) + (uint32_t)(cut >> 1)) << 1);
          budget--;
        }
      put((uint32_t)i, c);
      last2 = i;
    }
    for (int32_t i = 0; i <= hi_i; i++) {  // pass 3: remainders, bypass levels with their signs, un-mapping (:3299-3329)
      int32_t c = (int32_t)rl((uint32_t)val, (uint32_t)i);
      c = c < 0 ? -c : c;
      const int32_t cut = i <= last2 ? 10 : i <= last1 ? 2 : 0;
      if (c >= cut) {
        const int32_t rem = (int32_t)pd_rem_abs(d, 1u, g.max_log2);
        c += i <= last1 ? rem << 1 : rem;
        if (c != 0 && i > last1) {
          pd_check(d);
          sign_pattern |= pd_ep(d) << n_nz;
          n_nz++;
          nz_mask |= 1u << i;
        }
      }
      if (!bdpcm && cut != 0 && c > 0) {  // decDeriveModCoeff, context_modelling.hpp:367-384
        int32_t left = (int32_t)rl((uint32_t)nb_l, (uint32_t)i), above = (int32_t)rl((uint32_t)nb_a, (uint32_t)i);
        left = left < 0 ? -left : left;
        above = above < 0 ? -above : above;
        const int32_t pred = left > above ? left : above;
        c = (c == 1 && pred > 0) ? pred : c - (c <= pred ? 1 : 0);
      }
      put((uint32_t)i, c);
    }
    {  // signs in the order the positions became non-zero: ascending scan position
      const bool mine = lane < g.cg_size && ((nz_mask >> j) & 1u);
      const uint32_t k = (uint32_t)__builtin_popcount(nz_mask & ((1u << j) - 1u));
      const bool neg = ((sign_pattern >> k) & 1u) != 0u;
      if (mine) blk[((uint32_t)y << g.lwe) + (uint32_t)x] = neg ? -val : val;
    }
  }
}

}  // namespace

// C: the type the coefficients are stored as — int32_t (the reference's TCoeff) or int16_t (streams of 15-bit dynamic range: half
// the bytes back over PCIe for the host-pointer path; a level that does not fit sets CABAC_RES_RANGE and is stored truncated)
//
// kSide (cabac_hip_parse_unit.h): the substream is a run of side records with the blocks spliced in at positions.  The walk then
// alternates between the block walk above and a record walk in the manner of cabac_hip_decode_device on ONE context store of all
// 379 contexts (slot = ctxId).  The records are fetched as the input bytes are: 64 at a time, one coalesced 2-byte load per
// lane, the next 64 a step ahead, a record reaching the scalar side by v_readlane; the decoded bins are collected in the lanes
// (lane i holds the bin of record i of the group) and stored 64 at a time, a partial group in front of every block and at a stop.
//
// kSide == 2 (cabac_hip_parse_elements.h): the run is a PLAN of syntax elements (word0 of the binariser's record, word1 a guard)
// and every element is decoded to its value.  The plan is fetched as the records are (one coalesced 8-byte load per lane, the next
// 64 elements a step ahead).  The values go to a per-wave ring of 256 words in LDS (`ring`, owned by the kernel so that the other
// instantiations' LDS stays what it is): a guard reads value(i - back), back <= 255, from it, across group boundaries and blocks,
// and the values are stored from it 64 at a time, a partial group in front of every block and at a stop.  Every lane writes the
// (wave-uniform) value to the ring, so each lane reads back what it wrote itself.
//
// kSide == 3 (cabac_hip_parse_plan.h): the element walk with two more entry kinds that read no bin.  CABAC_PE_COND is a test
// on the ring, joined by AND / OR with another ring word; CABAC_PE_BLOCK_INFO is a field of the info word of one of the last 16
// blocks walked.  Those words live in `inf` (LDS of the kernel, per wave: 16 info words, then the count of blocks walked,
// skipped ones included), written where tu_info[t] is written, by every lane as the ring is, and read back the same way.  Both
// kinds are wave-uniform scalar work in the element loop; everything else is the kSide == 2 walk, instruction for instruction.
//
// Context sets (cabac_hip_plan_rows.h): the plan walk takes them the way the codec kernels do, as a trailing parameter PACK — empty
// for every instantiation the plain entry points launch, whose signature, arguments and code are then the ones from before the
// sets, and one ParseSets for the sets and rows calls.  Everything about sets is in the overloads below and behind
// `if constexpr (kSets)` in the walk: the LOAD (the init loop reads the start set instead), the EXPORT (all 64 lanes store the
// slots when the walk arrives at entry out_at, or behind the last block), and the bad index, checked once per substream.
struct ParseSets {
  CtxSets cs;
  const uint32_t *out_at;  // per substream the entry at which its contexts are handed over (null: behind the substream)
  uint32_t start_bound;    // a start index at or above it (other than "no set") is a bad one: n_sets, or the level's first row
  uint32_t slot_base;      // 0xffffffff: out sets as cs.out_set says; otherwise substream s writes set slot_base + s (rows)
};
struct ParseSetUse {
  const uint32_t *start;  // the start set's states (null: Ctx::init)
  uint32_t *out_state;    // where the out set goes (null: nowhere)
  uint8_t *out_rate;
  uint32_t out_at;
  bool bad;
};
__device__ __forceinline__ ParseSetUse parse_set_use(uint32_t, bool) { return ParseSetUse{nullptr, nullptr, nullptr, 0xffffffffu, false}; }
__device__ __forceinline__ ParseSetUse parse_set_use(uint32_t sub, bool live, const ParseSets &ps) {
  constexpr uint32_t kNone = 0xffffffffu;
  const CtxSets &cs = ps.cs;
  const uint32_t start = (live && cs.start_set != nullptr) ? cs.start_set[sub] : kNone;
  const uint32_t out = !live ? kNone : ps.slot_base != kNone ? ps.slot_base + sub : cs.out_set != nullptr ? cs.out_set[sub] : kNone;
  ParseSetUse u;
  u.bad = (start != kNone && start >= ps.start_bound) || (out != kNone && out >= cs.n_sets);  // once per substream
  u.start = (start != kNone && !u.bad) ? cs.state + (uint64_t)start * (uint64_t)kNumCtx : nullptr;
  u.out_state = (out != kNone && !u.bad) ? cs.out_state + (uint64_t)out * (uint64_t)kNumCtx : nullptr;
  u.out_rate = (out != kNone && !u.bad) ? cs.out_rate + (uint64_t)out * (uint64_t)kNumCtx : nullptr;
  u.out_at = (live && ps.out_at != nullptr) ? ps.out_at[sub] : kNone;
  return u;
}
// the contexts the wave holds now as its out set: all 379 states, and as rates the window sizes the slots carry (m_rate, what
// cabac_hip_ctx_init_device writes).  Slot = ctxId here.
__device__ __forceinline__ void parse_ctx_export(const uint4 *ctx, uint32_t lane, const ParseSetUse &u) {
  if (u.out_state == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (uint32_t k = lane; k < (uint32_t)kNumCtx; k += 64u) {
    const uint4 e = ctx[k];
    u.out_state[k] = e.x;
    u.out_rate[k] = (uint8_t)(16u * (e.y & 0xffffu) + (e.y >> 16));
  }
}

// Pieces (cabac_hip_plan_resume.h): the plan walk from and into the sets AND from and into a coder state per substream — the
// CABAC_CODER_DEC state of cabac_hip_pieces.h as cabac_hip_decode_pieces_device writes it: bits = S, the shifts so far; priv =
// range | the value field of the window (bits 62..47) | mark | 0.  One ParsePieces in the pack; everything about the state is
// in the functions below and behind `if constexpr (kPieces)` in the walk, so that the other instantiations keep their code.
//  * LOAD: quad_piece_use<false> (cabac_quad.h) checks what the header lists, and one thing more: a state without flags stands
//    inside its slot (2 + (S >> 3) <= byte_capacity; beyond it the underrun would have been flagged, and that flag is sticky).
//    A substream that is refused, or comes with flags, leaves before anything depends on the state's values.
//  * RESUME (in the walk, behind the fresh start, which a fresh state keeps): the look-ahead below the value is raw stream and is
//    read again.  Stream bit S + 16 is the first look-ahead bit; it lies in 16-bit unit u = (S >> 4) + 1, of which the low
//    16 - (S & 15) bits are still ahead: that is `look`, and rp = 2 u + 2 (8 rp - 16 - look = S).  The unit is fetched with a block
//    load of its own: where rp is a multiple of 256 it is the last unit of the block in front of in_cur.
//  * EXPORT: behind a terminate bin 1 pd_trm leaves range - 2 unrenormalised (254 .. 508) and the value at or above it.  The
//    state is then written marked, with bit 8 of the range set as the bin decoder keeps it (254 / 255 -> 510 / 511, which no
//    other range of a marked state gives: the load takes it back), value < (range + 2) << 7.  Nothing but finish() may follow.
struct ParsePieces : ParseSets {
  const cabac_coder_state *coder_in;
  cabac_coder_state *coder_out;
};
template <class... Sets>
constexpr bool kParsePieces = (std::is_base_of_v<ParsePieces, Sets> || ...);
__device__ __forceinline__ QuadPieceUse parse_piece_use(uint32_t sub, bool live, bool bad_set, uint32_t cap, const ParsePieces &pp) {
  const CtxPieces cp{pp.cs, pp.coder_in, pp.coder_out};
  QuadPieceUse u = quad_piece_use<false>(sub, live, bad_set, cap, cp);
  if (u.code && !u.fresh && (uint64_t)2u + (u.bits >> 3) > (uint64_t)cap) {  // no flagless decoder stands outside its slot
    u.code = false;
    u.refuse = true;
  }
  // a marked state (mark is 0 or 1 here) of range 510 / 511 is pd_trm's 254 / 255: range - 2 behind a terminate bin 1
  if (u.code && !u.fresh && pp.coder_in[sub].priv[2] != 0u && u.range >= 510u) u.range -= 256u;
  return u;
}
__device__ __forceinline__ void parse_piece_pass(cabac_substream_result *results, uint32_t sub, bool first_lane, const QuadPieceUse &u,
                                                 const ParsePieces &pp) {
  quad_piece_pass(results, sub, first_lane, u, CtxPieces{pp.cs, pp.coder_in, pp.coder_out});
}
__device__ __forceinline__ cabac_coder_state *parse_piece_out(const ParsePieces &pp) { return pp.coder_out; }

template <int W, class C, int kSide, class... Sets>
__device__ __forceinline__ void parse_walk(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                           const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                           const cabac_tu_desc *__restrict__ tus, C *__restrict__ coeff_all,
                                           uint32_t *__restrict__ tu_info, cabac_substream_result *__restrict__ results,
                                           const uint32_t *__restrict__ tu_at, const uint16_t *__restrict__ records,
                                           uint8_t *__restrict__ side_bins, const uint32_t *__restrict__ tu_guard = nullptr,
                                           const uint32_t *__restrict__ plan = nullptr, uint32_t *__restrict__ values = nullptr,
                                           uint32_t *ring = nullptr, uint32_t *inf = nullptr, Sets... sets) {
  constexpr bool kSets = sizeof...(Sets) != 0;
  static_assert(!kSets || kSide == 3, "only the plan walk takes sets");
  constexpr uint32_t kSlots = kSide ? kSideCtxSlots : kCtxSlots;
  __shared__ uint4 ctx_all[W * kSlots];
  __shared__ uint32_t side_park[kSide ? W : 1];  // the record cursor while a block is walked: out of the block walk's scalar registers
  __shared__ int32_t blk_all[W * kBlkWords];
  __shared__ LdsTables tab;
  // Placement: the walk is bound by what the waves of a CU share (instruction issue, the scalar unit), so the waves must
  // be spread evenly: with 33 KB of LDS per workgroup at most four fit on a CU, and a 4 096-substream batch is exactly
  // four per CU (measured: 16 waves on every CU, 4 on every SIMD).
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  {  // scan / shape tables into LDS
    uint8_t *dst = reinterpret_cast<uint8_t *>(&tab);
    const uint8_t *g0 = &c_diag.grid[0][0][0], *g1 = &c_diag.in_cg[0][0][0];
    for (uint32_t k = threadIdx.x; k < sizeof(tab.grid); k += 64u * W) dst[offsetof(LdsTables, grid) + k] = g0[k];
    for (uint32_t k = threadIdx.x; k < sizeof(tab.in_cg); k += 64u * W) dst[offsetof(LdsTables, in_cg) + k] = g1[k];
    const uint16_t *t0 = &c_shapes.in_template[0][0][0];
    uint16_t *t1 = &tab.in_template[0][0][0];
    for (uint32_t k = threadIdx.x; k < 5u * 5u * 16u; k += 64u * W) {
      t1[k] = t0[k];
      (&tab.left[0][0][0])[k] = (&c_shapes.left[0][0][0])[k];
      (&tab.above[0][0][0])[k] = (&c_shapes.above[0][0][0])[k];
    }
  }
  const uint32_t sub = rfl(blockIdx.x * W + wave);
  const bool live = sub < n_sub;
  uint4 *ctx = ctx_all + wave * kSlots;
  int32_t *blk = blk_all + wave * kBlkWords;
  const cabac_substream_desc dsc = desc[live ? sub : 0];
  [[maybe_unused]] const ParseSetUse su = parse_set_use(sub, live, sets...);
  constexpr bool kPieces = kParsePieces<Sets...>;
  [[maybe_unused]] QuadPieceUse pu{};                       // the coder state the substream continues from, checked here
  [[maybe_unused]] cabac_coder_state *piece_out = nullptr;  // where the state behind the piece goes
  if constexpr (kPieces) {
    pu = parse_piece_use(sub, live, su.bad, dsc.byte_capacity, sets...);
    piece_out = parse_piece_out(sets...);
  }
  {
    const int qp = dsc.qp < 0 ? 0 : (dsc.qp > 63 ? 63 : dsc.qp);
    const uint32_t iid = dsc.init_id & 3u;
    for (uint32_t k = lane; k < (kSide ? (uint32_t)CABAC_NUM_CONTEXTS : 230u); k += 64u) {
      const uint32_t id = kSide ? k : id_of_slot(k);
      uint32_t packed = ctx2_init(qp, c_init_tables[iid * kNumCtx + id], c_init_tables[3 * kNumCtx + id]);
      if constexpr (kSets) {  // the state halves of the start set; the window sizes stay the init table's (they depend on the id alone)
        if (su.start != nullptr) {
          const uint32_t st = su.start[k];
          packed = (st & kMask0) | (st & (kMask1 << 16)) | (packed & 31u);
        }
      }
      const uint32_t r0 = (packed & 3u) + 2u, r1 = ((packed >> 2) & 7u) + 5u;
      ctx[k] = make_uint4(packed & ~31u, r0 | (r1 << 16), ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16), 0u);
    }
    for (uint32_t k = lane; k < kBlkWords; k += 64u) blk[k] = 0;
  }
  __syncthreads();
  if (!live) return;
  if constexpr (kPieces) {
    // a state that is refused: {0, CABAC_RES_BAD_STATE} and nothing else; one that comes with flags, or a bad set index of this
    // piece: {0, flags} and the state copied.  No value, coefficient, info word or set either way.
    if (rfl(pu.code ? 1u : 0u) == 0u) {
      parse_piece_pass(results, sub, lane == 0u, pu, sets...);
      return;
    }
  }
  if constexpr (kSets) {
    if (su.bad) {  // a start or out index beyond the sets: nothing is parsed, nothing is written but the result
      if (lane == 0u) {
        cabac_substream_result r;
        r.n_bits = 0u;
        r.flags = 0x40u;  // CABAC_RES_BAD_SET
        results[sub] = r;
      }
      return;
    }
  }

  // every other wave SLOT of a SIMD keeps its decoder on the scalar pipe (pd_bin): whatever the placement, the waves that
  // share a SIMD split about evenly
#ifndef CABAC_PARSE_SCALAR_WAVES
#define CABAC_PARSE_SCALAR_WAVES 0   // 0: none, 1: every other wave slot, 2: all.  Measured on the bench tiles: 6.30 / 6.73 / - ms
#endif
  const bool scalar_wave = CABAC_PARSE_SCALAR_WAVES == 2 ||
                           (CABAC_PARSE_SCALAR_WAVES == 1 && (__builtin_amdgcn_s_getreg((4) | (0 << 6) | (3 << 11)) & 1u) != 0u);   // HW_ID.wave_id[3:0]
  auto walk = [&](auto kind) {
  typedef PDecT<decltype(kind)::value, kSide != 0> D;
  D d;
  d.lane = lane;
  d.cap = dsc.byte_capacity;
  const uint8_t *src = bytes + dsc.byte_offset;
  d.src_safe = d.cap != 0u ? src : reinterpret_cast<const uint8_t *>(desc);
  d.last_dword = d.cap != 0u ? ((d.cap - 1u) & ~3u) : 0u;
  d.in_cur = pd_load_block(d, 0u);
  d.in_nxt = pd_load_block(d, 1u);
  {  // start(), arith_codec.cpp:60-66
    const uint32_t first = rl(d.in_cur, 0u);
    d.hi = first >> 1;
    d.lo = first << 31;
  }
  d.look = 16;
  d.rp = 4u;
  d.range = 510u;
  [[maybe_unused]] bool resumed = false;
  if constexpr (kPieces) {
    resumed = rfl(pu.fresh) == 0u;
    if (resumed) {  // the window of a decoder that has shifted S bits (ParsePieces, above).  Plain code: this runs once.
      const uint32_t s0 = rfl(pu.bits), value = rfl(pu.value), range = rfl(pu.range);
      const uint32_t at = 2u * ((s0 >> 4) + 1u);           // byte offset of the unit that holds stream bit S + 16
      const uint32_t dw = rl(pd_load_block(d, at >> 8), (at >> 2) & 63u);
      const uint32_t unit = (at & 2u) ? (dw & 0xffffu) : (dw >> 16);
      const uint32_t look = 16u - (s0 & 15u);              // 1 .. 16 bits of it are still ahead
      const uint64_t win = ((uint64_t)value << 47) | ((uint64_t)(unit & (0xffffu >> (16u - look))) << (47u - look));
      d.hi = (uint32_t)(win >> 32);
      d.lo = (uint32_t)win;
      d.look = (int32_t)look;
      d.rp = at + 2u;
      d.in_cur = pd_load_block(d, d.rp >> 8);
      d.in_nxt = pd_load_block(d, (d.rp >> 8) + 1u);
      d.range = range;
    }
  }
  // A substream that begins with the byte 0xFF is not one the arithmetic coder wrote: its first nine bits are the coder's
  // value, which is below the initial range 510.  Decoding it would leave value >= range << 7, a state in which the
  // reference's arithmetic and this one's part ways, so it is refused as a whole: no block is parsed, BAD_STOP.
  const bool bad_start = !resumed && d.cap >= 2u && (rl(d.in_cur, 0u) >> 24) == 0xffu;
  uint32_t flags_out = bad_start ? CABAC_RES_BAD_STOP : 0u;

  const uint32_t t_end = bad_start ? tile_first[sub] : tile_first[sub + 1];
  PP_TICK(k0);
  // side walk: i = the next record of the run, n_rec its length; rec_cur / rec_nxt = records 64 * (i >> 6) + lane and the 64
  // behind them; bins_v = the bins of the current group, stored from record `stored` on
  const uint32_t n_rec = (kSide && !bad_start) ? dsc.n_records : 0u;
  [[maybe_unused]] bool hand_over = kSets;  // the out set is still to be written
  uint32_t rec_i = 0, stored = 0, rec_cur = 0, rec_nxt = 0, bins_v = 0;
  auto load_records = [&](uint32_t group) {
    const uint32_t k = 64u * group + lane;
    return k < n_rec ? (uint32_t)records[dsc.rec_offset + k] : 0u;
  };
  auto store_bins = [&](uint32_t upto) {  // lane = record of the current group: the bins of records [stored, upto)
    const uint32_t k = ((upto - 1u) & ~63u) + lane;
    if (k >= stored && k < upto) side_bins[dsc.rec_offset + k] = (uint8_t)bins_v;
  };
  if (kSide == 1 && n_rec != 0u) {
    rec_cur = load_records(0u);
    rec_nxt = load_records(1u);
  }
  // element walk: el_cur / el_nxt = the plan words of the current group and of the 64 elements behind it
  uint2 el_cur = make_uint2(0u, 0u), el_nxt = make_uint2(0u, 0u);
  auto load_plan = [&](uint32_t group) {
    const uint32_t k = 64u * group + lane;
    return k < n_rec ? reinterpret_cast<const uint2 *>(plan)[dsc.rec_offset + k] : make_uint2(0xfu, 0u);
  };
  auto store_values = [&](uint32_t upto) {  // the values of elements [stored, upto) of the current group, out of the ring
    const uint32_t k = ((upto - 1u) & ~63u) + lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (k >= stored && k < upto) values[dsc.rec_offset + k] = ring[k & 255u];
  };
  // value(i - back) cmp imm (cabac_hip_parse_elements.h, "Guard word"); back != 0 and back <= i
  auto guard_holds = [&](uint32_t gw, uint32_t i) {
    const uint32_t v = rfl(ring[(i - (gw & 0xffu)) & 255u]), imm = gw >> 16, cmp = (gw >> 8) & 3u;
    return cmp == 0u ? v != imm : cmp == 1u ? v == imm : cmp == 2u ? v >= imm : v < imm;
  };
  // the block that is walked next is block inf[16] of the substream; its info word goes to inf[that & 15]
  auto note_info = [&](uint32_t info) {
    const uint32_t k = rfl(inf[16]);
    inf[k & 15u] = info;
    inf[16] = k + 1u;
  };
  if (kSide == 3) inf[16] = 0u;
  if (kSide >= 2 && n_rec != 0u) {
    el_cur = load_plan(0u);
    el_nxt = load_plan(1u);
  }
  for (uint32_t t = tile_first[sub]; kSide || t < t_end; t++) {
    if (kSide >= 2) {
      uint32_t upto = n_rec;
      if (t < t_end && tu_at) upto = min(max(tu_at[t], rec_i), n_rec);
      uint32_t stop = 0;
      while (rec_i < upto) {
        if constexpr (kSets) {
          if (rec_i == su.out_at) {  // wave-uniform: the walk arrives at the hand-over entry, every block in front of it walked
            parse_ctx_export(ctx, lane, su);
            hand_over = false;
          }
        }
        pd_check(d);  // 32 look-ahead bits for the element's first step; the longer code words check again as they go
        const uint32_t w0 = rl(el_cur.x, rec_i & 63u), gw = rl(el_cur.y, rec_i & 63u);
        const uint32_t kind = w0 & 15u, p = w0 >> 4, id0 = p & 0x1ffu, idn = (p >> 9) & 0x1ffu;
        // a bad entry, whatever its guard would say: the substream stops in front of it
        bool bad = kind > (kSide == 3 ? CABAC_PE_BLOCK_INFO : CABAC_SE_ALIGN) || (gw & 0xfc00u) != 0u || (gw & 0xffu) > rec_i;
        if (kind == CABAC_SE_CTX_BIN) bad |= id0 >= (uint32_t)CABAC_NUM_CONTEXTS;
        else if (kind == CABAC_SE_UNARY_MAX) bad |= id0 >= (uint32_t)CABAC_NUM_CONTEXTS || idn >= (uint32_t)CABAC_NUM_CONTEXTS;
        else if (kind == CABAC_SE_EP_BINS || kind == CABAC_SE_UNARY_EP) bad |= (p & 63u) > 32u;
        else if (kind == CABAC_SE_TRUNC_BIN) bad |= p == 0u;
        else if (kind == CABAC_SE_REM_ABS) {
          const uint32_t ml = (p >> 10) & 63u;
          bad |= (p & 31u) > 14u || ml < 15u || ml > 20u || ((p >> 5) & 31u) > 32u - ml;
        } else if (kSide == 3 && kind == CABAC_PE_COND) {  // p: back2 in bits 7..0, join in 9..8; gw is the test
          const uint32_t back2 = p & 0xffu, join = (p >> 8) & 3u;
          bad |= join == 3u || (join != 0u && (back2 == 0u || back2 > rec_i));
        } else if (kSide == 3 && kind == CABAC_PE_BLOCK_INFO) {  // p: which in bits 3..0, shift in 8..4, width in 14..9
          const uint32_t width = (p >> 9) & 63u;
          bad |= (p & 15u) >= rfl(inf[16]) || width == 0u || ((p >> 4) & 31u) + width > 32u;
        }
        if (bad) {
          stop = CABAC_RES_BAD_RECORD;
          break;
        }
        uint32_t v = 0;
        if (kSide == 3 && kind == CABAC_PE_COND) {  // never skipped: word1 is a test, not a guard
          v = (gw & 0xffu) == 0u || guard_holds(gw, rec_i);
          const uint32_t join = (p >> 8) & 3u;
          if (join != 0u) {
            const uint32_t other = rfl(ring[(rec_i - (p & 0xffu)) & 255u]) != 0u;
            v = join == 1u ? (v & other) : (v | other);
          }
        } else if ((gw & 0xffu) == 0u || guard_holds(gw, rec_i)) {
          if (kind == CABAC_SE_CTX_BIN) {
            v = pd_bin(d, ctx, id0);
          } else if (kind == CABAC_SE_EP_BINS) {
            // one bin is decodeBinEP itself, the unit parse's CABAC_REC_EP: identity E1 then holds in every decoder state
            v = (p & 63u) == 1u ? pd_ep(d) : pd_bins_ep(d, p & 63u);
          } else if (kind == CABAC_SE_REM_ABS) {
            v = pd_rem_abs_cut(d, p & 31u, (p >> 5) & 31u, (p >> 10) & 63u);
          } else if (kind == CABAC_SE_TRM) {
            v = pd_trm(d);
          } else if (kind == CABAC_SE_UNARY_MAX) {  // cabac_reader.cpp:3349-3358: at most 255 context-coded bins, a check in front of each
            const uint32_t mx = (p >> 18) & 0xffu;
            while (v < mx) {
              pd_check(d);
              if (!pd_bin(d, ctx, v == 0u ? id0 : idn)) break;
              v++;
            }
          } else if (kind == CABAC_SE_UNARY_EP) {   // :3360-3368
            v = pd_ep_ones(d, p & 63u);
          } else if (kind == CABAC_SE_EXP_GOLOMB) {  // :3370-3379, the prefix bounded: count + ones < 32
            const uint32_t count = p & 31u, ones = pd_ep_ones(d, 32u - count);
            if (ones == 32u - count) {
              stop = CABAC_RES_BAD_VALUE;  // a code word no writer produces: the substream stops at this element
              break;
            }
            v = (((1u << ones) - 1u) << count) + pd_bins_ep(d, count + ones);
          } else if (kind == CABAC_SE_TRUNC_BIN) {   // cabac_reader.cpp:1162-1186
            const uint32_t thresh = 31u - (uint32_t)__builtin_clz(p), val = 1u << thresh, b = p - val;
            v = pd_bins_ep(d, thresh);
            if (v >= val - b) {
              pd_check(d);
              v = (v << 1) + pd_ep(d) - (val - b);
            }
          } else if (kSide == 3 && kind == CABAC_PE_BLOCK_INFO) {  // block nb(i) - 1 - which, nb(i) = inf[16]
            const uint32_t width = (p >> 9) & 63u, word = rfl(inf[(rfl(inf[16]) - 1u - (p & 15u)) & 15u]);
            v = (word >> ((p >> 4) & 31u)) & (width >= 32u ? 0xffffffffu : (1u << width) - 1u);
          } else {  // CABAC_SE_ALIGN
            d.range = 256u;
          }
        }
        ring[rec_i & 255u] = v;
        rec_i++;
        if ((rec_i & 63u) == 0u) {
          store_values(rec_i);
          stored = rec_i;
          el_cur = el_nxt;
          el_nxt = load_plan((rec_i >> 6) + 1u);
        }
      }
      if (stored < rec_i) {  // a partial group: in front of every block and at a stop
        store_values(rec_i);
        stored = rec_i;
      }
      if (stop != 0u) {
        flags_out |= stop;
        break;
      }
      if (t >= t_end) break;
      if (tu_guard) {  // the block's guard refers to element at(t) - back; a skipped block's descriptor is not examined
        const uint32_t gw = tu_guard[t];
        if ((gw & 0xfc00u) != 0u || (gw & 0xffu) > rec_i) {
          flags_out |= CABAC_RES_BAD_RECORD;
          break;
        }
        if ((gw & 0xffu) != 0u && !guard_holds(gw, rec_i)) {
          if (tu_info && lane == 0u) tu_info[t] = CABAC_TU_INFO_NOT_CODED;
          if (kSide == 3) note_info(CABAC_TU_INFO_NOT_CODED);
          continue;
        }
      }
      if (lane == 0u) side_park[wave] = rec_i;
    } else if (kSide) {
      // at(t) = min(max(tu_at[t], at(t - 1)), n_rec); behind the last block the rest of the run
      uint32_t upto = n_rec;
      if (t < t_end && tu_at) upto = min(max(tu_at[t], rec_i), n_rec);
      bool bad = false;
      while (rec_i < upto) {
        pd_check(d);  // 32 look-ahead bits; a record consumes at most 7
        const uint32_t id = rl(rec_cur, rec_i & 63u) & CABAC_REC_ID_MASK;
        uint32_t bin = 0;
        if (id < (uint32_t)CABAC_NUM_CONTEXTS) {
          bin = pd_bin(d, ctx, id);
        } else if (id == CABAC_REC_EP) {
          bin = pd_ep(d);
        } else if (id == CABAC_REC_TRM) {  // decodeBinTrm, arith_codec.cpp:181-197: decoding goes on whatever the bin is
          const uint32_t range = rfl(d.range) - 2u;
          bin = rfl(d.hi) >= (range << 22) ? 1u : 0u;
          d.range = range;
          if (!bin && range < 256u) {
            const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << 1;
            d.hi = (uint32_t)(v >> 32);
            d.lo = (uint32_t)v;
            d.look -= 1;
            d.range = range << 1;
          }
        } else if (id == CABAC_REC_ALIGN) {
          d.range = 256u;
        } else {
          bad = true;  // no record of the codec: the substream stops in front of it
          break;
        }
        bins_v = lane == (rec_i & 63u) ? bin : bins_v;
        rec_i++;
        if ((rec_i & 63u) == 0u) {
          store_bins(rec_i);
          stored = rec_i;
          rec_cur = rec_nxt;
          rec_nxt = load_records((rec_i >> 6) + 1u);
        }
      }
      if (stored < rec_i) {  // a partial group: in front of every block and at a stop
        store_bins(rec_i);
        stored = rec_i;
      }
      if (bad) {
        flags_out |= CABAC_RES_BAD_RECORD;
        break;
      }
      if (t >= t_end) break;
      if (lane == 0u) side_park[wave] = rec_i;
    }
    PP_TICK(b0);
    const cabac_tu_desc tu = tus[t];
    BlockGeom g;
    const uint32_t lw = tu.log2_width, lh = tu.log2_height;
    g.chroma = tu.channel;
    g.fl = tu.flags;
    g.max_log2 = tu.max_log2_tr_range ? tu.max_log2_tr_range : 15u;
    if (lw > 6u || lh > 6u || g.chroma > 1u || g.max_log2 > 20u || g.max_log2 < 15u) {
      flags_out |= CABAC_RES_BAD_RECORD;  // a block this parser does not cover: stop here
      break;
    }
    geom_init(g, lw, lh);
    // ts_flag, cabac_reader.cpp:2737-2752: in the stream where transform skip is allowed, else as the descriptor says
    uint32_t ts = (g.fl & CABAC_TU_TRANSFORM_SKIP) ? 1u : 0u;
    if (g.fl & CABAC_TU_TS_FLAG) {
      pd_check(d);
      ts = pd_bin(d, ctx, SL_TS_FLAG(g.chroma));
    }
    if (ts && (lw > 5u || lh > 5u)) {
      flags_out |= CABAC_RES_BAD_RECORD;
      break;
    }
    uint32_t info = CABAC_TU_INFO_TS;
    PP_TICK(b1);
    PP_ADD(0, b0, b1);
    if (ts) parse_ts(d, ctx, blk, tab, g, lane);
    else if ((g.fl & CABAC_TU_SBT_ZERO_OUT) && g.chroma == 0u && g.lw <= 5u && g.lh <= 5u) info = parse_regular<decltype(d), true>(d, ctx, blk, tab, g, lane);
    else info = parse_regular<decltype(d), false>(d, ctx, blk, tab, g, lane);
    if (tu_info && lane == 0u) tu_info[t] = info;
    if (kSide == 3) note_info(info);
    PP_TICK(b2);
    // the finished block goes out row by row (all lanes), the LDS copy is cleared for the next block
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    C *out = coeff_all + tu.coeff_offset;
    uint32_t outside = 0;  // int16_t: a level beyond the type
    for (uint32_t i = lane; i < g.we * g.he; i += 64u) {
      const int32_t v = blk[i];
      out[((i >> g.lwe) << lw) + (i & (g.we - 1u))] = (C)v;
      if (sizeof(C) == 2) outside |= ((uint32_t)v + 32768u) >> 16;
      blk[i] = 0;
    }
    if (sizeof(C) == 2 && __ballot(outside != 0u) != 0ull) flags_out |= CABAC_RES_RANGE;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    PP_TICK(b3);
    PP_ADD(7, b2, b3);
#ifdef CABAC_PARSE_PROFILE
    if (blockIdx.x == 0 && threadIdx.x == 0) g_parse_prof[12] += 1;  // blocks
#endif
    if (kSide) stored = rec_i = rfl(side_park[wave]);  // (the barriers of the write-out order the lanes' accesses)
  }
  if constexpr (kSets) {
    if (hand_over) parse_ctx_export(ctx, lane, su);  // out_at at or behind the end of the plan, or a stop in front of it
  }
  PP_TICK(k1);
  PP_ADD(8, k0, k1);
#ifdef CABAC_PARSE_PROFILE
  if (lane == 0u) {  // spread of the waves' walk times, and when (after the first wave's start) the last one ended
    atomicMin(&g_parse_prof[13], k1 - k0);
    atomicMax(&g_parse_prof[14], k1 - k0);
    atomicAdd(&g_parse_prof[15], k1 - k0);
    if (sub < 8192u) {
      g_parse_wave[3 * sub] = k0;
      g_parse_wave[3 * sub + 1] = k1;
      g_parse_wave[3 * sub + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)) |
                                  ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)) << 32);
    }
  }
#endif

  // encodeBinTrm(1) closes the substream (cabac_writer.cpp:104-107); decodeBinTrm, arith_codec.cpp:181-197
  uint32_t trm = 1;
  // (not after a refused block or a refused start: the parse stopped before the end of the substream.  CABAC_RES_RANGE does
  // not stop anything.)
  // (the side walk has no implied terminate bin: it is a side record; CABAC_SUB_FINISH is the stop check alone)
  const bool finish = (dsc.init_id & CABAC_SUB_FINISH) &&
                      !(flags_out & (CABAC_RES_BAD_RECORD | CABAC_RES_BAD_STOP | (kSide >= 2 ? CABAC_RES_BAD_VALUE : 0u)));
  if (finish && !kSide) {
    pd_check(d);
    const uint32_t range = rfl(d.range) - 2u, hi = rfl(d.hi);
    trm = hi >= (range << 22) ? 1u : 0u;
    if (!trm && range < 256u) {
      const uint64_t v = (((uint64_t)d.hi << 32) | d.lo) << 1;
      d.hi = (uint32_t)(v >> 32);
      d.lo = (uint32_t)v;
      d.look -= 1;
    }
  }
  // the reference's counters (arith_codec.cpp:257-260) from the bits consumed: everything moved into the window
  // (8 * rp) minus value (16) minus look-ahead
  const uint32_t shifts = 8u * d.rp - 16u - rfl((uint32_t)d.look);
  const uint32_t bytes_read = 2u + (shifts >> 3);
  const int32_t bits_needed = (int32_t)(shifts & 7u) - 8;
  if (bytes_read > d.cap) {
    // an underrun throws before finish() is reached — and before a block behind it could be refused: reported alone
    flags_out = (flags_out & CABAC_RES_RANGE) | CABAC_RES_UNDERRUN;
  } else if (finish) {
    // finish(), arith_codec.cpp:68-73: the last byte read holds the stop bit where the decoder stands
    const uint32_t lastb = src[bytes_read - 1u];
    const bool stop_ok = ((lastb << (8 + bits_needed)) & 0xffu) == 0x80u;
    if (!(trm && stop_ok)) flags_out |= CABAC_RES_BAD_STOP;
  }
  if (lane == 0u) {
    cabac_substream_result r;
    r.n_bits = 8u * bytes_read + (uint32_t)bits_needed;
    r.flags = flags_out;
    results[sub] = r;
  }
  if constexpr (kPieces) {
    // the state behind the piece (ParsePieces, above): eight plain vector stores from lane 0.  CABAC_RES_RANGE is the piece's
    // own and is not kept; every other flag is sticky (BAD_STOP can only be the refused 0xFF start here, or the last piece's).
    if (lane == 0u && piece_out != nullptr) {
      const uint32_t range = rfl(d.range), value = (rfl(d.hi) >> 15) & 0xffffu;
      const uint32_t mark = (range < 256u || value >= (range << 7)) ? 1u : 0u;
      const bool closed = (dsc.init_id & CABAC_SUB_FINISH) != 0u;
      uint32_t *q = reinterpret_cast<uint32_t *>(piece_out + sub);
      q[0] = closed ? CABAC_CODER_CLOSED : CABAC_CODER_DEC;
      q[1] = flags_out & ~(uint32_t)CABAC_RES_RANGE;
      q[2] = shifts;
      q[3] = 0u;
      q[4] = closed ? 0u : (range | 256u);
      q[5] = closed ? 0u : value;
      q[6] = closed ? 0u : mark;
      q[7] = 0u;
    }
  }
  };
  if (scalar_wave) walk(std::true_type{});
  else walk(std::false_type{});
}

template <int W, class C>
__global__ __launch_bounds__(64 * W) void residual_parse_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                  const uint8_t *__restrict__ bytes,
                                                                  const uint32_t *__restrict__ tile_first,
                                                                  const cabac_tu_desc *__restrict__ tus, C *__restrict__ coeff_all,
                                                                  uint32_t *__restrict__ tu_info,
                                                                  cabac_substream_result *__restrict__ results) {
  parse_walk<W, C, 0>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, nullptr, nullptr, nullptr);
}

template <int W, class C>
__global__ __launch_bounds__(64 * W) void unit_parse_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                              const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                                              const cabac_tu_desc *__restrict__ tus, const uint32_t *__restrict__ tu_at,
                                                              const uint16_t *__restrict__ records, C *__restrict__ coeff_all,
                                                              uint8_t *__restrict__ side_bins, uint32_t *__restrict__ tu_info,
                                                              cabac_substream_result *__restrict__ results) {
  parse_walk<W, C, 1>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, tu_at, records, side_bins);
}

// the element walk (cabac_hip_parse_elements.h): the parser's geometry, the plan in place of the records
template <int W, class C>
__global__ __launch_bounds__(64 * W) void element_parse_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                 const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                                                 const cabac_tu_desc *__restrict__ tus, const uint32_t *__restrict__ tu_at,
                                                                 const uint32_t *__restrict__ tu_guard, const uint32_t *__restrict__ plan,
                                                                 C *__restrict__ coeff_all, uint32_t *__restrict__ values,
                                                                 uint32_t *__restrict__ tu_info, cabac_substream_result *__restrict__ results) {
  __shared__ uint32_t ring_all[W * 256];  // the last 256 values of each wave's substream
  parse_walk<W, C, 2>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, tu_at, nullptr, nullptr, tu_guard, plan, values,
                      ring_all + 256u * (threadIdx.x >> 6));
}

// the plan walk (cabac_hip_parse_plan.h): the element walk's geometry and ring, and the info words of the last 16 blocks
template <int W, class C>
__global__ __launch_bounds__(64 * W) void plan_parse_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                              const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                                              const cabac_tu_desc *__restrict__ tus, const uint32_t *__restrict__ tu_at,
                                                              const uint32_t *__restrict__ tu_guard, const uint32_t *__restrict__ plan,
                                                              C *__restrict__ coeff_all, uint32_t *__restrict__ values,
                                                              uint32_t *__restrict__ tu_info, cabac_substream_result *__restrict__ results) {
  __shared__ uint32_t ring_all[W * 256];  // the last 256 values of each wave's substream
  __shared__ uint32_t info_all[W * 17];   // per wave: the info words of the last 16 blocks walked, and how many were walked
  parse_walk<W, C, 3>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, tu_at, nullptr, nullptr, tu_guard, plan, values,
                      ring_all + 256u * (threadIdx.x >> 6), info_all + 17u * (threadIdx.x >> 6));
}

// the plan walk from and into context sets (cabac_hip_plan_rows.h): the same geometry and LDS, one ParseSets more
template <int W, class C>
__global__ __launch_bounds__(64 * W) void plan_parse_sets_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                   const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                                                   const cabac_tu_desc *__restrict__ tus, const uint32_t *__restrict__ tu_at,
                                                                   const uint32_t *__restrict__ tu_guard, const uint32_t *__restrict__ plan,
                                                                   C *__restrict__ coeff_all, uint32_t *__restrict__ values,
                                                                   uint32_t *__restrict__ tu_info, cabac_substream_result *__restrict__ results,
                                                                   ParseSets ps) {
  __shared__ uint32_t ring_all[W * 256];
  __shared__ uint32_t info_all[W * 17];
  parse_walk<W, C, 3>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, tu_at, nullptr, nullptr, tu_guard, plan, values,
                      ring_all + 256u * (threadIdx.x >> 6), info_all + 17u * (threadIdx.x >> 6), ps);
}

// the plan walk in pieces (cabac_hip_plan_resume.h): the sets form with a coder state per substream in and out
template <int W, class C>
__global__ __launch_bounds__(64 * W) void plan_parse_pieces_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                     const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ tile_first,
                                                                     const cabac_tu_desc *__restrict__ tus, const uint32_t *__restrict__ tu_at,
                                                                     const uint32_t *__restrict__ tu_guard, const uint32_t *__restrict__ plan,
                                                                     C *__restrict__ coeff_all, uint32_t *__restrict__ values,
                                                                     uint32_t *__restrict__ tu_info, cabac_substream_result *__restrict__ results,
                                                                     ParsePieces pp) {
  __shared__ uint32_t ring_all[W * 256];
  __shared__ uint32_t info_all[W * 17];
  parse_walk<W, C, 3>(n_sub, desc, bytes, tile_first, tus, coeff_all, tu_info, results, tu_at, nullptr, nullptr, tu_guard, plan, values,
                      ring_all + 256u * (threadIdx.x >> 6), info_all + 17u * (threadIdx.x >> 6), pp);
}

#ifdef CABAC_PARSE_PROFILE
hipError_t debug_read_parse_waves(unsigned long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_parse_wave), sizeof(unsigned long long) * 3 * 8192);
}
hipError_t debug_read_parse_prof(unsigned long long *out) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_parse_prof), sizeof(unsigned long long) * 16);
  unsigned long long zero[16] = {};
  zero[13] = ~0ull;
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_parse_prof), zero, sizeof zero);
  return e;
}
#endif

// The family's two host choices, each made once: int16_t or int32_t coefficients, and one wave per workgroup or four.  `launch`
// receives the waves as a std::integral_constant, the typed coefficients, the grid and the workgroup, and launches its kernel.
template <class F>
static hipError_t parse_dispatch(uint32_t n_sub, const ParseIn &in, F launch) {
  auto as = [&](auto *coeff) {
    // four waves per workgroup, one per SIMD of the CU; small batches spread single waves over the chip
    if (n_sub >= 1024u) launch(std::integral_constant<int, 4>{}, coeff, dim3((n_sub + 3u) / 4u), dim3(256));
    else launch(std::integral_constant<int, 1>{}, coeff, dim3(n_sub), dim3(64));
    return hipGetLastError();
  };
  if (in.coeff_bytes == 2) return as(static_cast<int16_t *>(in.coeff));
  if (in.coeff_bytes == 4) return as(static_cast<int32_t *>(in.coeff));
  return hipErrorInvalidValue;
}

// What a launch lambda is given, as the kernels' template arguments
#define PARSE_W decltype(w)::value
#define PARSE_C std::remove_pointer_t<decltype(coeff)>

// The forms, in the order their kernels have in the code object.
static hipError_t unit_walk(hipStream_t st, uint32_t n_sub, const ParseIn &in) {
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((unit_parse_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus, in.tu_at,
                       in.records, coeff, in.side_bins, in.tu_info, in.results);
  });
}

static hipError_t element_walk(hipStream_t st, uint32_t n_sub, const ParseIn &in) {
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((element_parse_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus,
                       in.tu_at, in.tu_guard, in.plan, coeff, in.values, in.tu_info, in.results);
  });
}

static hipError_t plan_walk(hipStream_t st, uint32_t n_sub, const ParseIn &in) {
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((plan_parse_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus, in.tu_at,
                       in.tu_guard, in.plan, coeff, in.values, in.tu_info, in.results);
  });
}

hipError_t launch_plan_parse_sets(hipStream_t st, uint32_t n_sub, const ParseIn &in, const CtxSets &sets, const uint32_t *out_at,
                                  uint32_t start_bound, uint32_t slot_base) {
  if (n_sub == 0) return hipSuccess;
  const ParseSets ps{sets, out_at, start_bound, slot_base};
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((plan_parse_sets_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus,
                       in.tu_at, in.tu_guard, in.plan, coeff, in.values, in.tu_info, in.results, ps);
  });
}

hipError_t launch_plan_parse_pieces(hipStream_t st, uint32_t n_sub, const ParseIn &in, const CtxPieces &pieces) {
  if (n_sub == 0) return hipSuccess;
  ParsePieces pp;  // the out set is behind the piece, always: no hand-over entry; start indices below n_sets; out sets as out_set says
  pp.cs = pieces;
  pp.out_at = nullptr;
  pp.start_bound = pieces.n_sets;
  pp.slot_base = 0xffffffffu;
  pp.coder_in = pieces.coder_in;
  pp.coder_out = pieces.coder_out;
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((plan_parse_pieces_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus,
                       in.tu_at, in.tu_guard, in.plan, coeff, in.values, in.tu_info, in.results, pp);
  });
}

static hipError_t residual_walk(hipStream_t st, uint32_t n_sub, const ParseIn &in) {
  return parse_dispatch(n_sub, in, [&](auto w, auto *coeff, dim3 grid, dim3 group) {
    hipLaunchKernelGGL((residual_parse_kernel<PARSE_W, PARSE_C>), grid, group, 0, st, n_sub, in.desc, in.bytes, in.tile_first, in.tus, coeff,
                       in.tu_info, in.results);
  });
}

hipError_t launch_parse(hipStream_t st, ParseWalk walk, uint32_t n_sub, const ParseIn &in) {
  if (n_sub == 0) return hipSuccess;
  switch (walk) {
  case ParseWalk::kResidual: return residual_walk(st, n_sub, in);
  case ParseWalk::kUnit: return unit_walk(st, n_sub, in);
  case ParseWalk::kElement: return element_walk(st, n_sub, in);
  case ParseWalk::kPlan: return plan_walk(st, n_sub, in);
  }
  return hipErrorInvalidValue;
}

}  // namespace cabac
