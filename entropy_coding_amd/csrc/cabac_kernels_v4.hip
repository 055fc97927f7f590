// v4 "quad" kernels: FOUR substreams per wavefront, 16 lanes each, serial chain on the VECTOR pipe.
//
// Measured cost model of gfx950 (tools/ubench_*.hip): a wave issues one instruction per
// ~4.4 cycles, scalar or vector, dependent or not; a SIMD executes one wave-wide integer instruction per
// ~2.2 cycles (two waves per SIMD both run at full speed); a scalar instruction that consumes a vector
// result stalls the wave ~55 cycles.  With one substream per wave (v1, v3) every instruction of the serial
// low/range chain advances ONE bin.  Here the four 16-lane rows of a wave carry four different substreams and
// the chain is written with per-lane (row-uniform) vector arithmetic, so one instruction advances FOUR bins;
// the record of step i is delivered to its row with a DPP row broadcast (v_mov_b32_dpp row_newbcast:i — one
// instruction, no LDS, no scalar round trip).  Everything row-divergent is mask arithmetic; the only
// branches are the rare ones (output of whole 16-bit units; the decoder's input has none).
//
//  encode: per 16-bin step  (a) quad_resolve: the context state each of the 16 bins of a row sees (match-any
//          on ctxId, then every lane applies the earlier bins of its context itself);  (b) 16 unrolled
//          chain steps of 23 vector instructions for the 4 rows together.  encode_kernel_v4 does both in one
//          wave, encode_kernel_v5 in two (context wave / chain wave, see there).
//          Byte output: `low` is kept as the exact code value and 16 bits are peeled off whenever 16
//          have accumulated; the delayed carry of arith_codec.cpp:524-546 (buffered byte + count of
//          outstanding 0xFF) is the same algorithm in base 2^16 (buffered unit + count of outstanding
//          0xFFFF).  The emitted stream is the identical number: the top S+1 bits of low >> 8 with
//          carries resolved (S = bits shifted), which is what finish() (:339-357) leaves.
//  decode: a 64-bit look-ahead window per row, topped up from a bit cursor every fourth bin without a
//          branch.  The context states: a step in which no row has a context more than twice (chosen a step ahead,
//          quad_dec_steps_pairs) prepares what the chain needs of them lane-parallel in front of the chain and
//          brings them up to date once behind it; in any other step every lane applies every bin to its own copy of
//          the state and the lanes of that row holding the same ctxId keep it.
//  estimate: BitEstimator_Std on the same records — quad_resolve plus a table lookup, no chain.
//
// Layout: row r of wave w codes substream 4w + r.  Rows whose substreams are shorter idle at the end,
// so batches should group substreams of similar length (cabac_hip.h: order is the caller's).
#include <cstdlib>
#include <type_traits>

#include "cabac_device.h"
#include "cabac_kernels.h"
#include "cabac_quad.h"

namespace cabac {

// ---------------------------------------------------------------------------------------------
// encode

struct QuadEnc {       // row-uniform values
  uint64_t low;        // exact code value: 9 + pend (+1 carry) bits; pend <= 15 + 4*7 between flush checks
  uint32_t range;
  int32_t pend;        // bits shifted since the last 16-bit unit was peeled off (< 16 between steps)
  uint32_t buf;        // buffered unit
  int32_t nbuf;        // buffered unit + outstanding 0xFFFF units
  uint32_t pos;        // bytes stored so far
  uint8_t *dst;
  uint32_t cap;
};

__device__ __forceinline__ void quad_put_byte(QuadEnc &e, uint32_t byte, bool writer) {
  if (writer && e.pos < e.cap) e.dst[e.pos] = (uint8_t)byte;
  e.pos += 1;
}

__device__ __forceinline__ void quad_put16(QuadEnc &e, uint32_t unit, bool writer) {
  // big-endian 16-bit unit at byte offset pos (pos is even until finish)
  if (writer) {
    if (e.pos + 2u <= e.cap) {
      *reinterpret_cast<uint16_t *>(e.dst + e.pos) = (uint16_t)(((unit & 0xffu) << 8) | ((unit >> 8) & 0xffu));
    } else if (e.pos < e.cap) {
      e.dst[e.pos] = (uint8_t)(unit >> 8);
    }
  }
  e.pos += 2;
}

// one 16-bit unit with the carry that arrived on top of it (lead = carry << 16 | unit): delayed carry as
// writeOut (arith_codec.cpp:524-546), in base 2^16
__device__ __forceinline__ void quad_flush_lead(QuadEnc &e, uint32_t lead, bool writer) {
  const bool is_ff = lead == 0xffffu;
  const bool emit = !is_ff && e.nbuf > 0;
  const uint32_t carry = lead >> 16;
  const uint32_t first = e.buf + carry;
  const int32_t fill_n = e.nbuf - 1;
  e.buf = is_ff ? e.buf : (lead & 0xffffu);
  e.nbuf = is_ff ? e.nbuf + 1 : 1;
  if (emit) {
    quad_put16(e, first, writer);
    for (int32_t k = 0; k < fill_n; k++) quad_put16(e, 0xffffu + carry, writer);
  }
}

// peel 16 bits (and the carry above them) off the top of low
__device__ __forceinline__ void quad_flush16(QuadEnc &e, bool writer) {
  const uint32_t sh = (uint32_t)(9 + e.pend - 16);
  const uint32_t lead = (uint32_t)(e.low >> sh);  // carry + 16 bits
  e.low &= (1ull << sh) - 1ull;
  e.pend -= 16;
  quad_flush_lead(e, lead, writer);
}

// Where the chain wave of the two-wave encoder (v5) leaves its output: every 4th bin it posts (low, pend) to LDS
// and keeps only the pend % 16 bits that are not yet a whole unit; the context wave peels the units off the
// posted value one step later (quad_flush16) — the carry / output stage is serial per unit and full of
// per-row conditions, and on the chain wave it cost 30 % of the kernel.
struct QuadPost {
  uint32_t *lo, *hi, *pend;  // [check 0..3][row 0..3] of the current step's slot, already offset to this row
};

// Per-lane fields of one bin for the chain (phase A fills them; all zero = no-op step)
struct QuadEncInfo {
  uint32_t k;     // LPS factor (state folded to 0..127) >> 2; 0 for bypass / terminate
  uint32_t c2;    // 2 * constant term of the LPS width: 8 context bin, 4 terminate bin, 0 bypass
  uint32_t lpsm;  // ~0 if this bin takes the LPS path (context: bin != mps; terminate: bin == 1)
  uint32_t ep;    // 1 for a bypass bin
  uint32_t pem;   // ~0 for a bypass bin with value 1
  uint32_t alm;   // ~0 for an align() record
};

// One chain step for the four rows.  The fields reach the row by DPP row broadcasts; masks are used
// with and/bfi (no compares, no exec regions): the wave is alone on its SIMD and every VALU->SALU->EXEC
// round trip would sit on the critical path.
template <int I, bool kAlign, bool kPost>
__device__ __forceinline__ void quad_enc_step(const QuadEncInfo &f, QuadEnc &e, bool writer, const QuadPost &post) {
  const uint32_t k = row_bcast<I>(f.k), c2 = row_bcast<I>(f.c2), lpsm = row_bcast<I>(f.lpsm), ep = row_bcast<I>(f.ep);
  const uint32_t t = (__umul24((e.range >> 5) & 15u, k) + c2) >> 1;  // LPS width: ((r>>5)*k>>1) + c
  const uint32_t rm = e.range - t;
  const uint32_t nl = (uint32_t)(__builtin_clz(t) - 23);  // getRenormBitsLPS (contexts.cpp:952-954); masked out when t == 0
  const uint32_t nm = (rm >> 8) ^ 1u;                     // rm < 512: 1 iff rm < 256
  const uint32_t nb = sel(lpsm, nl, nm);
  e.range = sel(lpsm, t, rm) << nb;
  // low = ((low + (LPS ? rm : 0)) << nb), then for a bypass bin (low << 1) + bin * range (arith_codec.cpp:389-399,
  // :553-582).  The two additions exclude each other, so both go after ONE shift: a single 64-bit shift and
  // add per bin keep the 64-bit dependency chain short.
  const uint32_t term = ((rm & lpsm) << nb) | (e.range & row_bcast<I>(f.pem));
  e.low = (e.low << (nb + ep)) + term;
  if (kAlign) e.range = sel(row_bcast<I>(f.alm), 256u, e.range);
  e.pend += (int32_t)(nb + ep);
  // output check only every 4th bin: 4 bins shift at most 28 bits, which the 64-bit low absorbs, and the
  // three steps in between stay in one basic block, so hipcc can overlap their independent parts
  if ((I & 3) == 3) {
    if (kPost) {
      constexpr int kCheck = (I >> 2) * kQuadSubs;
      if (writer) {
        post.lo[kCheck] = (uint32_t)e.low;
        post.hi[kCheck] = (uint32_t)(e.low >> 32);
        post.pend[kCheck] = (uint32_t)e.pend;
      }
      // whole units, and the carry above them, now belong to the post; without a whole unit nothing is cut
      // (a carry bit above the 9 + pend bits must stay until it can be posted on top of a unit)
      const uint32_t keep = (uint32_t)e.pend & 15u;
      const uint32_t width = e.pend >= 16 ? 9u + keep : 63u;
      e.low &= ~(~0ull << width);
      e.pend = (int32_t)keep;
    } else {
      while (__builtin_expect(e.pend >= 16, 0)) quad_flush16(e, writer);
    }
  }
}

template <bool kAlign, bool kPost>
__device__ __forceinline__ void quad_enc_steps(const QuadEncInfo &f, QuadEnc &e, bool writer, const QuadPost &post) {
#define QSTEP(I) quad_enc_step<I, kAlign, kPost>(f, e, writer, post)
  QSTEP(0); QSTEP(1); QSTEP(2); QSTEP(3); QSTEP(4); QSTEP(5); QSTEP(6); QSTEP(7);
  QSTEP(8); QSTEP(9); QSTEP(10); QSTEP(11); QSTEP(12); QSTEP(13); QSTEP(14); QSTEP(15);
#undef QSTEP
}

__device__ __forceinline__ QuadEncInfo quad_unpack(uint32_t info) {
  QuadEncInfo f;
  f.k = info & 31u;
  f.c2 = (info >> 5) & 15u;
  f.lpsm = bit_mask<9>(info);
  f.ep = (info >> 10) & 1u;
  f.pem = bit_mask<11>(info);
  f.alm = bit_mask<12>(info);
  return f;
}

// finish(), arith_codec.cpp:339-357, on the exact code value (+ writeByteAlignment, bit_stream.cpp:152-155)
// probe (CABAC_SUB_PROBE): no flush; the answer of getNumWrittenBits() (arith_codec.cpp:482-485) instead — every shift so far
// has either left as a stored unit (8 * pos), waits as the buffered unit or an outstanding 0xFFFF (16 * nbuf), or is
// still inside low (pend)
__device__ __forceinline__ uint32_t quad_enc_finish(QuadEnc &e, bool align_rbsp, bool writer, bool probe = false) {
  if (probe) return 8u * e.pos + 16u * (uint32_t)e.nbuf + (uint32_t)e.pend;
  const uint32_t total = (uint32_t)(9 + e.pend);
  if ((e.low >> total) & 1ull) {
    quad_put16(e, e.buf + 1u, writer);
    for (int32_t k = 1; k < e.nbuf; k++) quad_put16(e, 0x0000u, writer);
    e.low -= 1ull << total;
  } else {
    if (e.nbuf > 0) quad_put16(e, e.buf, writer);
    for (int32_t k = 1; k < e.nbuf; k++) quad_put16(e, 0xffffu, writer);
  }
  uint32_t nb = (uint32_t)(e.pend + 1);  // write(low >> 8, 24 - bitsLeft)
  const uint32_t v = (uint32_t)(e.low >> 8);
  while (nb >= 8) {
    quad_put_byte(e, (v >> (nb - 8)) & 0xffu, writer);
    nb -= 8;
  }
  uint32_t held = nb ? ((v & ((1u << nb) - 1u)) << (8 - nb)) : 0u;
  if (align_rbsp) {
    held |= 1u << (7 - nb);
    quad_put_byte(e, held, writer);
    held = 0;
    nb = 0;
  }
  const uint32_t n_bits = e.pos * 8u + nb;
  if (nb) quad_put_byte(e, held, writer);
  return n_bits;
}

// encode, one wave per 4 substreams: phase (a) and the chain alternate in the same wave
template <class... Sets>
__global__ __launch_bounds__(64) void encode_kernel_v4(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                       const uint16_t *__restrict__ records, uint8_t *__restrict__ bytes,
                                                       cabac_substream_result *__restrict__ results, Sets... sets) {
  constexpr bool kSets = sizeof...(Sets) != 0;
  constexpr bool kPieces = kQuadPieces<Sets...>;  // cabac_hip_pieces.h: the coder state comes from and goes to memory
  __shared__ uint32_t ctx[kQuadSubs * kQuadCtxStride];
  const uint32_t lane = threadIdx.x, row = lane >> 4, j = lane & 15u;
  const uint32_t sub = blockIdx.x * kQuadSubs + row;
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, sets...);
  bool live = sub < n_sub && !su.bad;  // rows beyond the batch idle with n = 0
  const cabac_substream_desc d = desc[live ? sub : 0];
  // (pieces: the state is checked here, where it is loaded; a row that is refused or comes with flags codes nothing and
  // writes no set)
  QuadPieceUse pu{};
  QuadSetUse su_out = su;
  if constexpr (kPieces) {
    pu = quad_piece_use<true>(sub, sub < n_sub, su.bad, d.byte_capacity, sets...);
    live = live && pu.code;
    if (pu.refuse) su_out.out = kNoSet;
  }
  const uint32_t n = live ? d.n_records : 0u;
  const uint16_t *rec = records + d.rec_offset;
  uint32_t *rctx = ctx + row * kQuadCtxStride;
  if constexpr (kSets) quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, sets...);
  else quad_ctx_init(rctx, d.qp, d.init_id & 3u, j);
  __syncthreads();

  QuadEnc e;
  e.low = 0;
  e.range = 510;  // start(), arith_codec.cpp:329-337
  e.pend = 0;
  e.buf = 0;
  e.nbuf = 0;
  e.pos = 0;
  if constexpr (kPieces) {  // checked by quad_piece_use: pend < 16, low inside its 10 + pend bits, pos + 2 nbuf <= the capacity
    e.low = pu.low;
    e.range = pu.range;
    e.pend = (int32_t)pu.pend;
    e.buf = pu.buf;
    e.nbuf = (int32_t)pu.nbuf;
    e.pos = pu.pos;
  }
  e.dst = bytes + d.byte_offset;
  e.cap = live ? d.byte_capacity : 0u;
  const bool writer = live && j == 0;
  uint32_t bad = 0;

  uint32_t next_rec = j < n ? rec[j] : 0;
  for (uint32_t base = 0; __ballot(base < n) != 0; base += 16) {
    const uint32_t r = next_rec;  // loaded one step ago
    const uint32_t info = quad_phase_a(r, base + j < n, lane, row, rctx, bad);
    const QuadEncInfo f = quad_unpack(info);
    // prefetch the next 16 records of each row now: the load completes under the serial chain.  (Issued
    // any earlier, hipcc's s_waitcnt vmcnt(0) in front of the first use of `r` would wait for it too.)
    {
      const uint32_t nxt = base + 16u + j;
      next_rec = nxt < n ? rec[nxt] : 0;
    }
    // (b) the serial chain, 4 rows at once
    if (__ballot(info >> 12) == 0) quad_enc_steps<false, false>(f, e, writer, QuadPost());
    else quad_enc_steps<true, false>(f, e, writer, QuadPost());
  }

  if constexpr (kPieces) {
    // A piece without FINISH flushes nothing: every step has run its flush checks for all sixteen places, so pend < 16 here, and
    // what is left — low, the buffered unit, the outstanding 0xFFFF units — is the state.  All of the buffered units will be
    // written, so a slot they do not fit into overflows now, as it will in the end.
    const CtxPieces &cp = quad_pack_first(sets...);
    const bool fin = (d.init_id & CABAC_SUB_FINISH) != 0;
    const uint32_t n_bits = live ? quad_enc_finish(e, (d.init_id & CABAC_SUB_ALIGN_RBSP) != 0, writer, !fin) : 0u;
    const uint64_t bad_mask = __ballot(bad != 0);
    const bool row_bad = ((bad_mask >> (row * 16u)) & 0xffffull) != 0;
    if (writer) {
      const uint32_t ends = fin ? e.pos : e.pos + 2u * (uint32_t)e.nbuf;
      cabac_substream_result res;
      res.n_bits = n_bits;
      res.flags = (ends > e.cap ? CABAC_RES_OVERFLOW : 0u) | (row_bad ? CABAC_RES_BAD_RECORD : 0u);
      results[sub] = res;
      if (fin) quad_piece_store(cp, sub, CABAC_CODER_CLOSED, res.flags, n_bits, e.pos, 0u, 0u, 0u, 0u);
      else quad_piece_store(cp, sub, CABAC_CODER_ENC, res.flags, n_bits, e.pos, (uint32_t)e.low, e.range | ((uint32_t)e.pend << 16), e.buf,
                            (uint32_t)e.nbuf);
    }
    quad_piece_pass(results, sub, sub < n_sub && j == 0, pu, cp);
    __syncthreads();
    quad_ctx_export(rctx, j, 16u, su_out, sets...);
    return;
  }
  const uint32_t n_bits = live ? quad_enc_finish(e, (d.init_id & CABAC_SUB_ALIGN_RBSP) != 0, writer, (d.init_id & CABAC_SUB_PROBE) != 0) : 0u;
  const uint64_t bad_mask = __ballot(bad != 0);  // row-wide OR of the bad-record flag
  const bool row_bad = ((bad_mask >> (row * 16u)) & 0xffffull) != 0;
  if (writer) {
    cabac_substream_result res;
    res.n_bits = n_bits;
    res.flags = (e.pos > e.cap ? CABAC_RES_OVERFLOW : 0u) | (row_bad ? CABAC_RES_BAD_RECORD : 0u);
    results[sub] = res;
  }
  if constexpr (kSets) {
    __syncthreads();  // the store of the last step's phase (a) (surplus steps of shorter rows write the pad word only)
    quad_ctx_export(rctx, j, 16u, su, sets...);
    quad_bad_set_result(results, sub, j == 0, su);
  }
}

// ---- output stage of the two-wave encoder (runs on the context wave) ---------------------------------
// The chain wave posts (low, pend) after bins 3, 7, 11, 15 of a step.  A post with pend >= 16 carries
// pend / 16 whole 16-bit units (at most two) and possibly a carry above them; the units of one step are at
// most eight per row.  quad_flush16 is the exact, serial rule for one unit.  Almost always every row is in
// the plain state "one unit buffered, no 0xFFFF run, no new unit equals 0xFFFF, room in the buffer", and
// then the rule degenerates to "store the previous unit plus the carry that arrived with this one": that
// is done for all units of the four rows at once, lane k of a row taking unit k, through a small LDS list.
// Anything else (first unit of a substream, 0xFFFF runs, a full buffer) takes the serial path.
constexpr uint32_t kUnitSlots = 12;  // 8 units + spare + a dump slot for lanes that have nothing to list
constexpr uint32_t kUnitDump = 11;

template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {  // lane j gets lane j - N of its row, 0 below
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xf, 0xf, true);
}

// Everything below is written with 0 / ~0 masks in VGPRs (neg_mask, sel): boolean expressions become lane masks in SGPRs,
// and every scalar instruction that consumes a vector result stalls the wave for ~55 cycles.

struct QuadUnits {
  uint32_t m;            // units of this step in the row (0..8)
  uint64_t odd_rows;     // lanes of rows that are not in the plain state (before looking at the units themselves);
                         // kept as the raw mask: a scalar compare right behind the v_cmp would wait for it
  uint64_t store_lanes;  // lanes that will store a unit
};

// Part 1: lanes 0..3 of a row list the units of posts 0..3 in stream order.  kLanes = 4: a substream has FOUR lanes (a DPP
// quad, four substreams per 16-lane row, j = lane & 3), one per post, so the counts a row shift brings in from the
// neighbouring substream are masked away.  Lane j then stores unit j: a step with more than four units — it can produce
// eight, an all-LPS run; an ordinary mix produces about one — is "not plain" and takes the serial path.
template <int kLanes = 16>
__device__ __forceinline__ QuadUnits quad_list_units(const QuadEnc &e, const uint32_t *plo, const uint32_t *phi,
                                                     const uint32_t *ppend, uint32_t row, uint32_t j, bool live,
                                                     uint32_t *list) {
  static_assert(kLanes == 16 || kLanes == 4, "a row or a quad per substream");
  const uint32_t c = (j & 3u) * kQuadSubs + row;  // lanes >= 4 read along, and count nothing
  const uint64_t low = ((uint64_t)phi[c] << 32) | plo[c];
  const uint32_t pend = ppend[c];
  const uint32_t nun = kLanes == 4 ? pend >> 4 : (pend >> 4) & neg_mask(j - 4u);  // 0, 1 or 2 units
  const uint64_t v = low >> (9u + (pend & 15u));         // carry, then the units
  uint32_t incl = nun + (kLanes == 4 ? row_shr<1>(nun) & neg_mask(0u - j) : row_shr<1>(nun));
  incl += kLanes == 4 ? row_shr<2>(incl) & neg_mask(1u - j) : row_shr<2>(incl);
  const uint32_t idx = incl - nun;
  const uint32_t first = (uint32_t)(v >> (((nun - 1u) & 1u) << 4));  // carry + first unit (nun >= 1)
  const uint32_t second = (uint32_t)v & 0xffffu;                      // second unit (nun == 2)
  const uint32_t has1 = neg_mask(0u - nun);                           // nun >= 1
  const uint32_t has2 = neg_mask(1u - nun);                           // nun == 2
  list[sel(has1, idx, kUnitDump)] = first;
  list[sel(has2, idx + 1u, kUnitDump)] = second;
  QuadUnits u;
  u.m = group_bcast<kLanes, 3>(incl);
  const uint32_t room = e.cap - e.pos - 2u * u.m;                     // negative: the buffer would overflow
  uint32_t rowodd = neg_mask(0u - u.m) & (neg_mask(0u - ((uint32_t)e.nbuf ^ 1u)) | neg_mask(room));
  if (kLanes == 4) rowodd |= neg_mask(4u - u.m);                      // five to eight units: more than the lanes
  u.odd_rows = __ballot(live && rowodd != 0);   // (rows without a substream never store: nothing to be careful about)
  u.store_lanes = __ballot(live && j < u.m);
  return u;
}

// the serial path: the listed units of one step, one by one
__device__ __forceinline__ void quad_flush_list(QuadEnc &e, uint32_t m, const uint32_t *list, bool writer) {
  for (uint32_t k = 0; k < 8u && __ballot(k < m) != 0; k++) {
    if (k < m) quad_flush_lead(e, list[k], writer);
  }
}

// Part 2: emit the listed units (one step later, so that neither the list nor the masks are waited for).
__device__ __forceinline__ void quad_emit_units(QuadEnc &e, const QuadUnits &u, uint32_t j, const uint32_t *list,
                                                bool writer) {
  if (u.odd_rows != 0) return quad_flush_list(e, u.m, list, writer);
  const uint32_t act = neg_mask(j - u.m);  // lane j holds unit j
  const uint32_t jnz = neg_mask(0u - j);
  const uint32_t before = list[sel(act & jnz, j - 1u, kUnitDump)];
  const uint32_t mine = list[sel(act, j, kUnitDump)];
  const uint32_t last = list[sel(neg_mask(0u - u.m), u.m - 1u, kUnitDump)];
  const uint32_t x = (mine & 0x1ffffu) ^ 0xffffu;  // 0: no carry, unit 0xFFFF — starts or extends a run
  if (__ballot((act & neg_mask(x - 1u)) != 0) != 0) return quad_flush_list(e, u.m, list, writer);
  const uint32_t prev = sel(jnz, before & 0xffffu, e.buf);
  const uint32_t unit = prev + (mine >> 16);  // buf + carry (writeOut, arith_codec.cpp:524-546, in base 2^16)
  const uint32_t be = ((unit & 0xffu) << 8) | ((unit >> 8) & 0xffu);
  uint8_t *addr = e.dst + e.pos + 2u * j;
  uint64_t saved;
  asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tglobal_store_short %2, %3, off\n\ts_mov_b64 exec, %0"
               : "=&s"(saved) : "s"(u.store_lanes), "v"(addr), "v"(be) : "memory");
  e.buf = sel(neg_mask(0u - u.m), last & 0xffffu, e.buf);
  e.pos += 2u * u.m;
}

// encode, THREE waves per 4 substreams ("v5"): a context wave runs phase (a) one step ahead and owns the LDS
// context stores; a chain wave runs the range / low recurrence and nothing else; an output wave turns what the
// chain wave posts into bytes.  They never wait on each other's memory: the hand-offs are one packed word per bin
// through a double-buffered LDS mailbox (context -> chain), the posted (low, pend) of every 4th bin (chain ->
// output, see QuadPost) and one workgroup barrier per 16-bin step.  A wave issues at most one instruction per
// ~4.4 cycles while a SIMD executes one per ~2.2 (tools/ubench_ilp.hip): the chain wave (~420 instructions per
// step, raised priority) sets the pace, and the other two (~170 and ~100) fit into the issue slots it cannot use.
// All units of a workgroup run the same number of steps (the longest substream's) so that the barrier counts
// match; surplus steps are no-ops.
#ifdef CABAC_V5_PROFILE  // tools/ubench_v5.hip: where the two waves of workgroup 0 spend their cycles
__device__ unsigned long long g_v5_prof[32];
#define V5_TICK(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define V5_ADD(slot, t0, t1) \
  if (blockIdx.x == 0 && lane == 0) g_v5_prof[slot] += (t1) - (t0)
// where the hardware put wave `w` of workgroup 0: the whole HW_ID register (id 4, 32 bits; its bits 5..4 are the SIMD), one read
#define V5_HW_ID(w) \
  if (blockIdx.x == 0 && lane == 0) g_v5_prof[16 + (w)] = 0x100000000ull | (uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11))
#else
#define V5_TICK(var)
#define V5_ADD(slot, t0, t1)
#define V5_HW_ID(w)
#endif
#ifndef CABAC_V5_STAMP_UNIT   // v7: the unit whose context wave is stamped (unit 0 shares its SIMD with unit 3's, 1 with the low wave, 2 with the output wave)
#define CABAC_V5_STAMP_UNIT 0
#endif

// (encode_kernel_v5, the three-wave encoder described above, was retired in round 3: v6 and v7 below grew out of it and it
// was never dispatched after them; its pieces that they share — QuadPost, quad_list_units, quad_emit_units — stay.)

// ---------------------------------------------------------------------------------------------
// v6: the three-wave encoder with `low` taken out of the chain wave.
//
// In v5 the chain wave — the wave that sets the pace — spends 9 of its 23 instructions per bin on the code value: the
// addend, the 64-bit shift-and-add, the count of pending bits.  None of that feeds back into the range recurrence.  Here
// the chain wave only runs the range recurrence (14 instructions per bin) and leaves, per bin, the twelve bits the code
// value needs — rm (the MPS sub-range, nine bits) and the renormalisation shift (three) — in eight row-uniform registers
// it posts once per 16-bin step.  The output wave rebuilds the code value from them, exactly, with the lanes:
//   low' = (low << sh) + term per bin  (arith_codec.cpp:389-399, :553-582)   =>   over a step
//   new  = (acc << S) + sum_I term_I << (sh_{I+1} + .. + sh_15),   S = sh_0 + .. + sh_15,
// a sum of sixteen shifted 16-bit terms into a number of up to 138 bits: lane I forms (term_I, sh_I) of its bin, and a
// four-level tree over the row (row_shr 1, 2, 4, 8) combines neighbouring segments — (left << S_right) + right — in 64,
// 64, 96 and 160 bits; the remainder carried from the step before (9 bits, the bits of the unfinished 16-bit unit and a
// carry) enters as part of lane 0's term.  All carries inside `new` are resolved by the exact additions; the one carry
// that can leave its top lands on the buffered unit, as in writeOut (arith_codec.cpp:524-546).  The whole 16-bit units
// are then cut off the top by the lanes (lane k takes unit k) and go through v5's emission (quad_emit_units).
struct QuadRngCap {
  uint32_t w[8];  // bins 2k (low half) and 2k + 1 (high half): rm | shift << 9
};

template <int I, bool kAlign>
__device__ __forceinline__ void quad_rng_step(const QuadEncInfo &f, uint32_t &range, QuadRngCap &cap) {
  const uint32_t k = row_bcast<I>(f.k), c2 = row_bcast<I>(f.c2), lpsm = row_bcast<I>(f.lpsm);
  const uint32_t t = (__umul24((range >> 5) & 15u, k) + c2) >> 1;  // LPS width: ((r>>5)*k>>1) + c
  const uint32_t rm = range - t;
  // One renormalisation rule for both paths: the new range is the chosen sub-range shifted up to [256, 511].  LPS:
  // clz(t) - 23 is getRenormBitsLPS (contexts.cpp:952-954; 7 for the terminate bin's t = 2).  MPS: rm >= 128 always
  // (an LPS width is at most 15.5 / 32 of the range plus 4), so the shift is 1 iff rm < 256 (arith_codec.cpp:389-399).
  const uint32_t x = sel(lpsm, t, rm);
  const uint32_t nb = (uint32_t)(__builtin_clz(x) - 23);
  range = x << nb;
  if (kAlign) range = sel(row_bcast<I>(f.alm), 256u, range);
  const uint32_t w = rm | (nb << 9);
  if (I & 1) cap.w[I >> 1] |= w << 16;
  else cap.w[I >> 1] = w;
}

// the same with the row-uniform fields of the 16 bins in registers (read back from LDS, where lane I parked bin I's: an
// LDS read of one address by all lanes of a row is the broadcast — three v_mov_b32_dpp per bin less, see QuadDecRow)
struct QuadEncRow {
  uint32_t k[16], c2[16], lpsm[16];
};
template <int I, bool kAlign>
__device__ __forceinline__ void quad_rng_step_row(const QuadEncRow &u, const QuadEncInfo &f, uint32_t &range, QuadRngCap &cap) {
  const uint32_t t = (__umul24((range >> 5) & 15u, u.k[I]) + u.c2[I]) >> 1;  // LPS width: ((r>>5)*k>>1) + c
  const uint32_t rm = range - t;
  const uint32_t x = sel(u.lpsm[I], t, rm);
  const uint32_t nb = (uint32_t)(__builtin_clz(x) - 23);
  range = x << nb;
  if (kAlign) range = sel(row_bcast<I>(f.alm), 256u, range);
  const uint32_t w = rm | (nb << 9);
  if (I & 1) cap.w[I >> 1] |= w << 16;
  else cap.w[I >> 1] = w;
}
template <bool kAlign>
__device__ __forceinline__ void quad_rng_steps_row(const QuadEncRow &u, const QuadEncInfo &f, uint32_t &range, QuadRngCap &cap) {
#define QSTEP(I) quad_rng_step_row<I, kAlign>(u, f, range, cap)
  QSTEP(0); QSTEP(1); QSTEP(2); QSTEP(3); QSTEP(4); QSTEP(5); QSTEP(6); QSTEP(7);
  QSTEP(8); QSTEP(9); QSTEP(10); QSTEP(11); QSTEP(12); QSTEP(13); QSTEP(14); QSTEP(15);
#undef QSTEP
}

template <bool kAlign>
__device__ __forceinline__ void quad_rng_steps(const QuadEncInfo &f, uint32_t &range, QuadRngCap &cap) {
#define QSTEP(I) quad_rng_step<I, kAlign>(f, range, cap)
  QSTEP(0); QSTEP(1); QSTEP(2); QSTEP(3); QSTEP(4); QSTEP(5); QSTEP(6); QSTEP(7);
  QSTEP(8); QSTEP(9); QSTEP(10); QSTEP(11); QSTEP(12); QSTEP(13); QSTEP(14); QSTEP(15);
#undef QSTEP
}

__device__ __forceinline__ uint64_t shl64(uint32_t lo, uint32_t hi, uint32_t n) { return (((uint64_t)hi << 32) | lo) << n; }

// The code value of one step for the four rows (see above), in two parts.  Part 1 (chain wave, which has the time):
// lane I picks the twelve bits of its bin out of the row-uniform capture registers, forms (term, shift) and combines four
// bins at a time: lanes 4m + 3 end up with (value < 2^56, shift) of bins 4m .. 4m + 3.
// this lane's twelve bits (rm | shift << 9 of bin j) out of the row-uniform capture registers
__device__ __forceinline__ uint32_t quad_cap_mine(const QuadRngCap &cap, uint32_t j) {
  const uint32_t h = j >> 1;
  const uint32_t a0 = (h & 1u) ? cap.w[1] : cap.w[0], a1 = (h & 1u) ? cap.w[3] : cap.w[2], a2 = (h & 1u) ? cap.w[5] : cap.w[4],
                 a3 = (h & 1u) ? cap.w[7] : cap.w[6];
  const uint32_t b0 = (h & 2u) ? a1 : a0, b1 = (h & 2u) ? a3 : a2;
  const uint32_t pair = (h & 4u) ? b1 : b0;
  return ((j & 1u) ? pair >> 16 : pair) & 0xfffu;
}

// (term, shift) of the lane's bin and the first two tree levels: lanes 4m + 3 end up with (value < 2^56, shift) of bins 4m .. 4m + 3
__device__ __forceinline__ void quad_low_quads12(uint32_t w12, uint32_t info, uint32_t &v0, uint32_t &v1, uint32_t &s) {
  const uint32_t rm = w12 & 0x1ffu, nb = (w12 >> 9) & 7u;
  const uint32_t lpsm = bit_mask<9>(info), pem = bit_mask<11>(info), ep = (info >> 10) & 1u;
  const uint32_t term = ((rm & lpsm) << nb) | (rm & pem);  // what the bin adds to low after its shift
  s = nb + ep;                                             // ... and the shift itself
  uint64_t v = term;
  {  // bins (2m, 2m + 1) in lane 2m + 1
    const uint32_t p0 = row_shr<1>(term), ps = row_shr<1>(s);
    v = shl64(p0, 0u, s) + v;                              // < 2^24
    s += ps;
  }
  v0 = (uint32_t)v;
  {  // four bins in lane 4m + 3
    const uint32_t p0 = row_shr<2>(v0), ps = row_shr<2>(s);
    v = shl64(p0, 0u, s) + v;                              // < 2^39
    s += ps;
  }
  v0 = (uint32_t)v;
  v1 = (uint32_t)(v >> 32);
}

__device__ __forceinline__ void quad_low_quads(const QuadRngCap &cap, uint32_t info, uint32_t j, uint32_t &v0, uint32_t &v1,
                                               uint32_t &s) {
  quad_low_quads12(quad_cap_mine(cap, j), info, v0, v1, s);
}

// Part 2 (low wave): the four quads and the row's remainder `acc` (9 + rem bits and a possible carry above) -> the five
// words of `new`, in every lane of the row, and S.
__device__ __forceinline__ uint32_t quad_low_join(uint32_t v0, uint32_t v1, uint32_t s, uint32_t acc, uint32_t j, uint32_t (&out)[5]) {
  // the remainder rides on the first quad: (acc << S_quad0) + V_quad0, acc < 2^25, S_quad0 <= 28
  {
    const uint64_t a = shl64(acc & neg_mask(j - 4u), 0u, s) + ((((uint64_t)v1) << 32) | v0);  // lanes 0..3; < 2^54
    v0 = (uint32_t)a;
    v1 = (uint32_t)(a >> 32);
  }
  // eight bins in lane 8m + 7, three words
  uint32_t v2;
  {
    const uint32_t p0 = row_shr<4>(v0), p1 = row_shr<4>(v1), ps = row_shr<4>(s);  // s <= 28 here
    const uint64_t lo = shl64(p0, p1, s), hi = shl64(p1, 0u, s);                  // bits 0..63 and 32..95 of p << s
    const uint64_t a = (lo & 0xffffffffull) + v0;
    const uint64_t b = (lo >> 32) + v1 + (a >> 32);
    v0 = (uint32_t)a;
    v1 = (uint32_t)b;
    v2 = (uint32_t)(hi >> 32) + (uint32_t)(b >> 32);
    s += ps;
  }
  // the sixteen bins in lane 15, five words
  uint32_t w0, w1, w2, w3, w4;
  {
    const uint32_t p0 = row_shr<8>(v0), p1 = row_shr<8>(v1), p2 = row_shr<8>(v2), ps = row_shr<8>(s);  // s <= 56 here
    const uint32_t wide = neg_mask(31u - s);  // ~0: shift by 32 or more
    const uint32_t y0 = p0 & ~wide, y1 = sel(wide, p0, p1), y2 = sel(wide, p1, p2), y3 = p2 & wide, b = s & 31u;
    const uint64_t f01 = shl64(y0, y1, b), f12 = shl64(y1, y2, b), f23 = shl64(y2, y3, b), f34 = shl64(y3, 0u, b);
    const uint64_t a0 = (f01 & 0xffffffffull) + v0;
    const uint64_t a1 = (f01 >> 32) + v1 + (a0 >> 32);
    const uint64_t a2 = (f12 >> 32) + v2 + (a1 >> 32);
    const uint64_t a3 = (f23 >> 32) + (a2 >> 32);
    w0 = (uint32_t)a0;
    w1 = (uint32_t)a1;
    w2 = (uint32_t)a2;
    w3 = (uint32_t)a3;
    w4 = (uint32_t)(f34 >> 32) + (uint32_t)(a3 >> 32);
    s += ps;
  }
  out[0] = row_bcast<15>(w0);
  out[1] = row_bcast<15>(w1);
  out[2] = row_bcast<15>(w2);
  out[3] = row_bcast<15>(w3);
  out[4] = row_bcast<15>(w4);
  return row_bcast<15>(s);
}

#ifndef CABAC_V6_PRIO_CTX
#define CABAC_V6_PRIO_CTX 0
#define CABAC_V6_PRIO_CHAIN 3
#define CABAC_V6_PRIO_LOW 0
#define CABAC_V6_PRIO_EMIT 0
#endif
// Four waves per unit of four substreams: context wave (v5's), chain wave (range only), low wave (the code value of a
// step -> its 16-bit units) and emit wave (v5's emission: delayed carry, 0xFFFF runs, byte stores).  Measured with the
// code value and the emission in ONE output wave, that wave became the longest (its tree and its LDS round trips in a row:
// 1.02 ms against v5's 0.98); apart, each fits beside the chain wave.  One workgroup barrier per 16-bin step; step k is
// coded by the chain wave in iteration k, turned into units in iteration k + 1 and written out in iteration k + 2.
template <int U, int kSync, class... Sets>
__global__ __launch_bounds__(256 * U) void encode_kernel_v6(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                            const uint16_t *__restrict__ records,
                                                            uint8_t *__restrict__ bytes,
                                                            cabac_substream_result *__restrict__ results, Sets... sets) {
  constexpr bool kSets = sizeof...(Sets) != 0;
  // kSync 16-bin steps per workgroup barrier.  Measured (tools/ubench_v5.hip, per-role probes): every role waits ~130 ns
  // at each barrier on top of its own work, whoever arrives last.  With one unit per CU (small batches) two steps per
  // barrier are 8 % faster (C2 0.81 -> 0.75 ms, C3 17.2 -> 15.9 ms); with four units per CU the SIMDs are the limit and
  // one step per barrier is (C4 0.80 against 0.84 ms).  All hand-offs are rings of 2 kSync steps: in iteration i the
  // context wave prepares steps kSync (i + 1) + h, the chain wave runs kSync i + h, the low wave turns kSync (i - 1) + h
  // into units and the emit wave stores those of kSync (i - 2) + h (h < kSync).  Steps past the longest substream are
  // no-ops (no active record, no shift, no unit).
  __shared__ uint32_t ctx_all[U * kQuadSubs * kQuadCtxStride];
  constexpr uint32_t kRing = 2 * kSync;         // steps in flight between two neighbouring roles
  constexpr bool kTreeInChain = U == 4;         // where the first two levels of the code-value tree run (see the chain wave)
  __shared__ __attribute__((aligned(16))) uint32_t mail_all[U][kRing][4][64];   // context -> chain: per bin the packed word, k, 2c, the LPS mask
  __shared__ uint32_t quad_post[U][kRing][3][64];  // chain -> low: per lane (value low, value high, shift) of its four-bin segment
  __shared__ uint32_t unit_list[U][kRing][kQuadSubs][kUnitSlots];  // low -> emit: the units of a step, first with its carry
  __shared__ uint32_t unit_count[U][kRing][kQuadSubs];
  __shared__ uint32_t fin_acc[U][kQuadSubs], fin_rem[U][kQuadSubs];
  __shared__ uint32_t match_all[U][kMatchWords];   // the context waves' same-id bitmaps (quad_resolve)
  __shared__ uint2 rate_tab[512];
  __shared__ uint32_t bad_rows[U];
  __shared__ uint32_t wg_max_n;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = lane >> 4, j = lane & 15u;
  const uint32_t unit = wave % U, role = wave / U;  // role 0: context wave, 1: chain wave, 2: low wave, 3: emit wave
  quad_rate_tab_init(rate_tab, threadIdx.x, 256u * U);
  // the same-id lanes of the context wave through LDS (quad_resolve): C4 0.85 -> 0.81 ms, C3 16.3 -> 15.8 ms
  constexpr bool kLdsMatch = true;
  for (uint32_t k = threadIdx.x; k < U * kMatchWords; k += 256u * U) (&match_all[0][0])[k] = 0u;
  const uint32_t sub = (blockIdx.x * U + unit) * kQuadSubs + row;
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, sets...);
  const bool live = sub < n_sub && !su.bad;
  const cabac_substream_desc d = desc[live ? sub : 0];
  const uint32_t n = live ? d.n_records : 0u;
  uint32_t (*mail)[4][64] = mail_all[unit];

  if (threadIdx.x == 0) wg_max_n = 0;
  __syncthreads();
  atomicMax(&wg_max_n, n);
  __syncthreads();
  const uint32_t max_n = wg_max_n;
  const uint32_t n_iters = (max_n + 16u * kSync - 1u) / (16u * kSync);
  // every role: one barrier before the loop, one per iteration, two after it

  if (role == 0) {
    // ---- context wave ------------------------------------------------------------------------------
    __builtin_amdgcn_s_setprio(CABAC_V6_PRIO_CTX);
    const uint16_t *rec = records + d.rec_offset;
    uint32_t *rctx = ctx_all + (unit * kQuadSubs + row) * kQuadCtxStride;
    if constexpr (kSets) quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, sets...);
    else quad_ctx_init(rctx, d.qp, d.init_id & 3u, j);
    uint32_t bad = 0;
    const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
    const uint32_t last_rec = n != 0 ? n - 1u : 0u;
    auto rec_of = [&](uint32_t step) { return (uint32_t)rec_safe[min(16u * step + j, last_rec)]; };
    auto phase = [&](uint32_t step, uint32_t r) {
      const uint32_t info = quad_phase_a<kLdsMatch>(r, 16u * step + j < n, lane, row, rctx, bad, match_all[unit], rate_tab);
      uint32_t (*m)[64] = mail[step & (kRing - 1u)];
      m[0][lane] = info;
      m[1][lane] = info & 31u;
      m[2][lane] = (info >> 5) & 15u;
      m[3][lane] = bit_mask<9>(info);
    };
    // records are fetched four steps ahead: a step is shorter than a trip to HBM (measured: with one step of lead this
    // wave waited ~1 400 cycles per step for its load and was what every other wave of the unit waited for)
    uint32_t ahead[4];  // the records of the next four steps
#pragma unroll
    for (uint32_t h = 0; h < kSync; h++) phase(h, rec_of(h));
#pragma unroll
    for (uint32_t h = 0; h < 4; h++) ahead[h] = rec_of(kSync + h);
    __syncthreads();
    for (uint32_t it = 0; it < n_iters; it++) {
      const uint32_t first = kSync * (it + 1u);
      uint32_t fresh[kSync];
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) fresh[h] = rec_of(first + 4u + h);
      V5_TICK(t2);
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) phase(first + h, ahead[h]);
#pragma unroll
      for (uint32_t h = 0; h + kSync < 4; h++) ahead[h] = ahead[h + kSync];
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) ahead[4 - kSync + h] = fresh[h];
      V5_TICK(t3);
      __syncthreads();
      V5_TICK(t4);
      if (unit == 0) V5_ADD(2, t2, t3);  // phase (a)
      if (unit == 0) V5_ADD(3, t3, t4);  // waiting at the barrier
    }
    const uint64_t bad_mask = __ballot(bad != 0);
    if (lane == 0) {
      uint32_t rows = 0;
      for (uint32_t k = 0; k < 4; k++) rows |= ((bad_mask >> (16u * k)) & 0xffffull) ? (1u << k) : 0u;
      bad_rows[unit] = rows;
    }
    if constexpr (kSets) {
      // This wave alone owns the unit's context stores, and it has run phase (a) of every step of every row (the steps it runs
      // ahead of the chain are past the longest substream: no active record, the pad word): the final states are here, written
      // by this wave's own lanes — LDS executes one wave's instructions in order, so no workgroup barrier is needed, only the
      // compiler kept from moving the reads
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
      quad_ctx_export(rctx, j, 16u, su, sets...);
    }
    __syncthreads();
    __syncthreads();
  } else if (role == 1) {
    // ---- chain wave: the range recurrence and nothing else -----------------------------------------------
    __builtin_amdgcn_s_setprio(CABAC_V6_PRIO_CHAIN);
    uint32_t range = 510;  // start(), arith_codec.cpp:329-337
    __syncthreads();
    for (uint32_t it = 0; it < n_iters; it++) {
      V5_TICK(t0);
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) {
        const uint32_t slot = (kSync * it + h) & (kRing - 1u);
        const uint32_t info = mail[slot][0][lane];
        QuadEncRow u;
#pragma unroll
        for (int q = 0; q < 4; q++) {   // in bin order, so that the first four bins only wait for the first three reads
          lds_read4(&mail[slot][1][row * 16u], q, u.k);
          lds_read4(&mail[slot][2][row * 16u], q, u.c2);
          lds_read4(&mail[slot][3][row * 16u], q, u.lpsm);
        }
        QuadEncInfo f;
        f.alm = bit_mask<12>(info);
        QuadRngCap cap;
        if (__ballot(info >> 12) == 0) quad_rng_steps_row<false>(u, f, range, cap);
        else quad_rng_steps_row<true>(u, f, range, cap);
        if (kTreeInChain) {
          uint32_t q0, q1, qs;  // the first two levels of the code-value tree are done here, where there is time
          quad_low_quads(cap, info, j, q0, q1, qs);
          quad_post[unit][slot][0][lane] = q0;
          quad_post[unit][slot][1][lane] = q1;
          quad_post[unit][slot][2][lane] = qs;
        } else {                // one unit per workgroup: every wave has a SIMD to itself and this one is the longest
          quad_post[unit][slot][0][lane] = quad_cap_mine(cap, j);
          quad_post[unit][slot][1][lane] = info;
        }
      }
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      if (unit == 0) V5_ADD(4, t0, t1);   // chain + posting
      if (unit == 0) V5_ADD(5, t1, t2);   // waiting at the barrier
    }
    __syncthreads();
    __syncthreads();
  } else if (role == 2) {
    // ---- low wave: the code values of the steps of the iteration before and their whole units ------------------
    __builtin_amdgcn_s_setprio(CABAC_V6_PRIO_LOW);
    uint32_t acc = 0, rem = 0;  // row-uniform: the low 9 + rem bits of the code value (and a carry above), rem < 16
    auto list_step = [&](uint32_t step) {
      const uint32_t slot = step & (kRing - 1u);
      uint32_t w[5];
      uint32_t q0 = quad_post[unit][slot][0][lane], q1 = quad_post[unit][slot][1][lane], qs;
      if (kTreeInChain) qs = quad_post[unit][slot][2][lane];
      else quad_low_quads12(q0, q1, q0, q1, qs);
      const uint32_t s_total = quad_low_join(q0, q1, qs, acc, j, w);
      const uint32_t pendn = rem + s_total, m = pendn >> 4;  // whole units in this step: at most 7
      rem = pendn & 15u;
      const uint32_t base_off = 9u + rem;
      // unit k (k = 0 first in the stream) sits at bit base_off + 16 * (m - 1 - k); the first one with the carry above it
      const uint32_t o = base_off + 16u * ((m - 1u - min(j, m - 1u)) & 7u);
      const uint32_t wi = o >> 5;  // 0..3
      const uint32_t lo = wi >= 2u ? (wi == 3u ? w[3] : w[2]) : (wi == 1u ? w[1] : w[0]);
      const uint32_t hi = wi >= 2u ? (wi == 3u ? w[4] : w[3]) : (wi == 1u ? w[2] : w[1]);
      const uint32_t lead = (uint32_t)((((uint64_t)hi << 32) | lo) >> (o & 31u)) & (j == 0u ? 0x1ffffu : 0xffffu);
      acc = m != 0u ? w[0] & ((1u << base_off) - 1u) : w[0];
      unit_list[unit][slot][row][j < m ? j : kUnitDump] = lead;
      if (j == 0u) unit_count[unit][slot][row] = m;
    };
    __syncthreads();
    for (uint32_t it = 0; it < n_iters; it++) {
      V5_TICK(t0);
      if (it != 0) {
#pragma unroll
        for (uint32_t h = 0; h < kSync; h++) list_step(kSync * (it - 1u) + h);
      }
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      if (unit == 0) V5_ADD(1, t0, t1);   // low wave: code value + units
      if (unit == 0) V5_ADD(7, t1, t2);   // its barrier wait
    }
    if (n_iters != 0) {
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) list_step(kSync * (n_iters - 1u) + h);
    }
    if (j == 0u) {
      fin_acc[unit][row] = acc;
      fin_rem[unit][row] = rem;
    }
    __syncthreads();
    __syncthreads();
  } else {
    // ---- emit wave: the units of the steps two iterations back ------------------------------------------------
    __builtin_amdgcn_s_setprio(CABAC_V6_PRIO_EMIT);
    QuadEnc e;
    e.low = 0;
    e.range = 0;
    e.pend = 0;
    e.buf = 0;
    e.nbuf = 0;
    e.pos = 0;
    e.dst = bytes + d.byte_offset;
    e.cap = live ? d.byte_capacity : 0u;
    const bool writer = live && j == 0;
    auto emit_step = [&](uint32_t step) {
      const uint32_t slot = step & (kRing - 1u);
      const uint32_t *list = unit_list[unit][slot][row];
      QuadUnits u;
      u.m = unit_count[unit][slot][row];
      const uint32_t room = e.cap - e.pos - 2u * u.m;  // negative: the buffer would overflow
      const uint32_t rowodd = neg_mask(0u - u.m) & (neg_mask(0u - ((uint32_t)e.nbuf ^ 1u)) | neg_mask(room));
      u.odd_rows = __ballot(rowodd != 0);
      u.store_lanes = __ballot(live && j < u.m);
      quad_emit_units(e, u, j, list, writer);
    };
    __syncthreads();
    for (uint32_t it = 0; it < n_iters; it++) {
      V5_TICK(t0);
      if (it >= 2u) {
#pragma unroll
        for (uint32_t h = 0; h < kSync; h++) emit_step(kSync * (it - 2u) + h);
      }
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      if (unit == 0) V5_ADD(0, t0, t1);   // emit wave
      if (unit == 0) V5_ADD(12, t1, t2);  // its barrier wait
    }
    if (n_iters >= 2u) {  // listed in the last iteration
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) emit_step(kSync * (n_iters - 2u) + h);
    }
    __syncthreads();
    if (n_iters != 0) {   // listed after the loop
#pragma unroll
      for (uint32_t h = 0; h < kSync; h++) emit_step(kSync * (n_iters - 1u) + h);
    }
    __syncthreads();
    e.low = fin_acc[unit][row];
    e.pend = (int32_t)fin_rem[unit][row];
    const uint32_t n_bits = live ? quad_enc_finish(e, (d.init_id & CABAC_SUB_ALIGN_RBSP) != 0, writer, (d.init_id & CABAC_SUB_PROBE) != 0) : 0u;
    if (writer) {
      cabac_substream_result res;
      res.n_bits = n_bits;
      res.flags = (e.pos > e.cap ? CABAC_RES_OVERFLOW : 0u) | (((bad_rows[unit] >> row) & 1u) ? CABAC_RES_BAD_RECORD : 0u);
      results[sub] = res;
    }
    if constexpr (kSets) quad_bad_set_result(results, sub, j == 0, su);
  }
}

// ---------------------------------------------------------------------------------------------
// v7: the encoder with its serial parts turned by 90 degrees.
//
// v6 runs the range recurrence of FOUR substreams per chain wave, sixteen lanes per substream all computing the same
// value, and a SIMD executes the four waves of a unit (~740 instructions per 16-bin step) — measured, v6 is bound by
// that total, not by any one wave.  What needs the lanes of a row is only the context wave's work (which earlier bins of
// the step share my context).  Everything downstream of it is a per-substream recurrence with nothing to share, so here
// it runs one substream per LANE: per workgroup of S = 4U substreams
//   U context waves   (v6's, four substreams each, lane = bin): per bin the fields of the chain (k, c2, lpsm) and of the
//                      code value (lp9, ep), written to LDS field by field, [substream][bin] — five planes.  An align()
//                      record is given the fields of an LPS of width 256, so nothing downstream knows of it;
//   1 chain wave       lane = substream: reads its sixteen bins of the three chain fields with twelve 16-byte reads and
//                      runs the range recurrence — 9 vector instructions per bin (as compiled: bfe, mad, shift, sub,
//                      select, ffbh, sub, shift, shift-add) for ALL substreams of the workgroup instead of 13 per four —
//                      and posts rm | shift << 9 per bin with four 16-byte writes;
//   1 low wave         FOUR lanes per substream, a quarter of the step's bins each: the code value (low = (low << s) + term,
//                      64-bit), one step behind the chain — a quarter's bins folded into one update per lane, the four
//                      updates applied in order over the DPP quad (~108 instructions a step; one lane per substream and
//                      sixteen updates in a row were 175);
//   1 output wave      four lanes per substream, a post each: the 16-bit units, the delayed carry and the byte stores, two
//                      steps behind the chain.  A step of more than four units (an all-LPS run) takes the serial path.
// U + 3 waves: for U = 4 seven, dealt so that the chain wave is alone on its SIMD (see the roles below).
// One workgroup barrier per step; fields live in a ring of four steps (context waves one step ahead, low one behind).
constexpr uint32_t kV7Pad = 20;  // words per substream and field: 16 bins + 4, so that neighbouring lanes' 16-byte reads spread over the banks
enum : uint32_t { kV7K = 0, kV7C2, kV7Lpsm, kV7Lp9, kV7Ep, kV7Fields };

// One bin of the range recurrence, nine instructions.  No case for align(): its fields (quad_phase_fields) make it an LPS
// of width 256 — t = 256, rm = range - 256 in 0..255, x = 256, no shift, range = 256.
__device__ __forceinline__ uint32_t lane_rng_step(uint32_t k, uint32_t c2, uint32_t lpsm, uint32_t &range) {
  const uint32_t t = (__umul24((range >> 5) & 15u, k) + c2) >> 1;  // LPS width: ((r>>5)*k>>1) + c
  const uint32_t rm = range - t;
  const uint32_t x = sel(lpsm, t, rm);                              // see quad_rng_step
  const uint32_t nb = (uint32_t)(__builtin_clz(x) - 23);
  range = x << nb;
  return (nb << 9) + rm;                                            // rm < 512: the sum is the OR, and one shift-add
}

template <int U, class... Sets>
__global__ __launch_bounds__(64 * (U + 3)) void encode_kernel_v7(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                      const uint16_t *__restrict__ records,
                                                                      uint8_t *__restrict__ bytes,
                                                                      cabac_substream_result *__restrict__ results, Sets... sets) {
  constexpr bool kSets = sizeof...(Sets) != 0;
  constexpr bool kPieces = kQuadPieces<Sets...>;  // cabac_hip_piece_encoder.h: the coder state comes from and goes to memory
  constexpr uint32_t S = U * kQuadSubs;
  __shared__ uint32_t ctx_all[S * kQuadCtxStride];
  __shared__ __attribute__((aligned(16))) uint32_t fld[4][kV7Fields][S * kV7Pad];  // context waves -> chain / low wave
  // chain -> low: rm | shift << 9 per bin; one row per substream and one that all lanes past the last substream share (they
  // mirror it: same values) — LDS is what decides whether two workgroups fit on a CU (74 KB each, five field planes)
  __shared__ __attribute__((aligned(16))) uint32_t wpost[2][(S + 1) * kV7Pad];
  __shared__ uint32_t post_lo[U][2][4 * kQuadSubs], post_hi[U][2][4 * kQuadSubs], post_pend[U][2][4 * kQuadSubs];  // low -> output (v5's posts)
  __shared__ uint32_t fin_lo[S], fin_hi[S], fin_pend[S];
  __shared__ uint32_t fin_range[S];  // pieces only (64 bytes at U = 4; no other instantiation refers to it, so none of them holds it)
  __shared__ uint32_t unit_list[U][kQuadSubs][kUnitSlots];
  // What a record id means comes from a table (quad_resolve<.., kKindTab>) where context waves share a SIMD with the chain
  // and the low wave, U = 4: 22 of the context wave's 137 instructions per step less, 4 096 substreams 0.530 -> 0.514 ms
  // (profiles/encode_kind_table.json).  With U = 1 every wave has a SIMD of its own and the low wave sets the pace; there
  // the 16-byte rows measured 1.7 % slower (16 to 256 substreams), so it keeps the rates table and the masks from compares.
  constexpr bool kKinds = U == 4;
  constexpr uint32_t kMatch = kKinds ? kMatchWordsCtx : kMatchWords;
  __shared__ uint32_t match_all[U][kMatch];   // the context waves' same-id bitmaps (quad_resolve)
  __shared__ __attribute__((aligned(16))) uint4 kind_tab[kKinds ? kKindRows : 1];   // what a record id means, and its rates
  __shared__ uint2 rate_tab[kKinds ? 1 : 512];
  __shared__ uint32_t bad_rows[U];
  __shared__ uint32_t wg_max_n;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  V5_HW_ID(wave);
  if constexpr (kKinds) quad_kind_tab_init(kind_tab, threadIdx.x, blockDim.x);
  else quad_rate_tab_init(rate_tab, threadIdx.x, blockDim.x);
  // same-id lanes of the context waves through LDS (C4 0.81 -> 0.65 ms)
  constexpr bool kLdsMatch = true;
  for (uint32_t k = threadIdx.x; k < U * kMatch; k += blockDim.x) (&match_all[0][0])[k] = 0u;
  // Roles by wave number: U + 3 waves.  The hardware deals the waves of a workgroup to the CU's four SIMDs in turn (wave w
  // and wave w + 4 share one; which SIMD wave 0 gets varies — read from HW_ID in the profiled build, tools/ubench_v5.hip), so
  // with seven waves, U = 4, wave 3 has a SIMD to itself.  That is the chain wave: a wave alone issues an instruction every
  // ~4.8 ticks whatever depends on what (tools/ubench_lat.hip: the bin of lane_rng_step with eight, and two rewrites of it with
  // six, dependent instructions all take 43 ticks), so its ~177 instructions a step are the floor of the step, and any wave
  // that shares its SIMD comes late to the barrier (before this deal: the context wave beside it).
  //   U = 4: context 0, context 1, context 2, chain | context 3, low, output   ->   context + context | context + low |
  //          context + output | chain
  //   U = 1: context, chain, low, output — a SIMD each.
  // Context waves: lane = (row, bin) of one unit's four substreams; chain wave: lane = substream; low and output wave: FOUR
  // lanes per substream, a DPP quad (the low wave: a quarter of the step's bins each; the output wave: a post each).
  constexpr uint32_t kChainWave = U == 4 ? 3u : 1u, kLowWave = U == 4 ? 5u : 2u, kOutWave = U == 4 ? 6u : 3u;
  const bool is_chain = wave == kChainWave, is_low = wave == kLowWave, is_out = wave == kOutWave;
  const bool is_ctx = !is_chain && !is_low && !is_out;
  // the substream of this thread
  uint32_t row, j, unit, local;
  bool in_range = true;
  if (is_ctx) {
    row = lane >> 4;
    j = lane & 15u;
    unit = min(wave, U - 1u);                          // context waves 0, 1, 2 | 4 -> units 0 .. 3
    local = unit * kQuadSubs + row;
  } else if (is_chain) {
    row = lane >> 4;
    j = lane & 15u;
    unit = 0;
    in_range = lane < S;
    local = min(lane, S - 1u);
  } else {
    const uint32_t g = lane >> 2;                      // substream of the workgroup
    in_range = g < S;
    local = min(g, S - 1u);
    unit = local >> 2;
    row = local & 3u;
    j = lane & 3u;
  }
  const uint32_t sub = blockIdx.x * S + local;
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, sets...);
  bool in_batch = sub < n_sub && !su.bad;
  const cabac_substream_desc d = desc[in_batch ? sub : 0];
  // Pieces: every role loads and checks the state of its substream here (32 bytes, the same for all lanes of a substream) and
  // takes from it what it owns — the chain wave the range, the low wave low and pend, the output wave the buffered unit, the
  // count and the position.  A substream that is refused or comes with flags idles with n = 0: it keeps every barrier count,
  // writes no byte and no set (refused) and its n = 0 is what enters wg_max_n.  IN PLACE (coder_out == coder_in): these are
  // the only reads of coder_in in front of the last barrier, and they stand before the first one; the store, and the
  // re-read inside quad_piece_pass, come behind the last one, from the one lane that owns the substream (output wave).
  QuadPieceUse piece{};
  QuadSetUse su_out = su;
  if constexpr (kPieces) {
    piece = quad_piece_use<true>(sub, sub < n_sub, su.bad, d.byte_capacity, sets...);
    in_batch = in_batch && piece.code;
    if (piece.refuse) su_out.out = kNoSet;
  }
  const bool live = in_batch && in_range;
  const uint32_t n = in_batch ? d.n_records : 0u;

  if (threadIdx.x == 0) wg_max_n = 0;
  __syncthreads();
  atomicMax(&wg_max_n, n);
  __syncthreads();
  const uint32_t max_n = wg_max_n;
  const uint32_t n_steps = (max_n + 15u) >> 4;
  // every role: one barrier before the loop, one per step, two after it.  In iteration k the context waves prepare step
  // k + 1, the chain wave runs step k, the low wave step k - 1, the output waves list the units of step k - 2 and store
  // those of step k - 3.

  if (is_ctx) {
    const uint16_t *rec = records + d.rec_offset;
    uint32_t *rctx = ctx_all + local * kQuadCtxStride;
    if constexpr (kSets) quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, sets...);
    else quad_ctx_init(rctx, d.qp, d.init_id & 3u, j);
    uint32_t bad = 0;
    const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
    const uint32_t last_rec = n != 0 ? n - 1u : 0u;
    const uint32_t at = local * kV7Pad + j;
    auto post = [&](uint32_t slot, const QuadFields &f) {
      fld[slot][kV7K][at] = f.k;
      fld[slot][kV7C2][at] = f.c2;
      fld[slot][kV7Lpsm][at] = f.lpsm;
      fld[slot][kV7Lp9][at] = f.lp9;
      fld[slot][kV7Ep][at] = f.ep;
    };
    const uint32_t cur_rec = rec_safe[min(j, last_rec)];
    uint32_t next_rec = rec_safe[min(16u + j, last_rec)];
    uint32_t ahead1 = rec_safe[min(32u + j, last_rec)], ahead2 = rec_safe[min(48u + j, last_rec)], ahead3 = rec_safe[min(64u + j, last_rec)];
    post(0, quad_phase_fields<kLdsMatch, kKinds>(cur_rec, j < n, lane, row, rctx, bad, match_all[unit], rate_tab, kind_tab));  // step 0
    __syncthreads();
    for (uint32_t k = 0; k < n_steps; k++) {
      const uint32_t base = 16u * k;
      const uint32_t r = next_rec;
      next_rec = ahead1;
      ahead1 = ahead2;
      ahead2 = ahead3;
      ahead3 = rec_safe[min(base + 80u + j, last_rec)];
      V5_TICK(t0);
      post((k + 1u) & 3u, quad_phase_fields<kLdsMatch, kKinds>(r, base + 16u + j < n, lane, row, rctx, bad, match_all[unit], rate_tab, kind_tab));
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      if (unit == CABAC_V5_STAMP_UNIT) V5_ADD(0, t0, t1);
      if (unit == CABAC_V5_STAMP_UNIT) V5_ADD(1, t1, t2);
    }
    const uint64_t bad_mask = __ballot(bad != 0);
    if (lane == 0) {
      uint32_t rows = 0;
      for (uint32_t q = 0; q < 4; q++) rows |= ((bad_mask >> (16u * q)) & 0xffffull) ? (1u << q) : 0u;
      bad_rows[unit] = rows;
    }
    if constexpr (kSets) {  // as in v6: each context wave owns its unit's four stores and has run every step of them
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
      quad_ctx_export(rctx, j, 16u, su_out, sets...);  // (su_out is su but for a refused piece: no set written)
    }
    __syncthreads();
    __syncthreads();
  } else if (is_chain) {
    // ---- chain wave: lane = substream ------------------------------------------------------------------------
    __builtin_amdgcn_s_setprio(3);
    uint32_t range = 510;  // start(), arith_codec.cpp:329-337
    if constexpr (kPieces) range = piece.range;  // checked by quad_piece_use: 256..510
    __syncthreads();
    for (uint32_t k = 0; k < n_steps; k++) {
      V5_TICK(t0);
      const uint32_t slot = k & 3u;
      uint32_t kk[16], c2[16], lm[16], w[16];
      // in bin order, so that the first four bins only wait for the first three reads
#pragma unroll
      for (int q = 0; q < 4; q++) {
        lds_read4(&fld[slot][kV7K][local * kV7Pad], q, kk);
        lds_read4(&fld[slot][kV7C2][local * kV7Pad], q, c2);
        lds_read4(&fld[slot][kV7Lpsm][local * kV7Pad], q, lm);
      }
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = lane_rng_step(kk[i], c2[i], lm[i], range);
      uint4 *dst = reinterpret_cast<uint4 *>(&wpost[k & 1u][min(lane, S) * kV7Pad]);
#pragma unroll
      for (int i = 0; i < 4; i++) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      V5_ADD(2, t0, t1);
      V5_ADD(3, t1, t2);
    }
    if constexpr (kPieces) fin_range[local] = range;  // (lanes past the last substream mirror it: the same value)
    __syncthreads();
    __syncthreads();
  } else if (is_low) {
    // ---- low wave: the code value, one step behind the chain, FOUR lanes per substream.  Lane (substream, quarter q) takes
    // bins 4q .. 4q + 3 of the step with three 16-byte reads and folds them into one update of the code value,
    //   low' = (low << S) + P,   S = sh_0 + .. + sh_3,   P = sum of term_i << (sh_(i+1) + .. + sh_3)   (P < 2^40, S <= 32),
    // which needs nothing from the quarters before it.  The quarters are then joined in order over the DPP quad: in round r
    // every lane takes the state its left neighbour holds (quarter 0: the state the step began with), applies its update,
    // and cuts — what a lane holds is right from round q on and does not change after, because its input does not.  What a
    // quarter posts, (low, pend) before the cut, and where (slot q * kQuadSubs + row) is what the serial form posted after
    // bins 3, 7, 11, 15; it keeps only the pend % 16 bits that are not yet a whole unit (v5's chain wave did the same, see
    // quad_enc_step).  low < 2^58 before a cut, as there. ----
    uint64_t low = 0;       // the state behind the last quarter, in all four lanes of a substream
    uint32_t pend = 0;
    if constexpr (kPieces) {  // checked by quad_piece_use: pend < 16, low inside its 10 + pend bits — the state behind a cut (below)
      low = piece.low;
      pend = piece.pend;
    }
    const uint32_t pu = local >> 2, pr = local & 3u, q = j;
    auto quad_from_left = [](uint32_t v) {   // lane q of a quad gets lane q - 1 (quad_perm:[0,0,1,2]; quarter 0 does not use it)
      return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x90, 0xf, 0xf, true);
    };
    auto low_step = [&](uint32_t k) {
      const uint32_t slot = k & 3u;
      const uint4 w4 = reinterpret_cast<const uint4 *>(&wpost[k & 1u][local * kV7Pad])[q];
      const uint4 l4 = reinterpret_cast<const uint4 *>(&fld[slot][kV7Lp9][local * kV7Pad])[q];
      const uint4 e4 = reinterpret_cast<const uint4 *>(&fld[slot][kV7Ep][local * kV7Pad])[q];
      const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w}, lp9[4] = {l4.x, l4.y, l4.z, l4.w}, ep[4] = {e4.x, e4.y, e4.z, e4.w};
      // low = (low + (LPS ? rm : 0)) << shift for a context / terminate bin, (low << 1) + (bin ? range : 0) for a bypass
      // bin (arith_codec.cpp:389-399, :426-478); a bypass bin does not renormalise (nb = 0), so both are (rm << nb)
      uint32_t term[4], sh[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t nb = w[i] >> 9;
        term[i] = (w[i] & lp9[i]) << nb;     // < 2^16
        sh[i] = nb + ep[i];                  // <= 8
      }
      const uint32_t p01 = (term[0] << sh[1]) + term[1];          // < 2^25
      const uint64_t P = ((((uint64_t)p01 << sh[2]) + term[2]) << sh[3]) + term[3];
      const uint32_t Ssum = sh[0] + sh[1] + sh[2] + sh[3];
      uint64_t cut = 0, posted = 0;        // this quarter's state after and before its cut
      uint32_t cut_pend = 0, posted_pend = 0;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        uint64_t in = low;
        uint32_t in_pend = pend;
        if (r != 0) {
          const uint32_t lo = quad_from_left((uint32_t)cut), hi = quad_from_left((uint32_t)(cut >> 32)), pp = quad_from_left(cut_pend);
          in = q == 0 ? low : ((uint64_t)hi << 32) | lo;
          in_pend = q == 0 ? pend : pp;
        }
        posted = (in << Ssum) + P;
        posted_pend = in_pend + Ssum;
        // whole units, and the carry above them, now belong to the post; without a whole unit nothing is cut
        const uint32_t keep = posted_pend & 15u;
        const uint32_t width = posted_pend >= 16u ? 9u + keep : 63u;
        cut = posted & ~(~0ull << width);
        cut_pend = keep;
      }
      // (no `if (lane < 4 * S)`: the lanes past the last substream mirror it — same fields, same values)
      const uint32_t c = q * kQuadSubs + pr;
      post_lo[pu][k & 1u][c] = (uint32_t)posted;
      post_hi[pu][k & 1u][c] = (uint32_t)(posted >> 32);
      post_pend[pu][k & 1u][c] = posted_pend;
      low = ((uint64_t)group_bcast<4, 3>((uint32_t)(cut >> 32)) << 32) | group_bcast<4, 3>((uint32_t)cut);
      pend = group_bcast<4, 3>(cut_pend);
    };
    __syncthreads();
    for (uint32_t k = 0; k < n_steps; k++) {
      V5_TICK(t0);
      if (k != 0) low_step(k - 1u);
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      V5_ADD(4, t0, t1);
      V5_ADD(5, t1, t2);
    }
    if (n_steps != 0) low_step(n_steps - 1u);
    fin_lo[local] = (uint32_t)low;
    fin_hi[local] = (uint32_t)(low >> 32);
    fin_pend[local] = pend;
    __syncthreads();
    __syncthreads();
  } else {
    // ---- output wave: v5's (quad_list_units / quad_emit_units) with four lanes per substream, two steps behind the chain ----
    QuadEnc e;
    e.low = 0;
    e.range = 0;
    e.pend = 0;
    e.buf = 0;
    e.nbuf = 0;
    e.pos = 0;
    if constexpr (kPieces) {  // checked by quad_piece_use: pos even, pos + 2 nbuf <= the capacity
      e.buf = piece.buf;
      e.nbuf = (int32_t)piece.nbuf;
      e.pos = piece.pos;
    }
    e.dst = bytes + d.byte_offset;
    e.cap = live ? d.byte_capacity : 0u;
    const bool writer = live && j == 0;
    uint32_t *list = unit_list[unit][row];   // (lanes past the last substream of the workgroup share the last one's; they never store)
    QuadUnits units;
    units.m = 0;
    units.odd_rows = 0;
    units.store_lanes = 0;
    bool listed = false;
    auto list_step = [&](uint32_t k) {
      units = quad_list_units<4>(e, post_lo[unit][k & 1u], post_hi[unit][k & 1u], post_pend[unit][k & 1u], row, j, live, list);
    };
    // Every load of the prologue has landed before the loop.  Without this the compiler waits for one of them (a register
    // it reuses) INSIDE the loop, with vmcnt(0) — where, from the second step on, what that waits for is the round trip of
    // the step's own stores: the output wave was then the last at the barrier, 1 270 ticks busy for ~80 instructions.
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
    __syncthreads();
    for (uint32_t k = 0; k < n_steps; k++) {
      V5_TICK(t0);
      if (listed) quad_emit_units(e, units, j, list, writer);
      listed = k >= 2u;
      if (listed) list_step(k - 2u);
      V5_TICK(t1);
      __syncthreads();
      V5_TICK(t2);
      V5_ADD(6, t0, t1);
      V5_ADD(7, t1, t2);
    }
    if (listed) quad_emit_units(e, units, j, list, writer);
    if (n_steps >= 2u) {
      list_step(n_steps - 2u);
      quad_emit_units(e, units, j, list, writer);
    }
    __syncthreads();  // the low wave has posted its last step and what it still holds; bad_rows is written
    if (n_steps != 0) {
      list_step(n_steps - 1u);
      quad_emit_units(e, units, j, list, writer);
    }
    e.low = ((uint64_t)fin_hi[local] << 32) | fin_lo[local];
    e.pend = (int32_t)fin_pend[local];
    if constexpr (kPieces) {
      // The tail of encode_kernel_v4's pieces form, from the substream's first lane.  A piece without FINISH flushes nothing:
      // the low wave has cut whole units after bins 3, 7, 11, 15 of every step, so pend < 16, and what is left — low, the
      // buffered unit, the outstanding 0xFFFF units, the chain wave's range — is the state.  Behind the LAST barrier (in place,
      // see where the state is loaded): nothing reads coder_in any more but quad_piece_pass, this lane, its own substream.
      __syncthreads();
      const CtxPieces &cp = quad_pack_first(sets...);
      const bool fin = (d.init_id & CABAC_SUB_FINISH) != 0;
      const uint32_t n_bits = live ? quad_enc_finish(e, (d.init_id & CABAC_SUB_ALIGN_RBSP) != 0, writer, !fin) : 0u;
      if (writer) {
        const uint32_t ends = fin ? e.pos : e.pos + 2u * (uint32_t)e.nbuf;
        cabac_substream_result res;
        res.n_bits = n_bits;
        res.flags = (ends > e.cap ? CABAC_RES_OVERFLOW : 0u) | (((bad_rows[unit] >> row) & 1u) ? CABAC_RES_BAD_RECORD : 0u);
        results[sub] = res;
        if (fin) quad_piece_store(cp, sub, CABAC_CODER_CLOSED, res.flags, n_bits, e.pos, 0u, 0u, 0u, 0u);
        else quad_piece_store(cp, sub, CABAC_CODER_ENC, res.flags, n_bits, e.pos, (uint32_t)e.low, fin_range[local] | ((uint32_t)e.pend << 16),
                              e.buf, (uint32_t)e.nbuf);
      }
      quad_piece_pass(results, sub, sub < n_sub && in_range && j == 0, piece, cp);
      return;
    }
    const uint32_t n_bits = live ? quad_enc_finish(e, (d.init_id & CABAC_SUB_ALIGN_RBSP) != 0, writer, (d.init_id & CABAC_SUB_PROBE) != 0) : 0u;
    if (writer) {
      cabac_substream_result res;
      res.n_bits = n_bits;
      res.flags = (e.pos > e.cap ? CABAC_RES_OVERFLOW : 0u) | (((bad_rows[unit] >> row) & 1u) ? CABAC_RES_BAD_RECORD : 0u);
      results[sub] = res;
    }
    if constexpr (kSets) quad_bad_set_result(results, sub, in_range && j == 0, su);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// decode

struct QuadDec {   // row-uniform values
  uint32_t hi, lo;   // 64-bit window: value in [62:47] (see v2)
  uint32_t used;     // bits shifted out of the window since the last top-up (the look-ahead below the value is 47 - used)
  uint32_t range;
  uint32_t npos;     // bit cursor, complemented: ~pos, pos = the substream bits moved into the window so far (bits 5..10 of
                     // ~pos are 63 - the ring dword that holds bit pos: the ring runs backwards, see below)
  uint32_t q_hi, q_lo;  // the two ring dwords from the one that holds bit `pos` (big-endian: first bit on top),
                     // fetched by the previous top-up
  uint32_t *ring;    // this row's input ring in LDS: 64 byte-swapped dwords, BACKWARDS — dword k of the substream at
                     // 64 - (k & 63), so that an ascending pair of LDS words is (q_lo, q_hi), a 64-bit register pair as it
                     // is read — and word 0 = a copy of word 64 (the pair that starts at dword 63 ends with dword 64 = 0)
  uint32_t filled;   // bytes of the substream staged into the ring so far (a multiple of 64)
  uint32_t pf_data, pf_off, pf_mask;  // a 64-byte block on its way: this lane's dword, its byte offset, wanted or not
  const uint8_t *src;
  uint32_t cap;
  const uint8_t *src_safe;  // src, or any readable address for an empty substream
  uint32_t last_dword;      // offset of the last dword that holds a byte of the substream
};

// Per-lane fields of one record for the decode chain.  A lane past the end of its substream carries the
// fields of "nothing" (c2 = 0, ep = 0, ctxm = 0): t = 0, value < range keeps the comparison false, and the
// step changes nothing.
struct QuadDecInfo {
  uint32_t c2;    // 2 * constant term of the LPS width: 8 context bin, 4 terminate bin, 0 bypass / none
  uint32_t ep;    // 1 for a bypass bin
  uint32_t srmul; // -2^(22 - ep) (as a signed 24-bit factor): the bypass doubling of value (arith_codec.cpp:100-105) is done by comparing against
                  // scaledRange / 2 and shifting afterwards, together with the renormalisation
  uint32_t ctxm;  // ~0 for a context-coded bin
  uint32_t ntrm;  // 0 for a terminate bin, ~0 otherwise            (kSpecial steps only)
  uint32_t alm;   // ~0 for an align() record                        (kSpecial steps only)
  uint32_t key;   // ctxId of a context bin; a value unique in the row otherwise (so that it matches no other lane)
};

// Input.  The substream is staged into an LDS ring in 64-byte blocks — one dword per lane, byte-swapped so that
// the first bit is on top — by quad_dec_stage_load / _store below (every 4th step, a block whenever fewer than
// 128 bytes are staged ahead of the cursor; 4 steps consume at most 48).
//
// Top-up, every fourth bin, without a question asked: the window is filled to all 63 bits below the sign bit
// (a look-ahead of 47).  The chain keeps no look-ahead count: all a top-up needs is `used`, the sum of the four
// shifts (tot) since the last one.  Four bins consume at most 24 bits, so used is 0..24 here, the missing `used`
// bits lie wholly in `lo`, and they are the top of the 32 stream bits at `pos` — cut out of (q_hi, q_lo), two
// ring dwords read by the PREVIOUS top-up, which also reads the two dwords for the next one: no global memory, no
// compare, no branch and no wait anywhere near the chain.  The cut is v_bfe_u32(next32, offset 32 - used, width
// used); both shift counts have an edge that the hardware takes modulo 32: pos & 31 == 0 (the 64-bit shift by 0
// leaves q_hi on top) and used == 0 (the offset 32 is read as 0, but v_bfe_u32 with a width of 0 returns 0
// whatever its offset; used <= 24 keeps the width inside the five bits the instruction reads, and the offset is
// then 8..31).  Reading ahead never changes a decision: a bit enters the comparison only
// when it reaches bit 54 of the window, and it is the same bit of the stream whenever it was appended (past the
// end of the substream: a zero, as the staging feeds them).
__device__ __forceinline__ void quad_dec_topup(QuadDec &w) {
  const uint64_t q = (((uint64_t)w.q_hi << 32) | w.q_lo) << (~w.npos & 31u);
  const uint32_t next32 = (uint32_t)(q >> 32);      // stream bits pos .. pos + 31
  const uint32_t want = w.used;                     // 0..24
  uint32_t add;                                     // next32 >> (32 - want), 0 for want == 0
  asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(add) : "v"(next32), "v"(32u - want), "v"(want));
  w.lo |= add;
  w.npos -= want;
  w.used = 0;
  const uint32_t *p = w.ring + ((w.npos >> 5) & 63u);  // 63 - dword: the second of the pair (dword 64 = dword 0 sits at 0)
  w.q_lo = p[0];
  w.q_hi = p[1];
}

// staging, part 1 (a step whose number is 0 mod 4): request the next block (one dword per lane of the substream: 64 bytes
// with 16 lanes, 16 with 4 — four steps of L bins consume at most 3 L bytes) if it is wanted
template <int L = 16>
__device__ __forceinline__ void quad_dec_stage_load(QuadDec &w, uint32_t j) {
  constexpr uint32_t kLanes = L > 16 ? 16u : (uint32_t)L;  // a block is at most 64 bytes (the ring holds 256)
  const uint32_t wanted = neg_mask(w.filled - (~w.npos >> 3) - 128u);  // fewer than 128 bytes ahead of the cursor (never behind it)
  w.pf_mask = L > 16 ? wanted & neg_mask(j - kLanes) : wanted;  // (with 64 lanes per substream the first 16 fetch)
  w.pf_off = w.filled + 4u * (j & (kLanes - 1u));
  w.pf_data = *reinterpret_cast<const uint32_t *>(w.src_safe + min(w.pf_off, w.last_dword));
  w.filled += (4u * kLanes) & wanted;
}
// part 2 (the step after): into the ring; past the end of the substream the window is fed zeros
__device__ __forceinline__ void quad_dec_stage_store(QuadDec &w) {
  const uint32_t v = __builtin_bswap32(w.pf_data) & neg_mask(w.pf_off - w.cap);
  const uint32_t at = (w.pf_off >> 2) & 63u;
  w.ring[sel(w.pf_mask, 64u - at, 65u)] = v;                            // word 65: nobody reads it
  w.ring[sel(w.pf_mask & neg_mask(at - 1u), 0u, 65u)] = v;              // at == 0: also the mirror
}

constexpr uint32_t kRingStride = 66;  // 64 ring dwords + the mirror of dword 0 + a dump word

// One decode step for the four rows.  Written with bit masks instead of ?: on purpose: on a lone wave
// every exec-mask region hipcc builds out of a conditional costs a VALU->SALU->EXEC round trip.  The cost
// of a step is its instruction count: a wave issues one instruction per ~4.4 cycles whether or not it
// depends on the previous one (tools/ubench_ilp.hip), so nothing is gained by shortening dependency
// chains and everything by dropping instructions.
// Per-lane state: st_v, the packed context word of the lane's own record (0 for a non-context record).
// Three variants of a step, chosen a step ahead (prepare() in the kernel):
//   pairs (kPairs, L = 16 only): no row has a context more than twice.  The chain does no context update at all: lane I
//     hands bin I the derived word of its state (QuadDecPair), and the states are brought up to date once behind the
//     chain, lane-parallel (quad_dec_steps_pairs).
//   generic: any repetition.  After each bin every lane applies it to its own copy of the state, and the lanes of the
//     row that hold the bin's ctxId keep the result — six instructions per bin of which all but the matching lanes'
//     are thrown away.
//   kSpecial: the generic one for steps whose 16 records contain a terminate or an align record (rare) — the other
//     two leave their handling out.
// The row-uniform fields of the 16 records of a step, one register per bin: the lanes compute them (lane I for bin I),
// park them in LDS and every lane reads its row's sixteen back with four 16-byte reads per field — an LDS read of one
// address by all lanes of a row IS the broadcast, and it replaces one v_mov_b32_dpp per bin and field (the consumers are
// VOP3 / VOPC / SDWA encodings that cannot take a DPP operand themselves).
template <int L = 16>
struct QuadDecRow {   // L = 64: the fields of sixteen bins at a time (quad_dec_steps fetches four times a step)
  static constexpr int kN = L > 16 ? 16 : L;
  uint32_t c2[kN], ctxm[kN], srmul[kN], ep[kN], key[kN];
  // fields: this wave's parking area, [5][64] words — c2, ctxm, key, srmul, ep of the lanes' records; at: the first lane
  __device__ __forceinline__ void fetch(const uint32_t *fields, uint32_t at) {
    auto one = [&](uint32_t which, uint32_t (&dst)[kN]) {
      const uint4 *p = reinterpret_cast<const uint4 *>(fields + which * 64u + at);
#pragma unroll
      for (int q = 0; q < kN / 4; q++) {
        const uint4 v = p[q];
        dst[4 * q] = v.x;
        dst[4 * q + 1] = v.y;
        dst[4 * q + 2] = v.z;
        dst[4 * q + 3] = v.w;
      }
    };
    one(0, c2);
    one(1, ctxm);
    one(2, key);
    one(3, srmul);
    one(4, ep);
  }
};

// What the pairs variant keeps per lane instead of a state that is updated bin by bin.  A context occurs at most twice
// in the row's step: the lane of a first (or only) occurrence hands the chain the derived word of the stored state; the
// lane of a second occurrence that of the state after ONE earlier bin — one of two candidates, both known before the
// chain starts, picked as soon as that earlier bin is in `bits` (row-uniform).
// Derived word: k | MPS << 31 — the 24-bit multiply-add of the LPS width reads k unmasked, and the MPS meets the sign of
// value - scaledRange in bit 31 with one exclusive or.
#ifndef CABAC_PAIR_PICK
#define CABAC_PAIR_PICK 4     // experiments only: 1, 2 — other cadences; 0 — the choice is made, the variant never taken
#endif
constexpr int kPairPick = CABAC_PAIR_PICK;  // the pick runs behind bins kPairPick - 1, 2 kPairPick - 1, ...: the two occurrences of a
                                            // context then must not share an aligned group of kPairPick bins (1: no such condition)
constexpr int kPairEvery = kPairPick > 0 ? kPairPick : 1;
struct QuadDecPair {
  uint32_t d;       // the derived word this lane hands to the chain (settled before the lane's bin is reached)
  uint32_t d0, d1;  // ... after the earlier occurrence decoded 0 / 1 (a first occurrence: twice that of the stored state)
  uint32_t p1;      // position of the context's first occurrence in the step
};
__device__ __forceinline__ uint32_t quad_dec_derived(uint32_t st) {  // state() / getLPS, contexts.cpp:939-950
  const uint32_t sum = (st & 0xffffu) + (st >> 16);
  const uint32_t sx = (uint32_t)((int32_t)(sum << 16) >> 31);
  return (((sum >> 10) ^ sx) & 31u) | (sx & 0x80000000u);
}

template <int I, bool kSpecial, int L = 16, bool kPairs = false>
__device__ __forceinline__ void quad_dec_step(const QuadDecInfo &f, const QuadDecRow<L> &u, uint32_t r0_v, uint32_t a_v, uint32_t &st_v,
                                              uint32_t (&bits)[2], QuadDec &w, QuadDecPair *pr = nullptr) {
  constexpr int J = I % QuadDecRow<L>::kN;  // where bin I's fields sit in u
  if constexpr (kPairs) {
    static_assert(L == 16 && !kSpecial, "the pairs variant is the quad decoder's, without special records");
    const uint32_t dw = group_bcast<L, I>(pr->d);
    const uint32_t t = (__umul24(w.range >> 5, dw) + u.c2[J]) >> 1;  // (the multiplication reads bits 23..0: k)
    const uint32_t rm = w.range - t;
    uint32_t e, ngem;  // as below
    asm("v_mad_i32_i24 %0, %2, %3, %4\n\tv_ashrrev_i32 %1, 31, %0" : "=v"(e), "=v"(ngem) : "v"(rm), "v"(u.srmul[J]), "v"(w.hi));
    const uint32_t x = sel(u.ctxm[J] & ~ngem, t, rm);
    const uint32_t nsh = (uint32_t)__builtin_clz(x) - 23u;
    w.hi = sel(ngem, w.hi, e);
    w.range = x << nsh;
    const uint32_t tot = nsh + u.ep[J];
    const uint64_t v = (((uint64_t)w.hi << 32) | w.lo) << tot;
    w.hi = (uint32_t)(v >> 32);
    w.lo = (uint32_t)v;
    w.used += tot;
    // The bin as 0 / 1 is needed by no update here, so it is never formed: bit 31 of e ^ dw is (LPS taken) ^ MPS = NOT the bin,
    // and one v_alignbit_b32 shifts it into bits[0] from below — the bins run the other way, inverted, and after bin I the
    // bin of position p sits at bit I - p; behind bin 15 they are turned into the usual order (bit I = bin I).
    bits[0] = __builtin_amdgcn_alignbit(bits[0], e ^ dw, 31);
    if constexpr (I % kPairEvery == kPairEvery - 1 && I != 15) {
      // every lane, a second occurrence or not: NOT bin p1 as a mask (some other bit where p1 is yet to come — those lanes
      // pick again before their bin is reached)
      uint32_t pm;
      asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(pm) : "v"(bits[0]), "v"((uint32_t)I - pr->p1));
      pr->d = sel(pm, pr->d0, pr->d1);
    }
    if constexpr (I == 15) bits[0] = ~__builtin_bitreverse32(bits[0]) >> 16;
    if ((I & 3) == 0) quad_dec_topup(w);
    return;
  }
  // the state of this bin's context, from the lane that holds the record; state() / getLPS, contexts.cpp:939-950
  uint32_t sum;  // the two estimators added: the low half carries no rate bits here (see the kernel)
  if constexpr (L == 64) {
    // one substream per wave: the state crosses as a scalar and is consumed by the SDWA add at once; its result is a vector
    // register, so that the chain stays the vector code of the other geometries (hipcc makes scalar code of a uniform chain,
    // and that is longer: 157 instructions per four bins against 145)
    const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)st_v, I);
    asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "=v"(sum) : "s"(st));
  } else {
    const uint32_t st = group_bcast<L, I>(st_v);
    sum = (st & 0xffffu) + (st >> 16);
  }
  const uint32_t sx = (uint32_t)((int32_t)(sum << 16) >> 31);  // 0 / ~0 from the MPS bit (bit 15)
  const uint32_t k = ((sum >> 10) ^ sx) & 31u;
  const uint32_t t = (__umul24(w.range >> 5, k) + u.c2[J]) >> 1;
  const uint32_t rm = w.range - t;
  // scaledRange at the window's scale is 2^22 (2^21 for a bypass bin) * rm.  (Round 1 had the scale as a DPP operand of a
  // multiplication, because v_lshlrev_b32 with DPP on its shift-amount operand returned wrong results on gfx950 — bisected
  // with the parity tests.)
  // value - scaledRange in ONE instruction: the record's field is MINUS the scale, a signed 24-bit factor (v_mad_i32_i24)
  // 0: value >= scaledRange (LPS / bin 1), ~0: MPS / bin 0.  Through asm so that hipcc sees an opaque mask: written
  // as (int)e >> 31 it turns every use back into v_cmp + v_cndmask pairs, two instructions where a v_bfi /
  // v_bitop3 on the mask is one.
  // (Both in ONE statement: hipcc pads every asm statement whose result the next instruction reads with an s_nop,
  // an issue slot like any other, and the shift reads the difference at once.)
  uint32_t e, ngem;
  asm("v_mad_i32_i24 %0, %2, %3, %4\n\tv_ashrrev_i32 %1, 31, %0" : "=v"(e), "=v"(ngem) : "v"(rm), "v"(u.srmul[J]), "v"(w.hi));
  const uint32_t bin = ~(ngem ^ sx) & 1u;                        // LPS ? !mps : mps; sx is the MPS as a mask (0 if st == 0)
  const uint32_t gc = u.ctxm[J] & ~ngem;
  // One renormalisation rule for both paths: the chosen sub-range shifted up to [256, 511].  LPS (context bins only):
  // clz(t) - 23 is getRenormBitsLPS.  Otherwise rm >= 128 (an LPS width is at most 15.5 / 32 of the range plus 4), so
  // clz(rm) - 23 is 1 iff rm < 256 — the one-bit MPS renormalisation (arith_codec.cpp:60-73) — and 0 for a bypass bin
  // (rm = range) and for the no-op steps past the end.
  const uint32_t x = sel(gc, t, rm);
  uint32_t nsh = (uint32_t)__builtin_clz(x) - 23u;
  uint32_t keep = ngem;
  if (kSpecial) {
    keep |= ~group_bcast<L, I>(f.ntrm);                               // terminate bin 1 leaves value untouched (:184-185)
    nsh &= ngem | group_bcast<L, I>(f.ntrm);                          // ... and does not renormalise
  }
  w.hi = sel(keep, w.hi, e);
  w.range = x << nsh;
  if (kSpecial) {
    w.range = sel(group_bcast<L, I>(f.alm), 256u, w.range);
    // After a terminate bin 1 nothing but finish() follows; keep range >= 256 so that the no-op steps past the
    // end of the substream (t = 0, rm = range) never look like a renormalising MPS step.
    w.range |= 256u & ~(ngem | group_bcast<L, I>(f.ntrm));
  }
  {
    // (as DPP operands of their VOP2 consumers srmul and ep would cost no move, but hipcc then pads every such consumer
    // with s_nops — it applies the DPP read-after-write hazard to all of its operands: 122 s_nops per step against 38)
    const uint32_t tot = nsh + u.ep[J];  // the renormalisation shift and the bypass bit
    const uint64_t v = (((uint64_t)w.hi << 32) | w.lo) << tot;
    w.hi = (uint32_t)(v >> 32);
    w.lo = (uint32_t)v;
    w.used += tot;
  }
  bits[I >> 5] |= bin << (I & 31);
  if constexpr (L == 64) asm volatile("" : "+v"(bits[I >> 5]));  // now: left to itself hipcc keeps all 64 shifted bins and ORs them at the end
  // (generic and special steps) every lane applies the bin to its own copy of the state; the lanes of this row that hold
  // the same ctxId keep it (update(), contexts.cpp:903-913).
  // Both 15-bit estimators at once with packed 16-bit math: the halves never borrow or carry into each
  // other, and the rate bits below bit 5 ride along untouched.
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 st2 = __builtin_bit_cast(u16x2, st_v);
  const u16x2 dlt2 = (st2 >> __builtin_bit_cast(u16x2, r0_v)) & __builtin_bit_cast(u16x2, (kMask1 << 16) | kMask0);
  const uint32_t rest = __builtin_bit_cast(uint32_t, (u16x2)(st2 - dlt2));
  uint32_t upd;  // both halves: rest + a * bin, the low half of `bin` feeding both lanes of the packed mad (op_sel_hi)
  // The update and its selection in one volatile statement (the padding again), which also keeps them unconditional:
  // hipcc would otherwise wrap the update in an exec region (SALU round trip + branch per bin).
  const uint64_t same = __builtin_amdgcn_uicmp(f.key, u.key[J], 32);  // 32: equal
  asm volatile("v_pk_mad_u16 %1, %2, %3, %4 op_sel_hi:[1,0,1]\n\tv_cndmask_b32_e64 %0, %0, %1, %5"
               : "+v"(st_v), "=v"(upd) : "v"(a_v), "v"(bin), "v"(rest), "s"(same));
  if ((I & 3) == 0) quad_dec_topup(w);  // every 4th bin (4 bins consume at most 24 bits)
}

template <bool kSpecial, int L = 16>
__device__ __forceinline__ void quad_dec_steps(const QuadDecInfo &f, QuadDecRow<L> &u, const uint32_t *fields, uint32_t r0_v, uint32_t a_v,
                                               uint32_t &st_v, uint32_t (&bits)[2], QuadDec &w) {
#define QSTEP(U, I) quad_dec_step<I, kSpecial, L>(f, U, r0_v, a_v, st_v, bits, w)
#define QSTEP16(U, B)                                                                                                     \
  QSTEP(U, B + 0); QSTEP(U, B + 1); QSTEP(U, B + 2); QSTEP(U, B + 3); QSTEP(U, B + 4); QSTEP(U, B + 5); QSTEP(U, B + 6);   \
  QSTEP(U, B + 7); QSTEP(U, B + 8); QSTEP(U, B + 9); QSTEP(U, B + 10); QSTEP(U, B + 11); QSTEP(U, B + 12); QSTEP(U, B + 13); \
  QSTEP(U, B + 14); QSTEP(U, B + 15)
  if constexpr (L == 64) {
    // sixty-four bins of ONE substream, the fields of sixteen at a time (a second set of eighty registers to fetch the next
    // sixteen under the chain does not fit: 256 vector registers are addressable, the rest is reached through moves)
    QSTEP16(u, 0);
    u.fetch(fields, 16u);
    QSTEP16(u, 16);
    u.fetch(fields, 32u);
    QSTEP16(u, 32);
    u.fetch(fields, 48u);
    QSTEP16(u, 48);
  } else if constexpr (L == 16) {
    QSTEP16(u, 0);
  } else {
    QSTEP(u, 0); QSTEP(u, 1); QSTEP(u, 2); QSTEP(u, 3);
  }
#undef QSTEP16
#undef QSTEP
}

// The pairs variant of a 16-bin step (L = 16).  same: the lanes of this lane's row that hold its context (bit k: lane k of
// the row; itself included; 0 for a lane without a context) — at most two, and no two inside an aligned group of kPairPick
// bins, which is what prepare() chose the variant by.  In front of the chain every lane forms the two states its context
// can have after one bin and the derived words; behind it every lane of a context computes the same final state — the
// stored one updated by the first occurrence's bin, then by the second's if there is one — with the packed 16-bit update
// of the generic step, so that the store that follows stays the unconditional one it is.
__device__ __forceinline__ void quad_dec_steps_pairs(const QuadDecInfo &f, const QuadDecRow<16> &u, uint32_t r0_v, uint32_t a_v, uint32_t same,
                                                     uint32_t j, uint32_t &st_v, uint32_t (&bits)[2], QuadDec &w) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 r2 = __builtin_bit_cast(u16x2, r0_v), a2 = __builtin_bit_cast(u16x2, a_v);
  const u16x2 mask2 = __builtin_bit_cast(u16x2, (kMask1 << 16) | kMask0);
  auto decayed = [&](uint32_t s) {  // update(), contexts.cpp:903-913, by a bin 0; a bin 1 adds a2 to it
    const u16x2 s2 = __builtin_bit_cast(u16x2, s);
    return (u16x2)(s2 - ((s2 >> r2) & mask2));
  };
  const u16x2 rest = decayed(st_v);
  const uint32_t u0 = __builtin_bit_cast(uint32_t, rest), u1 = __builtin_bit_cast(uint32_t, (u16x2)(rest + a2));
  const uint32_t secondm = neg_mask(0u - (same & ((1u << j) - 1u)));  // ~0: an earlier lane of the row holds this context
  QuadDecPair pr;
  pr.p1 = (uint32_t)__builtin_ctz(same | 0x10000u);
  pr.d0 = quad_dec_derived(sel(secondm, u0, st_v));
  pr.d1 = quad_dec_derived(sel(secondm, u1, st_v));
  pr.d = pr.d0;
#define QSTEP(I) quad_dec_step<I, false, 16, true>(f, u, r0_v, a_v, st_v, bits, w, &pr)
  QSTEP(0); QSTEP(1); QSTEP(2); QSTEP(3); QSTEP(4); QSTEP(5); QSTEP(6); QSTEP(7);
  QSTEP(8); QSTEP(9); QSTEP(10); QSTEP(11); QSTEP(12); QSTEP(13); QSTEP(14); QSTEP(15);
#undef QSTEP
  uint32_t m1;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m1) : "v"(bits[0]), "v"(pr.p1));
  const uint32_t s1 = sel(m1, u1, u0);
  const uint32_t later = same & (same - 1u);                          // the second occurrence, if there is one
  uint32_t m2;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m2) : "v"(bits[0]), "v"((uint32_t)__builtin_ctz(later | 0x10000u)));
  const uint32_t s2 = __builtin_bit_cast(uint32_t, (u16x2)(decayed(s1) + __builtin_bit_cast(u16x2, a_v & m2)));
  st_v = sel(neg_mask(0u - later), s2, s1);
}

// W independent waves per workgroup: with W = 4 a workgroup's waves are dealt to the CU's four SIMDs, which
// pins "one chain wave per SIMD" instead of leaving it to where the dispatcher happens to put
// single-wave workgroups (measured: the same decode kernel ran 2.06 ms or 3.3 ms depending on the geometry
// of the kernel launched before it).
// L lanes per substream, 64 / L substreams per wave, L bins per step.  L = 16 is the quad decoder; L = 4 ("hex": sixteen
// substreams per wave, the state of bin I of a step broadcast inside its quad of lanes by a DPP quad permutation) trades a
// longer chain per bin — the per-step work is spread over 4 bins instead of 16 — for four times the substreams per
// instruction: the geometry for batches that offer more than one quad wave per SIMD (launch_decode_v4).
// select (may be null): the launch runs only if *select == want — the dispatch launches both geometries behind
// decode_select_kernel, which looks at the batch on the device (the descriptors of a *_device call are not on the host).
template <int W, int L = 16, class... Sets>
__global__ __launch_bounds__(64 * W) void decode_kernel_v4(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                           const uint16_t *__restrict__ records,
                                                           const uint8_t *__restrict__ bytes, uint8_t *__restrict__ bins,
                                                           cabac_substream_result *__restrict__ results,
                                                           const uint32_t *__restrict__ select, uint32_t want, Sets... sets) {
  constexpr bool kSets = sizeof...(Sets) != 0;
  if (select != nullptr && *select != want) return;
  // decode keeps the two window sizes of a context (they never change) apart from its state word, whose low
  // five bits are then zero: state() is one SDWA add of the two halves, without masking
  constexpr uint32_t kSubs = 64u / L;  // substreams per wave
  __shared__ uint32_t ctx_all[W * kSubs * kQuadCtxStride];
  // what a record id means for the chain, looked up instead of computed (one 32-byte entry per id, the same for every
  // substream: the window sizes of a context do not depend on QP or slice type): {c2, srmul, ctxm, ep | r0_v, a_v, ntrm, alm}
  __shared__ __attribute__((aligned(16))) uint32_t rec_tab[512][8];
  __shared__ uint32_t ring_all[W * kSubs * kRingStride];
  __shared__ uint32_t field_all[W][5][64];  // the record fields of a step on their way from lane I to the row (QuadDecRow)
  // L = 16: which lanes of a row hold which context, 16 bits per row and context, two rows per word (the bitmap of the v7
  // encoder's context waves, quad_resolve; only contexts take part, so 384 words per pair of rows; all zero between uses)
  constexpr uint32_t kPairWords = L == 16 ? 768u : 1u;
  __shared__ uint32_t pair_all[W][kPairWords];
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t *ctx = ctx_all + wave * (kSubs * kQuadCtxStride);
  const uint32_t lane = threadIdx.x & 63u, row = lane / L, j = lane % L;
  const uint32_t sub = (blockIdx.x * W + wave) * kSubs + row;
  constexpr bool kPieces = kQuadPieces<Sets...>;  // cabac_hip_pieces.h: the coder state comes from and goes to memory
  static_assert(!kPieces || L == 16, "the pieces call is the quad decoder's");
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, sets...);
  bool live = sub < n_sub && !su.bad;
  const cabac_substream_desc d = desc[live ? sub : 0];
  // (pieces: the state is checked here, where it is loaded; a row that is refused or comes with flags codes nothing and
  // writes no set)
  QuadPieceUse pu{};
  QuadSetUse su_out = su;
  if constexpr (kPieces) {
    pu = quad_piece_use<false>(sub, sub < n_sub, su.bad, d.byte_capacity, sets...);
    live = live && pu.code;
    if (pu.refuse) su_out.out = kNoSet;
  }
  const uint32_t n = live ? d.n_records : 0u;
  const uint16_t *rec = records + d.rec_offset;
  uint8_t *out = bins + d.rec_offset;
  uint32_t *rctx = ctx + row * kQuadCtxStride;
  if constexpr (kSets) {
    quad_ctx_load<false>(rctx, d.qp, d.init_id & 3u, j, (uint32_t)L, su, sets...);
  } else {
    const int qp = d.qp < 0 ? 0 : (d.qp > 63 ? 63 : d.qp);
    const uint32_t iid = d.init_id & 3u;
    for (uint32_t k = j; k < (uint32_t)kNumCtx; k += L) {
      const uint32_t packed = ctx2_init(qp, c_init_tables[iid * kNumCtx + k], c_init_tables[3 * kNumCtx + k]);
      rctx[k] = packed & ~31u;
    }
  }
  for (uint32_t id = threadIdx.x; id < 512u; id += 64u * W) {
    const uint32_t ctxm = id < (uint32_t)kNumCtx ? ~0u : 0u;
    const uint32_t trm_m = id == CABAC_REC_TRM ? ~0u : 0u, aln_m = id == CABAC_REC_ALIGN ? ~0u : 0u;
    const uint32_t ep = id == CABAC_REC_EP ? 1u : 0u;
    uint32_t r0_v = 0, a_v = 0;
    if (ctxm) {
      const uint32_t rates = ctx2_init(0, c_init_tables[id], c_init_tables[3 * kNumCtx + id]) & 31u;
      const uint32_t r0 = (rates & 3u) + 2u, r1 = ((rates >> 2) & 7u) + 5u;
      a_v = ((0x7fffu >> r0) & kMask0) | (((0x7fffu >> r1) & kMask1) << 16);
      r0_v = r0 | (r1 << 16);  // packed shift amounts for the 2 x 16-bit update
    }
    rec_tab[id][0] = (8u & ctxm) | (4u & trm_m);  // 2 * constant term of the LPS width
    rec_tab[id][1] = 0u - (0x400000u >> ep);      // -2^(22 - ep), see quad_dec_step
    rec_tab[id][2] = ctxm;
    rec_tab[id][3] = ep;
    rec_tab[id][4] = r0_v;
    rec_tab[id][5] = a_v;
    rec_tab[id][6] = ~trm_m;
    rec_tab[id][7] = aln_m;
  }
  if constexpr (L == 16) {
    for (uint32_t k = threadIdx.x; k < W * kPairWords; k += 64u * W) (&pair_all[0][0])[k] = 0u;
  }
  __syncthreads();

  QuadDec w;
  w.src = bytes + d.byte_offset;
  w.cap = live ? d.byte_capacity : 0u;
  w.src_safe = w.cap != 0 ? w.src : reinterpret_cast<const uint8_t *>(desc);
  w.last_dword = w.cap != 0 ? ((w.cap - 1u) & ~3u) : 0u;
  {
    // start(), arith_codec.cpp:60-66.  Input is read as aligned dwords that contain at least one valid byte
    // (cabac_hip.h: the bytes buffer is readable up to the next multiple of 4 past every substream).
    const uint32_t first = __builtin_bswap32(w.cap ? *reinterpret_cast<const uint32_t *>(w.src) : 0u);
    w.hi = first >> 1;
    w.lo = first << 31;
  }
  // the first 192 bytes go into the ring at once (blocks of 4 L bytes); the window itself starts from bytes 0..7
  w.ring = ring_all + (wave * kSubs + row) * kRingStride;
  constexpr uint32_t kStageLanes = L > 16 ? 16u : (uint32_t)L;  // lanes that fetch a block (quad_dec_stage_load)
  for (uint32_t blk = 0; blk < 192u / (4u * kStageLanes); blk++) {
    w.filled = 4u * kStageLanes * blk;
    w.npos = ~0u;  // "wanted"
    quad_dec_stage_load<L>(w, j);
    w.pf_mask = L > 16 ? neg_mask(j - kStageLanes) : ~0u;
    quad_dec_stage_store(w);
  }
  w.filled = 192;
  w.pf_mask = 0;
  w.q_hi = w.ring[63];  // dwords 1 and 2
  w.q_lo = w.ring[62];
  w.lo |= w.q_hi >> 1;  // 63 bits: the value and a full look-ahead from bin 0 on (quad_dec_topup)
  w.used = 0;
  w.npos = ~63u;
  w.range = 510;
  if constexpr (kPieces) {
    // A row that continues: the state is range, the sixteen bits of the value and the shifts so far, S.  The look-ahead below the
    // value is raw stream and is read again: the window is rebuilt with the value on top and stream bits S + 16 .. S + 62 below
    // it, as a top-up leaves it (bit cursor S + 63), over the fresh start above, which a fresh row keeps (S = 0 restages the same
    // three blocks).  The ring is staged from the 64-byte block that holds bit S + 16.  Plain code: this runs once.
    // (A blend over the fresh start and two opaque reads, not a second prologue beside it: hipcc ends with "illegal VGPR to SGPR
    // copy" for this kernel when the fresh window's words have no use left or the pair of ring dwords is read as one.)
    const uint32_t resumed = pu.fresh ? 0u : ~0u;
    const uint32_t shifts0 = pu.bits;
    const uint32_t block0 = ((shifts0 + 16u) >> 3) & ~63u;
    for (uint32_t blk = 0; blk < 3u; blk++) {
      w.filled = block0 + 64u * blk;
      w.npos = ~0u;
      quad_dec_stage_load<L>(w, j);
      w.pf_mask = ~0u;
      quad_dec_stage_store(w);
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    w.filled = block0 + 192u;
    w.pf_mask = 0;
    auto stream32 = [&](uint32_t bit) {  // stream bits bit .. bit + 31 out of the ring (the pair of dwords as quad_dec_topup reads it)
      const uint32_t *p = w.ring + (63u - ((bit >> 5) & 63u));
      return (uint32_t)(((((uint64_t)p[1]) << 32) | p[0]) << (bit & 31u) >> 32);
    };
    w.hi = sel(resumed, (pu.value << 15) | (stream32(shifts0 + 16u) >> 17), w.hi);
    w.lo = sel(resumed, stream32(shifts0 + 31u), w.lo);
    w.npos = ~(shifts0 + 63u);
    const uint32_t *p = w.ring + ((w.npos >> 5) & 63u);
    uint32_t q_lo = p[0];
    asm volatile("" : "+v"(q_lo));
    uint32_t q_hi = p[1];
    asm volatile("" : "+v"(q_hi));
    w.q_lo = q_lo;
    w.q_hi = q_hi;
    w.range = pu.range;
  }
  uint32_t bad = 0;

  // Loop bound and loads without lane conditions: an exec region or a branch on a vector compare makes the
  // scalar unit wait for the vector result (~55 cycles each, per step).  The longest row's length is made
  // scalar once; loads past the end of a row read a valid address and are ignored (`active`).
  uint32_t n_wave = n;
#pragma unroll
  for (int d = L; d < 64; d <<= 1) n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, d));
  const uint32_t max_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_wave);
  const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
  const uint32_t last_rec = n != 0 ? n - 1u : 0u;
  // Records are requested four steps ahead (three in the rolled loop of L = 64).  What a step needs besides the bins — the
  // meaning of its record ids (rec_tab), the fields of the chain parked in LDS and read back per row (QuadDecRow), the choice
  // of the step variant, the context states — is prepared in two stages off the top of the step: the table rows are requested
  // at the START of the step before (they arrive during its chain), the rest at its END (the context store has just been
  // written back).
  auto load_rec = [&](uint32_t at) { return (uint32_t)rec_safe[min(at + j, last_rec)]; };
  // rq<k>: the record of the next step whose number is k mod 4 (L = 64: rq0..rq2 are the next three steps' and rotate)
  uint32_t rq0 = load_rec(0), rq1 = load_rec(L), rq2 = load_rec(2u * L), rq3 = L == 64 ? 0u : load_rec(3u * L);
  uint32_t prev_bin = 0, prev_idx = ~0u;  // the bins of the previous step, not yet stored
  uint64_t prev_lanes = 0;                 // ... and the lanes that have one
  // L = 16, the choice of the pairs variant: this lane's place in the bitmap, its own bit among the row's sixteen and the
  // other lanes of its aligned group of kPairPick (a context twice in there is too close for the pick's cadence)
  uint32_t *const pair_words = &pair_all[wave][(row >> 1) * 384u];
  const uint32_t pair_shift = (row & 1u) << 4, pair_own = 1u << (j & 15u);
  const uint32_t pair_near = ((((1u << kPairEvery) - 1u) << (j & 15u & ~(uint32_t)(kPairEvery - 1))) & ~pair_own) & 0xffffu;
  uint32_t cur_same = 0;
  uint64_t cur_generic = 0;  // lanes that rule the pairs variant out for the step
  uint32_t nxt_got = 0;       // the bitmap word of this lane's context, read a step ahead
  uint32_t nxt_id, nxt_actm;
  uint4 nxt_a, nxt_b;
  auto request = [&](uint32_t base, uint32_t r) {  // stage 1 for the step at `base`, whose record is r: its id and table row
    nxt_actm = neg_mask(base + j - n);                              // ~0: a record of this substream
    nxt_id = sel(nxt_actm, r & CABAC_REC_ID_MASK, 0x1f0u);         // past the end: an id that is nothing
    const uint4 *row4 = reinterpret_cast<const uint4 *>(rec_tab[nxt_id]);
    nxt_a = row4[0];
    nxt_b = row4[1];
    if constexpr (L == 16) {
      // the lanes of the row with this lane's context: every context lane ORs its bit into the word of (row, id), reads the
      // word back and clears it (one wave: LDS executes its instructions in order).  Lanes without a context — bypass,
      // terminate, align, "nothing" past the row's end — go to spare words, and prepare() leaves them no lane at all.
      // Asked here, a whole chain before prepare() reads the answer: at the end of the step it was a round trip waited for.
      uint32_t *word = pair_words + sel(neg_mask(nxt_id - (uint32_t)kNumCtx), nxt_id, (uint32_t)kNumCtx + (j & 3u));
      atomicOr(word, pair_own << pair_shift);
      asm volatile("" ::: "memory");
      nxt_got = *word;
      asm volatile("" ::: "memory");
      *word = 0u;
    }
  };
  uint32_t cur_id, cur_stored, cur_ctxm, cur_r0v, cur_av;
  uint64_t cur_special;
  QuadDecInfo f;
  QuadDecRow<L> u;
  auto prepare = [&]() {              // stage 2 for the step requested last
    const uint32_t id = nxt_id, ctxm = nxt_a.z;
    cur_id = id;
    cur_ctxm = ctxm;
    cur_r0v = nxt_b.x;
    cur_av = nxt_b.y;
    cur_stored = rctx[min(id, (uint32_t)kNumCtx)];                 // slot kNumCtx is the row's pad word
    f.c2 = nxt_a.x;
    f.srmul = nxt_a.y;
    f.ctxm = ctxm;
    f.ep = nxt_a.w;
    f.ntrm = nxt_b.z;
    f.alm = nxt_b.w;
    cur_special = __ballot((~f.ntrm | f.alm) != 0);
    if constexpr (L == 16) {
      cur_same = (nxt_got >> pair_shift) & 0xffffu & ctxm;   // the row's lanes with this lane's context (request())
      // pairs variant iff no lane has a special record, two other lanes with its context, or one too near
      const uint32_t others = cur_same & ~pair_own;
      cur_generic = __ballot(((~f.ntrm | f.alm) | (others & (others - 1u)) | (others & pair_near)) != 0);
    }
    bad |= nxt_actm & ~ctxm & neg_mask(id - CABAC_REC_ALIGN);
    f.key = sel(ctxm, id, 0x200u + j);
    // one wave writes and reads: LDS executes a wave's instructions in order, only the compiler has to keep it
    field_all[wave][0][lane] = f.c2;
    field_all[wave][1][lane] = f.ctxm;
    field_all[wave][2][lane] = f.key;
    field_all[wave][3][lane] = f.srmul;
    field_all[wave][4][lane] = f.ep;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    u.fetch(&field_all[wave][0][0], row * L);
  };
  request(0, rq0);
  if constexpr (L == 64) {
    rq0 = rq1;
    rq1 = rq2;
    rq2 = load_rec(3u * L);
  } else {
    rq0 = load_rec(4u * L);
  }
  prepare();
  // One step.  P = 0..3: its place in a trip of four steps (L = 16 and L = 4, whose input staging has period four: the
  // phases are then known where the step is written, the record register is the place's own and everything a step hands to
  // the next is a plain value; only the trip's back-edge carries registers).  P = -1: the rolled loop of L = 64, which
  // stages in every step.  rq: the register that holds the NEXT step's record; it is refilled for the step four on.
  auto step = [&](uint32_t base, auto place, uint32_t &rq) __attribute__((always_inline)) {
    constexpr int P = decltype(place)::value;
    V5_TICK(t0);
    V5_TICK(t1);
    // The bins of the previous step are stored only now, after the wait at the end of that step: loads and stores share
    // one in-order counter, so a store issued before a wait would add its whole latency to it (the same goes for the
    // input block requested a step ago: into the ring with it before anything new is issued)
    // (L = 64: a step consumes up to 48 bytes, so a 64-byte block is requested in EVERY step and stored in the next)
    if (P < 0 ? base != 0u : P == 1) quad_dec_stage_store(w);     // steps 1, 5, 9, ...
    {  // under the lane mask asked for at the end of the step before: an `if` here is a compare the scalar unit waits for
      uint64_t saved;
      asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tglobal_store_byte %2, %3, off\n\ts_mov_b64 exec, %0"
                   : "=&s"(saved) : "s"(prev_lanes), "v"(out + min(prev_idx, last_rec)), "v"(prev_bin) : "memory");
    }
    if (P <= 0) quad_dec_stage_load<L>(w, j);    // steps 0, 4, 8, ...: request a block of input
    const uint32_t id = cur_id, ctxm = cur_ctxm;
    // asked long ago, needed now (the choice of the step variant): the branch finds the answer waiting
    uint64_t special = cur_special;
    asm volatile("" : "+s"(special));
    uint64_t generic = cur_generic;
    const uint32_t same = cur_same;
    if constexpr (L == 16) asm volatile("" : "+s"(generic));
    uint32_t st_v = cur_stored & ctxm;
    const uint32_t a_v = cur_av, r0_v = cur_r0v;
    request(base + L, rq);                              // the id and table row of the next step
    if constexpr (P < 0) {
      rq0 = rq1;
      rq1 = rq2;
      rq2 = load_rec(base + 4u * L);
    } else {
      rq = load_rec(base + 5u * L);
    }
    uint32_t bits[2] = {0u, 0u};  // row-uniform: bit I = the bin of record base + I
    V5_TICK(t2);
    if constexpr (L == 16) {
      // one branch on the expected path: pairs or not; from the other side on as before
      if (kPairPick > 0 && __builtin_expect(generic == 0, 1)) quad_dec_steps_pairs(f, u, r0_v, a_v, same, j, st_v, bits, w);
      else if (__builtin_expect(special == 0, 1)) quad_dec_steps<false, L>(f, u, &field_all[wave][0][0], r0_v, a_v, st_v, bits, w);
      else quad_dec_steps<true, L>(f, u, &field_all[wave][0][0], r0_v, a_v, st_v, bits, w);
    } else {
      if (__builtin_expect(special == 0, 1)) quad_dec_steps<false, L>(f, u, &field_all[wave][0][0], r0_v, a_v, st_v, bits, w);
      else quad_dec_steps<true, L>(f, u, &field_all[wave][0][0], r0_v, a_v, st_v, bits, w);
    }
    V5_TICK(t3);
    const uint32_t my_bin = ((L > 32 && j >= 32u ? bits[1] : bits[0]) >> (j & 31u)) & 1u;
    rctx[sel(ctxm, id, (uint32_t)kNumCtx)] = st_v;  // a lane without a context writes the pad word
    prev_bin = my_bin;
    prev_idx = base + j;
    prev_lanes = __ballot(prev_idx < n);
    prepare();                                      // the next step's context states and record fields
    V5_TICK(t4);
    if (wave == 0) {
      V5_ADD(8, t0, t1);   // waiting for the record
      V5_ADD(9, t1, t2);   // prologue
      V5_ADD(10, t2, t3);  // 16 chain steps incl. top-ups
      V5_ADD(11, t3, t4);  // epilogue
    }
  };
  if constexpr (L == 64) {
    for (uint32_t base = 0; base < max_n; base += L) step(base, std::integral_constant<int, -1>{}, rq0);
  } else {
    // ceil(max_n / 4L) trips: the surplus steps of the last one are the no-op steps that the shorter rows of a wave run
    // anyway — the id of "nothing", t = 0, tot = 0, no bin stored (prev_lanes), no record counted bad (nxt_actm); a top-up
    // after them appends nothing (want = 0), and they sit at places 1..3, which request no input: shifts, bytes_read and
    // the flags below do not depend on how many of them ran.
    for (uint32_t base = 0; base < max_n; base += 4u * L) {
      step(base, std::integral_constant<int, 0>{}, rq1);
      step(base + L, std::integral_constant<int, 1>{}, rq2);
      step(base + 2u * L, std::integral_constant<int, 2>{}, rq3);
      step(base + 3u * L, std::integral_constant<int, 3>{}, rq0);
    }
  }
  if (prev_idx < n) out[prev_idx] = (uint8_t)prev_bin;

  // bits shifted so far: everything moved into the window minus value (16) minus look-ahead (47 at the last top-up, less
  // what the bins of the incomplete group since then have used)
  const uint32_t shifts = ~w.npos - 63u + w.used;
  const uint32_t bytes_read = 2u + (shifts >> 3);  // the reference's counters (arith_codec.cpp:257-260)
  const int32_t bits_needed = (int32_t)(shifts & 7u) - 8;
  uint32_t flags = 0;
  if (live && (d.init_id & CABAC_SUB_FINISH)) {
    uint32_t ok = 0;
    if (bytes_read <= w.cap) {
      const uint32_t last = w.src[bytes_read - 1];
      ok = ((last << (8 + bits_needed)) & 0xffu) == 0x80u;
    }
    if (!ok && bytes_read <= w.cap) flags |= CABAC_RES_BAD_STOP;  // an underrun throws before finish() is reached
  }
  if (bytes_read > w.cap) flags |= CABAC_RES_UNDERRUN;
  const uint64_t bad_mask = __ballot(bad != 0);
  if ((bad_mask >> (row * L)) & (L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull)) flags |= CABAC_RES_BAD_RECORD;
  if (live && j == 0) {
    cabac_substream_result res;
    res.n_bits = 8u * bytes_read + (uint32_t)bits_needed;
    res.flags = flags;
    results[sub] = res;
  }
  if constexpr (kPieces) {
    // the state behind the piece: the value field of the window (bits 62..47), range and the shifts; behind a terminate bin 1 the
    // value stands at or above the scaled range (quad_dec_step: it is left untouched, and range may have been raised to 511)
    const CtxPieces &cp = quad_pack_first(sets...);
    if (live && j == 0) {
      const uint32_t value = (w.hi >> 15) & 0xffffu;
      const uint32_t mark = (value >= (w.range << 7) || w.range > 510u) ? 1u : 0u;
      if (d.init_id & CABAC_SUB_FINISH) quad_piece_store(cp, sub, CABAC_CODER_CLOSED, flags, shifts, 0u, 0u, 0u, 0u, 0u);
      else quad_piece_store(cp, sub, CABAC_CODER_DEC, flags, shifts, 0u, w.range, value, mark, 0u);
    }
    quad_piece_pass(results, sub, sub < n_sub && j == 0, pu, cp);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    quad_ctx_export(rctx, j, (uint32_t)L, su_out, sets...);
    return;
  }
  if constexpr (kSets) {
    // Every step ends with the store of its final states (all lanes of a context hold the same word, after a pairs step too:
    // quad_dec_steps_pairs brings st_v up to date behind its chain), and the surplus steps of the last trip and of shorter rows
    // carry the id of "nothing": they write the pad word.  The row's lanes belong to one wave, whose LDS instructions execute in
    // order: only the compiler has to be kept from moving the reads.
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    quad_ctx_export(rctx, j, (uint32_t)L, su, sets...);
    quad_bad_set_result(results, sub, j == 0, su);
  }
}

// ---------------------------------------------------------------------------------------------
// bit estimator: BitEstimator_Std, arith_codec.cpp:603-711
//
// The cost of a bin string in 1/32768 bit: a context bin costs m_binFracBits[state][bin] and updates its
// context (estFracBitsUpdate, contexts.cpp:922-925), a bypass bin 1 bit, a terminate bin a constant, and
// align() rounds the running total up to a whole bit.  There is no low / range recurrence: the only serial
// part is the context state each bin sees, which quad_resolve gives for 16 bins of four substreams at once.
// Every lane adds up its own bins; the sixteen partial sums of a row meet at the end — and at an align
// record, which needs the running total in order (rare: that step is then summed serially).
static __constant__ uint32_t c_frac_bits[512] = {CABAC_FRAC_BITS_TABLE_VALUES};

__device__ __forceinline__ uint64_t row_sum64(uint64_t v) {  // sum over the 16 lanes of a row, in every lane
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// The probe form (cabac_hip_probe.h) is the same walk with a trailing ProbeList — a parameter pack that is empty for the plain
// calls, whose signature, arguments and code are then the ones from before the probes (as the sets of the codec kernels).  With
// it frac_bits is indexed by probe, not by substream: a step that holds a probe of one of its rows takes the ordered path of the
// align / reset / restart records, lane k keeps the running total behind record k, and the row's probes fetch theirs from there
// (quad_probe_drain).  The start sets are then the codec calls' (CABAC_CTX_NO_SET, an index >= n_sets: CABAC_RES_BAD_SET).
struct NoProbes {};
__device__ __forceinline__ NoProbes estimate_probes() { return NoProbes{}; }
__device__ __forceinline__ const ProbeList &estimate_probes(const ProbeList &pl) { return pl; }

template <int W, class... Probes>
__global__ __launch_bounds__(64 * W) void estimate_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                          const uint16_t *__restrict__ records,
                                                          uint64_t *__restrict__ frac_bits, uint32_t *__restrict__ flags,
                                                          const uint32_t *__restrict__ start_state,
                                                          const uint8_t *__restrict__ start_rate,
                                                          const uint32_t *__restrict__ start_set, Probes... probes) {
  constexpr bool kProbes = sizeof...(Probes) != 0;
  const auto pl = estimate_probes(probes...);
  __shared__ uint32_t ctx_all[W * kQuadSubs * kQuadCtxStride];
  __shared__ uint32_t frac[512];
  __shared__ uint32_t match_all[W][kMatchWords];   // same-id lanes through LDS (quad_resolve: 347 -> 291 ns per step alone)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = lane >> 4, j = lane & 15u;
  for (uint32_t k = threadIdx.x; k < W * kMatchWords; k += 64u * W) (&match_all[0][0])[k] = 0u;
  const uint32_t sub = (blockIdx.x * W + wave) * kQuadSubs + row;
  QuadSetUse su{kNoSet, kNoSet, false};
  CtxSets cs{};
  if constexpr (kProbes) {
    cs.n_sets = pl.n_sets;
    cs.state = start_state;
    cs.rate = start_rate;
    cs.start_set = start_set;
    su = quad_set_use(sub, sub < n_sub, cs);
  }
  const bool live = sub < n_sub && !su.bad;
  const cabac_substream_desc d = desc[live ? sub : 0];
  const uint32_t n = live ? d.n_records : 0u;
  const uint16_t *rec = records + d.rec_offset;
  uint32_t *rctx = ctx_all + (wave * kQuadSubs + row) * kQuadCtxStride;
  if constexpr (kProbes) {
    quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, cs);
  } else if (start_state == nullptr) {
    quad_ctx_init(rctx, d.qp, d.init_id & 3u, j);  // reset(qp, initId), arith_codec.cpp:623-626
  } else {
    // contexts assigned from another coder's (contexts.hpp:254): set start_set[sub] of the given states, in the
    // format of cabac_hip_ctx_init_device (m_state[0] | m_state[1] << 16, m_rate = 16 * rate0 + rate1)
    const uint64_t set = live ? start_set[sub] : 0u;
    for (uint32_t k = j; k < (uint32_t)kNumCtx; k += 16) {
      const uint32_t st = start_state[set * kNumCtx + k], rt = start_rate[set * kNumCtx + k];
      rctx[k] = (st & kMask0) | (st & 0xffff0000u) | (((rt >> 4) - 2u) & 3u) | ((((rt & 15u) - 5u) & 7u) << 2);
    }
  }
  for (uint32_t k = threadIdx.x; k < 512u; k += 64u * W) frac[k] = c_frac_bits[k];
  __syncthreads();

  uint32_t n_wave = n;
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 16));
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 32));
  const uint32_t max_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_wave);
  const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
  const uint32_t last_rec = n != 0 ? n - 1u : 0u;
  uint32_t next_rec = rec_safe[min(j, last_rec)];
  uint32_t bad = 0;
  uint64_t acc = 0;  // this lane's share of the row's total
  QuadProbeCursor pc{0u, 0u, 0xffffffffu, 0xffffffffu};
  if constexpr (kProbes) {
    pc = quad_probe_begin(pl, sub, sub < n_sub, n, lane);
    if (__ballot(pc.at == 0u) != 0) quad_probe_drain(pl, pc, n, 0u, (uint64_t)0, lane, frac_bits);  // in front of every record: 0
  }
  for (uint32_t base = 0; base < max_n; base += 16) {
    const uint32_t r = next_rec;
    next_rec = rec_safe[min(base + 16u + j, last_rec)];
    const QuadRecord q = quad_resolve<CABAC_REC_EST_RESTART, true>(r, base + j < n, lane, row, rctx, bad, match_all[wave]);
    const bool active = base + j < n;
    const bool zero = active && q.id == CABAC_REC_EST_RESETBITS, whole = active && q.id == CABAC_REC_EST_RESTART;
    uint32_t cost = 0;
    if (q.ctxm) cost = frac[2u * ctx2_q8(q.st) + q.bin];
    if (q.epm) cost = 1u << 15;                       // estFracBitsEP, contexts.cpp:880-882
    if (q.trmm) cost = q.bin ? 0x3bfbbu : 0x0010cu;    // estFracBitsTrm, contexts.cpp:931-933
    const uint32_t special = q.alnm ? 1u : zero ? 2u : whole ? 3u : 0u;  // records that need the total in order
    bool in_order = special != 0;
    if constexpr (kProbes) in_order = in_order || pc.at <= base + 16u;  // a probe of the row lies in this step: one ballot for both
    if (__builtin_expect(__ballot(in_order) != 0, 0)) {
      uint64_t total = row_sum64(acc);  // everything before this step
      uint64_t mine = 0;                // (probes) the running total behind this lane's record
      for (int k = 0; k < 16; k++) {
        total += (uint32_t)__shfl((int)cost, (int)(row * 16u + k));
        const int what = __shfl((int)special, (int)(row * 16u + k));
        if (what == 1) total = (total + 0x7fffull) & ~0x7fffull;  // align(), arith_codec.cpp:679-684
        if (what == 2) total = 0;                                   // resetBits() / start(), :615, :628
        if (what == 3) total &= ~0x7fffull;                         // restart(), :619-621
        if constexpr (kProbes) mine = (int)j == k ? total : mine;
      }
      acc = j == 0 ? total : 0ull;
      if constexpr (kProbes) quad_probe_drain(pl, pc, n, base + 16u, mine, lane, frac_bits);
    } else {
      acc += cost;
    }
  }
  const uint64_t total = row_sum64(acc);
  const uint64_t bad_mask = __ballot(bad != 0);
  if constexpr (kProbes) {  // every value has left through its probe; a substream with a bad set had its probes answered with 0
    if (sub < n_sub && j == 0 && flags)
      flags[sub] = su.bad ? 0x40u /* CABAC_RES_BAD_SET */ : (((bad_mask >> (row * 16u)) & 0xffffull) ? CABAC_RES_BAD_RECORD : 0u);
    return;
  }
  if (live && j == 0) {
    frac_bits[sub] = total;
    if (flags) flags[sub] = ((bad_mask >> (row * 16u)) & 0xffffull) ? CABAC_RES_BAD_RECORD : 0u;
  }
}

hipError_t launch_estimate_probes(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                  const ProbeList &probes, const uint32_t *start_state, const uint8_t *start_rate,
                                  const uint32_t *start_set, uint64_t *frac_bits, uint32_t *flags) {
  if (n_sub == 0) return hipSuccess;
  const uint32_t waves = (n_sub + kQuadSubs - 1) / kQuadSubs;
  if (waves >= 1024u)
    hipLaunchKernelGGL((estimate_kernel<4, ProbeList>), dim3((waves + 3) / 4), dim3(256), 0, st, n_sub, desc, records, frac_bits, flags,
                       start_state, start_rate, start_set, probes);
  else
    hipLaunchKernelGGL((estimate_kernel<1, ProbeList>), dim3(waves), dim3(64), 0, st, n_sub, desc, records, frac_bits, flags, start_state,
                       start_rate, start_set, probes);
  return hipGetLastError();
}

hipError_t launch_estimate(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                           uint64_t *frac_bits, uint32_t *flags, const uint32_t *start_state, const uint8_t *start_rate,
                           const uint32_t *start_set) {
  if (n_sub == 0) return hipSuccess;
  const uint32_t waves = (n_sub + kQuadSubs - 1) / kQuadSubs;
  // four-wave workgroups pin one wave per SIMD (see decode_kernel_v4); small batches spread single waves
  if (waves >= 1024u)
    hipLaunchKernelGGL(estimate_kernel<4>, dim3((waves + 3) / 4), dim3(256), 0, st, n_sub, desc, records, frac_bits, flags,
                       start_state, start_rate, start_set);
  else
    hipLaunchKernelGGL(estimate_kernel<1>, dim3(waves), dim3(64), 0, st, n_sub, desc, records, frac_bits, flags, start_state,
                       start_rate, start_set);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// context advance (cabac_hip_ctx_sets.h): the estimator's walk with the cost dropped and the export added — quad_resolve brings
// the row's store up to date for the sixteen records of a step, same-context repeats included; bypass, terminate and align
// records touch no context, any other id is a bad record.  Sets in, sets out; nothing is coded.
template <int W>
__global__ __launch_bounds__(64 * W) void ctx_advance_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                             const uint16_t *__restrict__ records, CtxSets cs,
                                                             uint32_t *__restrict__ flags) {
  __shared__ uint32_t ctx_all[W * kQuadSubs * kQuadCtxStride];
  __shared__ uint32_t match_all[W][kMatchWords];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = lane >> 4, j = lane & 15u;
  for (uint32_t k = threadIdx.x; k < W * kMatchWords; k += 64u * W) (&match_all[0][0])[k] = 0u;
  const uint32_t sub = (blockIdx.x * W + wave) * kQuadSubs + row;
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, cs);
  const bool live = sub < n_sub && !su.bad;
  const cabac_substream_desc d = desc[live ? sub : 0];
  const uint32_t n = live ? d.n_records : 0u;
  const uint16_t *rec = records + d.rec_offset;
  uint32_t *rctx = ctx_all + (wave * kQuadSubs + row) * kQuadCtxStride;
  quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, cs);
  __syncthreads();

  uint32_t n_wave = n;
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 16));
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 32));
  const uint32_t max_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_wave);
  const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
  const uint32_t last_rec = n != 0 ? n - 1u : 0u;
  uint32_t next_rec = rec_safe[min(j, last_rec)];
  uint32_t bad = 0;
  for (uint32_t base = 0; base < max_n; base += 16) {
    const uint32_t r = next_rec;
    next_rec = rec_safe[min(base + 16u + j, last_rec)];
    (void)quad_resolve<CABAC_REC_ALIGN, true>(r, base + j < n, lane, row, rctx, bad, match_all[wave]);
  }
  const uint64_t bad_mask = __ballot(bad != 0);
  asm volatile("" ::: "memory");  // the row's stores are its own wave's: in order in LDS
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  quad_ctx_export(rctx, j, 16u, su, cs);
  if (sub < n_sub && j == 0 && flags != nullptr)
    flags[sub] = su.bad ? 0x40u : (((bad_mask >> (row * 16u)) & 0xffffull) ? CABAC_RES_BAD_RECORD : 0u);
}

hipError_t launch_ctx_advance(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                              const CtxSets &sets, uint32_t *flags) {
  if (n_sub == 0) return hipSuccess;
  const uint32_t waves = (n_sub + kQuadSubs - 1) / kQuadSubs;
  if (waves >= 1024u) hipLaunchKernelGGL(ctx_advance_kernel<4>, dim3((waves + 3) / 4), dim3(256), 0, st, n_sub, desc, records, sets, flags);
  else hipLaunchKernelGGL(ctx_advance_kernel<1>, dim3(waves), dim3(64), 0, st, n_sub, desc, records, sets, flags);
  return hipGetLastError();
}

// One level of a WPP call (cabac_hip_ctx_sets.h), substreams [first, first + n): the descriptors of its prefix pass (the first
// min(sync_at, n_records) records, flag bits cleared), its slot indices (slot = substream) and its links checked against the
// level — a link that does not point below `first` becomes an index no call accepts (CABAC_RES_BAD_SET)
__global__ __launch_bounds__(256) void wpp_level_kernel(uint32_t first, uint32_t n, const cabac_substream_desc *__restrict__ desc,
                                                        const uint32_t *__restrict__ sync_from, const uint32_t *__restrict__ sync_at,
                                                        cabac_substream_desc *__restrict__ desc_out, uint32_t *__restrict__ start_out,
                                                        uint32_t *__restrict__ slot_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = first + i;
  cabac_substream_desc d = desc[s];
  d.n_records = min(sync_at[s], d.n_records);
  d.init_id &= 3u;
  desc_out[s] = d;
  const uint32_t from = sync_from[s];
  start_out[s] = (from == kNoSet || from < first) ? from : 0xfffffffeu;
  slot_out[s] = s;
}

hipError_t launch_wpp_level(hipStream_t st, uint32_t first, uint32_t n, const cabac_substream_desc *desc, const uint32_t *sync_from,
                            const uint32_t *sync_at, cabac_substream_desc *desc_out, uint32_t *start_out, uint32_t *slot_out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(wpp_level_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, first, n, desc, sync_from, sync_at, desc_out,
                     start_out, slot_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Each dispatch below is written once, over the pack: `sets` is one CtxSets (the instantiations that start from and write context
// sets) or nothing (the plain ones); the public functions call it with *sets or without.
template <class F>
static hipError_t with_sets(const CtxSets *sets, F dispatch) {
  return sets != nullptr ? dispatch(*sets) : dispatch();
}

hipError_t launch_encode_v4(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, const CtxSets *sets) {
  return with_sets(sets, [&](auto... s) {
    hipLaunchKernelGGL(encode_kernel_v4<decltype(s)...>, dim3((n_sub + kQuadSubs - 1) / kQuadSubs), dim3(64), 0, st, n_sub, desc, records,
                       bytes, results, s...);
    return hipGetLastError();
  });
}

// the pieces calls (cabac_hip_pieces.h): the coder state loaded, checked and stored by the same kernels.  The encoder in one of two
// geometries (cabac_hip_piece_encoder.h), same bytes, results, sets and states: variant 4 the in-wave one, 7 the lane-serial one
// with launch_encode_v7's rule for its two sizes (in_flight = 0)
hipError_t launch_encode_pieces(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                uint8_t *bytes, cabac_substream_result *results, const CtxPieces &pieces, int variant) {
  if (variant == 7) {
    if (n_sub >= 1024u)
      hipLaunchKernelGGL((encode_kernel_v7<4, CtxPieces>), dim3((n_sub + 15) / 16), dim3(448), 0, st, n_sub, desc, records, bytes, results,
                         pieces);
    else
      hipLaunchKernelGGL((encode_kernel_v7<1, CtxPieces>), dim3((n_sub + 3) / 4), dim3(256), 0, st, n_sub, desc, records, bytes, results,
                         pieces);
    return hipGetLastError();
  }
  if (variant != 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(encode_kernel_v4<CtxPieces>, dim3((n_sub + kQuadSubs - 1) / kQuadSubs), dim3(64), 0, st, n_sub, desc, records, bytes,
                     results, pieces);
  return hipGetLastError();
}

hipError_t launch_decode_pieces(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                const uint8_t *bytes, uint8_t *bins, cabac_substream_result *results, const CtxPieces &pieces) {
  hipLaunchKernelGGL((decode_kernel_v4<4, 16, CtxPieces>), dim3((n_sub + 15u) / 16u), dim3(256), 0, st, n_sub, desc, records, bytes, bins,
                     results, (const uint32_t *)nullptr, 0u, pieces);
  return hipGetLastError();
}

hipError_t launch_encode_v6(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, uint32_t in_flight, const CtxSets *sets) {
  const uint32_t units = (n_sub + kQuadSubs - 1) / kQuadSubs;
  const uint32_t units_on_chip = (max(n_sub, in_flight) + kQuadSubs - 1) / kQuadSubs;
  return with_sets(sets, [&](auto... s) {
    if (units_on_chip >= 1024u)
      hipLaunchKernelGGL((encode_kernel_v6<4, 1, decltype(s)...>), dim3((units + 3) / 4), dim3(1024), 0, st, n_sub, desc, records, bytes,
                         results, s...);
    else
      hipLaunchKernelGGL((encode_kernel_v6<1, 2, decltype(s)...>), dim3(units), dim3(256), 0, st, n_sub, desc, records, bytes, results, s...);
    return hipGetLastError();
  });
}

hipError_t launch_encode_v7(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, uint32_t in_flight, const CtxSets *sets) {
  return with_sets(sets, [&](auto... s) {
    // sixteen substreams per workgroup once there are enough of them to give every CU one; four below that
    if (max(n_sub, in_flight) >= 1024u)
      hipLaunchKernelGGL((encode_kernel_v7<4, decltype(s)...>), dim3((n_sub + 15) / 16), dim3(448), 0, st, n_sub, desc, records, bytes,
                         results, s...);
    else
      hipLaunchKernelGGL((encode_kernel_v7<1, decltype(s)...>), dim3((n_sub + 3) / 4), dim3(256), 0, st, n_sub, desc, records, bytes,
                         results, s...);
    return hipGetLastError();
  });
}

// How many substreams of the longest one's length the batch is worth: sum of n_records / max n_records.  The sixteen-per-wave
// geometry pays when the chip is offered more than two quad waves per SIMD of EQUAL work; a batch whose time is that of a
// few long substreams (BASELINE config C5: 4 096 long ones among 8 192) is better off with the shorter chain per bin of the
// quad decoder.  *select = 1: sixteen per wave, 0: four.
__global__ __launch_bounds__(1024) void decode_select_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                             uint32_t threshold, uint32_t *__restrict__ select) {
  __shared__ unsigned long long sum_w[16];
  __shared__ uint32_t max_w[16];
  unsigned long long sum = 0;
  uint32_t mx = 0;
  for (uint32_t s = threadIdx.x; s < n_sub; s += 1024u) {
    const uint32_t n = desc[s].n_records;
    sum += n;
    mx = max(mx, n);
  }
  for (int d = 1; d < 64; d <<= 1) {
    sum += __shfl_xor(sum, d);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
  }
  if ((threadIdx.x & 63u) == 0) {
    sum_w[threadIdx.x >> 6] = sum;
    max_w[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; k++) {
      sum += sum_w[k];
      mx = max(mx, max_w[k]);
    }
    *select = (mx != 0 && sum >= (unsigned long long)threshold * mx) ? 1u : 0u;
  }
}

// Between 1 024 and 3 072 substreams: is the batch's time that of at most 1 024 long substreams that come first (a share of a
// longest-first sharded batch: BASELINE config C5 on four GPUs is 1 024 long + 1 024 short ones)?  Then one substream per wave
// (*select = 2: the long ones get a SIMD each, the short ones pass through beside them), else four (0).  "Long": more than a
// sixteenth of the longest.  They must come first because workgroups are placed in order: two long waves on one SIMD would
// cost more than the geometry saves.
__global__ __launch_bounds__(1024) void decode_select_solo_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                                  uint32_t max_long, uint32_t *__restrict__ select) {
  __shared__ uint32_t red[16];
  __shared__ uint32_t longest;
  auto block_max = [&](uint32_t v) {
    for (int d = 1; d < 64; d <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t m = 0;
    for (int k = 0; k < 16; k++) m = max(m, red[k]);
    return m;
  };
  uint32_t mx = 0;
  for (uint32_t s = threadIdx.x; s < n_sub; s += 1024u) mx = max(mx, desc[s].n_records);
  mx = block_max(mx);
  if (threadIdx.x == 0) longest = mx;
  __syncthreads();
  const uint32_t cut = longest >> 4;
  uint32_t past = 0;  // 1 + the index of the last long substream
  for (uint32_t s = threadIdx.x; s < n_sub; s += 1024u)
    if (desc[s].n_records > cut) past = s + 1u;
  past = block_max(past);
  // all long ones among the first max_long: then there are at most max_long of them
  if (threadIdx.x == 0) *select = (longest != 0u && past <= max_long) ? 2u : 0u;
}

constexpr uint32_t kSoloUpTo = 1024;     // substreams in flight up to which each gets a wave (and a SIMD) of its own ...
constexpr uint32_t kSoloAskUpTo = 3072;  // ... and up to here the batch is looked at on the device (below the headline's 4 096)
constexpr uint32_t kHexFrom = 9216;  // measured (tools/batch_scaling.py): 8 192 equal substreams 2.12 ms quad / 2.23 ms hex, 12 288: 3.14 / 2.23

// The decoder's dispatch, over the same pack.  A geometry is decode_kernel_v4<W, L> in workgroups of 64 * W threads that hold
// W * 64 / L substreams; one that the device chooses (`chosen`: the device word) returns at once unless the word holds its `mine`.
template <class... Sets>
static hipError_t decode_v4_dispatch(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                     const uint8_t *bytes, uint8_t *bins, cabac_substream_result *results, uint32_t in_flight,
                                     int lanes_per_sub, uint32_t *select, const Sets &...sets) {
  const uint32_t on_chip = max(n_sub, in_flight);
  auto launch = [&](auto kernel, uint32_t W, uint32_t L, const uint32_t *chosen = nullptr, uint32_t mine = 0u) {
    const uint32_t per_group = W * 64u / L;
    hipLaunchKernelGGL(kernel, dim3((n_sub + per_group - 1u) / per_group), dim3(64u * W), 0, st, n_sub, desc, records, bytes, bins, results,
                       chosen, mine, sets...);
  };
  if (lanes_per_sub == 0) {  // auto
    if (on_chip <= kSoloUpTo) {
      // up to one substream per SIMD: a wave each, 64 bins a step (16 ... 1 024 C4-type substreams 1.13-1.16 ms against 1.30)
      lanes_per_sub = 64;
    } else if (select != nullptr && on_chip <= kSoloAskUpTo && in_flight <= n_sub) {  // (not for chunks of a bigger batch)
      hipLaunchKernelGGL(decode_select_solo_kernel, dim3(1), dim3(1024), 0, st, n_sub, desc, kSoloUpTo, select);
      launch(decode_kernel_v4<4, 64, Sets...>, 4, 64, select, 2u);
      launch(decode_kernel_v4<4, 16, Sets...>, 4, 16, select, 0u);
      return hipGetLastError();
    } else if (on_chip < kHexFrom || select == nullptr) {
      lanes_per_sub = 16;
    } else {
      // enough substreams for the sixteen-per-wave geometry IF they are about equally long: asked on the device, both
      // geometries launched, the one not chosen returns at once
      // (a chunk of a bigger batch in flight is judged by its share of the threshold)
      const uint32_t thr = (uint32_t)((uint64_t)kHexFrom * n_sub / on_chip);
      hipLaunchKernelGGL(decode_select_kernel, dim3(1), dim3(1024), 0, st, n_sub, desc, thr, select);
      launch(decode_kernel_v4<4, 4, Sets...>, 4, 4, select, 1u);
      launch(decode_kernel_v4<4, 16, Sets...>, 4, 16, select, 0u);
      return hipGetLastError();
    }
  }
  if (lanes_per_sub == 64) {  // one substream per wave, 64 bins per step: the per-step work around the chain is spread over 64 bins
    if (on_chip >= 1024u) launch(decode_kernel_v4<4, 64, Sets...>, 4, 64);
    else launch(decode_kernel_v4<1, 64, Sets...>, 1, 64);
  } else if (lanes_per_sub == 4) {  // sixteen substreams per wave, 64 per workgroup (one workgroup's LDS fills most of a CU)
    launch(decode_kernel_v4<4, 4, Sets...>, 4, 4);
  } else if ((on_chip + kQuadSubs - 1) / kQuadSubs >= 1024u) {  // four substreams per wave: four-wave workgroups pin one wave per SIMD
    launch(decode_kernel_v4<4, 16, Sets...>, 4, 16);
  } else {
    launch(decode_kernel_v4<1, 16, Sets...>, 1, 16);
  }
  return hipGetLastError();
}

hipError_t launch_decode_v4(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            const uint8_t *bytes, uint8_t *bins, cabac_substream_result *results, uint32_t in_flight, int lanes_per_sub,
                            uint32_t *select, const CtxSets *sets) {
  if (sets == nullptr) return decode_v4_dispatch(st, n_sub, desc, records, bytes, bins, results, in_flight, lanes_per_sub, select);
  return decode_v4_dispatch(st, n_sub, desc, records, bytes, bins, results, in_flight, lanes_per_sub, select, *sets);
}

}  // namespace cabac
