/*
 * cabac_hip_parse_elements.h — C ABI of the element parse: the unit parse (cabac_hip_parse_unit.h) with a side plan of SYNTAX
 * ELEMENTS in the device binariser's own format, each decoded to its value on the device, and with the smallest form of
 * steering that makes the walk a reader: an element or a block may be GUARDED by the value of an earlier element (cbf -> block,
 * cbf -> transform_skip_flag, cu_qp_delta_abs prefix == 5 -> Exp-Golomb escape, prefix != 0 -> sign bin).  No jumps, no loops:
 * the plan is walked forwards once.  An extension of cabac_hip_parse.h (same rules on empty, damaged and refused input), in a
 * header of its own so that the declaration lists of the other headers stay what they are.
 *
 * DEFINITION OF THE RESULT.
 *   Substream s is described by d_desc[s] as for the unit parse — byte_offset, byte_capacity, qp, init_id | CABAC_SUB_FINISH,
 *   rec_offset, n_records —, where rec_offset and n_records count ELEMENTS of d_plan, by its PLAN
 *   d_plan[2 * rec_offset .. 2 * (rec_offset + n_records)) and by its blocks d_tu[d_tile_first[s] .. d_tile_first[s + 1]), in coded
 *   order.
 *   PLAN.  An element is 2 x uint32_t (d_plan is 8-byte aligned).  word0 is the syntax-element record's word0 of cabac_hip.h,
 *   unchanged: the kind in bits 3..0, the parameters where the binariser reads them (bits it does not read are ignored here too).
 *   word1 is the GUARD WORD; it sits where the binariser's record holds the value.
 *   BLOCK POSITIONS.  d_tu_at[t] indexes elements, with the clipping rule of the unit parse:
 *   at(t) = min(max(d_tu_at[t], at(t - 1)), n_records); d_tu_at == NULL puts every block behind the plan.
 *   THE WALK.  start(); then for i = 0 .. n_records: first every block with at(t) == i, in order, then element i if
 *   i < n_records.
 *   GUARD WORD.
 *     bits  7..0   back   0 means unguarded
 *     bits  9..8   cmp    0 !=, 1 ==, 2 >=, 3 < (unsigned)
 *     bits 15..10  -      must be zero
 *     bits 31..16  imm    comparison operand
 *   Element i with back != 0 is coded if and only if value(i - back) cmp imm holds, where value(j) is what d_values receives for
 *   element j of the same substream.  value() of a skipped element is 0, so guards chain.  A skipped element reads no bin and
 *   touches no context; d_values gets 0 for it.  With back == 0 cmp and imm are ignored.
 *   A block's guard, d_tu_guard[t] (d_tu_guard == NULL: no block is guarded), has the same format and refers to element
 *   at(t) - back.  A skipped block reads no bin, its coefficients are not written, its descriptor is not examined on the device,
 *   and d_tu_info[t] = CABAC_TU_INFO_NOT_CODED.  A block that is coded is parsed exactly as the unit parse parses it.
 *   VALUES.  d_values[rec_offset + i] is what the reference's reader returns for the element:
 *     CTX_BIN, TRM   the bin (decodeBin / decodeBinTrm, arith_codec.cpp:181-197).  Decoding goes on after a terminate bin of 1,
 *                    as in the unit parse, from the state the reference's decoder is left in (see OUT OF RANGE).
 *     EP_BINS        decodeBinsEP(numBins) (arith_codec.cpp:116-151); 0 bins gives 0; 1 bin is decodeBinEP (:100-114)
 *     REM_ABS        decodeRemAbsEP (arith_codec.cpp:153-179)
 *     UNARY_MAX, UNARY_EP, EXP_GOLOMB   the reader twins of the writer's helpers (cabac_reader.cpp:3349-3379)
 *     TRUNC_BIN      xReadTruncBinCode (cabac_reader.cpp:1162-1186)
 *     ALIGN          range := 256, value 0
 *   Arithmetic on values is modulo 2^32.
 *   A BAD PLAN ENTRY stops the substream in front of it with CABAC_RES_BAD_RECORD, exactly as a bad side record does in the unit
 *   parse: nothing behind it is written (no value, no block, no d_tu_info word), the stop check is not made, and n_bits counts up
 *   to it.  Whether an entry is bad does not depend on any decoded value; a bad entry stops the substream even where its guard
 *   would have skipped it.  Bad entries are: kind > 8; a ctxId >= 379 (CTX_BIN, or either id of UNARY_MAX); EP_BINS numBins > 32;
 *   UNARY_EP maxSymbol > 32; TRUNC_BIN maxSymbol 0; REM_ABS outside maxLog2TrDR 15..20, cutoff <= 32 - maxLog2TrDR, rice <= 14
 *   (outside this region the code word is not defined); nonzero reserved guard bits (15..10), also where back is 0; back > i, or
 *   for a block back > at(t).  A block guard with one of the last two faults stops the substream in front of the block.
 *   A CODE WORD NO WRITER PRODUCES.  The reference's Exp-Golomb reader has no bound on its prefix.  Here the prefix ends at a 0
 *   bin, or when count + ones reaches 32.  In the second case the substream stops at that element with CABAC_RES_BAD_VALUE: the
 *   element's value and everything behind it are not written, there is no stop check, and n_bits counts the 32 - count prefix
 *   bins that were read.  No other kind needs such a rule: every other loop is bounded by its parameters (<= 255 context bins,
 *   <= 32 bypass bins per code word).
 *   BOUNDS.  Every loop of the walk is bounded by n_records, the parameters of the plan's entries and the block geometry alone:
 *   arbitrary bytes terminate, and no decoded value enters a loop bound other than through the length of a code word's suffix: a
 *   code word has a prefix and a suffix of at most 32 bins each, whatever was decoded (63 bins for a 31-bit Exp-Golomb value,
 *   17 + 30 for REM_ABS).
 *   OUT OF RANGE.  The arithmetic decoder keeps value < range << 7 on every stream a writer produced.  Two things can break that:
 *   a terminate bin of 1 (the reference's decoder leaves range - 2 below the value and does not renormalise), and ALIGN on bytes
 *   no writer produced (range := 256 below the value).  The reference's own readers then disagree with one another — the
 *   eight-at-a-time and aligned paths of decodeBinsEP and bin-by-bin decodeBinEP — and its 32-bit value register runs over.  So:
 *   from the first element or coded block that is MET IN THAT STATE on (skipped ones and ALIGN, which read no bin, are not
 *   counted), the values, the guard outcomes, the blocks, n_bits and the flags CABAC_RES_BAD_STOP / CABAC_RES_BAD_VALUE of that
 *   substream are unspecified, as after an underrun; everything in front of it is as defined above, every loop stays bounded and
 *   nothing is written outside what the substream may write.  One thing stays defined for any bytes: CTX_BIN, EP_BINS with
 *   numBins 1, TRM and ALIGN elements and the blocks are decoded with the very arithmetic of the unit parse, so E1 has no
 *   exception.
 *   EVERYTHING ELSE is the unit parse's: ONE context store per substream with all 379 contexts, shared by elements and blocks
 *   (a skipped element leaves its context as it was); CABAC_SUB_FINISH is the finish() stop check alone (no implied terminate
 *   bin); CABAC_RES_UNDERRUN is reported alone (from the read past byte_capacity on, blocks, values, guard outcomes and n_bits are
 *   unspecified); CABAC_RES_RANGE applies to 16-bit coefficients and stops nothing; a first byte 0xFF is refused (nothing parsed,
 *   no value written, CABAC_RES_BAD_STOP, n_bits 8); byte_capacity 0 gives CABAC_RES_UNDERRUN with nothing read; and the rules of
 *   cabac_hip_parse.h about what is written: nothing outside the coded regions of the parsed blocks, the values of the elements
 *   walked (skipped ones included: 0), and the info words of the blocks walked (skipped ones included).
 *   TWO IDENTITIES.
 *   E1. A plan of unguarded CTX_BIN / EP_BINS with numBins 1 / TRM / ALIGN elements and d_tu_guard == NULL gives the outputs of
 *       cabac_hip_parse_unit_device on the corresponding records (ctxId / CABAC_REC_EP / CABAC_REC_TRM / CABAC_REC_ALIGN):
 *       d_values = d_side_bins widened, and d_results, the blocks and d_tu_info equal.
 *   E2. With no blocks and no guards d_values equals the values of the reference's reader run over the same elements
 *       (decodeBin, decodeBinsEP, decodeRemAbsEP and the reader twins named above) wherever no flag is set and no element is
 *       met OUT OF RANGE.
 *
 * The device form is asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host
 * synchronisation, no allocation that depends on the data, no kernel that waits for another workgroup.  It needs no library
 * scratch.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call after the kinds listed in the other headers: kind 26, "element parse".
 */
#ifndef CABAC_HIP_PARSE_ELEMENTS_H
#define CABAC_HIP_PARSE_ELEMENTS_H

#include "cabac_hip_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_RES_BAD_VALUE 0x20u          /* an Exp-Golomb prefix that reaches count + ones == 32 */
#define CABAC_TU_INFO_NOT_CODED 0x40000u   /* d_tu_info[t]: the block's guard did not hold, nothing was read for it */

/* the guard word */
#define CABAC_GUARD_NE 0u
#define CABAC_GUARD_EQ 1u
#define CABAC_GUARD_GE 2u
#define CABAC_GUARD_LT 3u
#define CABAC_GUARD(back, cmp, imm) (((uint32_t)(back) & 0xFFu) | (((uint32_t)(cmp) & 3u) << 8) | ((uint32_t)(imm) << 16))

/* coeff_bytes 4: d_coeff is int32_t, 2: int16_t (d_tu[t].coeff_offset counts elements of that type).  d_tu_at, d_tu_guard and
 * d_tu_info may be NULL; d_tu and d_coeff when there is no block; d_plan and d_values when every plan is empty. */
int cabac_hip_parse_elements_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                    const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                    const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                    uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results);

/* Host-pointer form (synchronous), staged like the unit parse's: bytes_total, n_elements_total and n_coeff_total bound bytes,
 * plan (2 * n_elements_total words) / values and coeff; tu_at, tu_guard and tu_info (each may be NULL) hold tile_first[n_sub]
 * entries.  coeff: int32_t keeps the caller's values where nothing is written, int16_t is output only (zero there).  values
 * keeps the caller's content where nothing was decoded.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for: a NULL that is needed, coeff_bytes other than 4 or
 * 2, bytes or coefficients out of range, an init_id above 2, a plan that leaves n_elements_total, a tile_first that decreases, a
 * tu_at that decreases inside a substream or exceeds its plan length, and a bad plan entry or block guard (cabac_hip_last_error
 * names the substream and the element, or the block).  The coefficient range of EVERY block is checked, guarded ones included:
 * whether a block is skipped is not known on the host.  Returns CABAC_HIP_ERR_SUBSTREAM when a result flag is set. */
int cabac_hip_parse_elements_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                   uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                                   const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                                   int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                                   cabac_substream_result *results);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PARSE_ELEMENTS_H */
