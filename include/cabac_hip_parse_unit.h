/*
 * cabac_hip_parse_unit.h — C ABI of the unit parse: the residual parser over SPLICED substreams, side records and transform blocks
 * read back in one walk.  The reader's side of what cabac_hip_encode_residual_device writes, cabac_hip_estimate_unit_device costs
 * and the winner log codes: the caller supplies the ctxId / EP / TRM sequence of the syntax it walks itself (the decode boundary
 * of cabac_hip_decode_device) ... and the blocks' contexts are derived on the device (cabac_hip_residual_parse_device).  No
 * variable-length syntax is interpreted here and no side bin steers the walk: the side plan and the block geometry are inputs.
 * An extension of cabac_hip_parse.h (same rules on empty, damaged and refused input), in a header of its own so that the
 * declaration lists of the other headers stay what they are.
 *
 * DEFINITION OF THE RESULT.
 *   Substream s is described by d_desc[s] — byte_offset, byte_capacity, qp, init_id | CABAC_SUB_FINISH as for the residual parser,
 *   and additionally rec_offset / n_records —, by its SIDE RUN d_records[rec_offset .. rec_offset + n_records) (records in the
 *   format of cabac_hip.h; the bin bit is ignored, as in cabac_hip_decode_device) and by its blocks
 *   d_tu[d_tile_first[s] .. d_tile_first[s + 1]), in coded order.
 *   BLOCK POSITIONS.  d_tu_at[t] (uint32_t, one per block) is the index into the substream's own side run in front of which block t
 *   is coded.  The clipping rule of cabac_hip_search_unit.h: at(t) = min(max(d_tu_at[t], at(t - 1)), n_records), where at() before
 *   the substream's first block is 0 — positions never go backwards and never pass the end of the run, several blocks at one
 *   position keep their order.  d_tu_at == NULL puts every block behind the run.
 *   THE WALK.  start(); then for i = 0 .. n_records: first every block with at(t) == i, in order, then side record i if
 *   i < n_records.
 *   A BLOCK is parsed exactly as cabac_hip_residual_parse_device parses it: CABAC_TU_TS_FLAG, CABAC_TU_TRANSFORM_SKIP,
 *   CABAC_TU_BDPCM, CABAC_TU_SBT_ZERO_OUT, CABAC_TU_DEP_QUANT and CABAC_TU_SIGN_HIDING as documented there, what is written and
 *   what is not as in cabac_hip_parse.h, d_tu_info likewise; a refused block stops the substream with CABAC_RES_BAD_RECORD.
 *   A SIDE RECORD is decoded as cabac_hip_decode_device decodes it, and its bin goes to d_side_bins[rec_offset + i], one byte per
 *   record: ids 0..378 decodeBin(id); CABAC_REC_EP a bypass bin; CABAC_REC_TRM decodeBinTrm (arith_codec.cpp:181-197) — decoding
 *   goes on whatever the bin is, from the state the reference's decoder is left in (after a bin of 1: range - 2, not
 *   renormalised); CABAC_REC_ALIGN range := 256, bin 0.  Any other id stops the substream there with CABAC_RES_BAD_RECORD, like a
 *   refused block: nothing behind it is written (no bin, no block, no d_tu_info word), the stop check is not made, and n_bits
 *   counts up to it.
 *   ONE context store per substream, with all 379 contexts, initialised from (qp, init_id & 3).  A side record may name a
 *   residual-coding context (86..291, 310 / 311, 357..378): the next block then reads what that record left, and the other way
 *   round.  Code a block's transform_skip_flag either as a side record (context 310 / 311) in front of the block with
 *   CABAC_TU_TS_FLAG clear — how cabac_hip_encode_residual_device asks for it — or let the parser read it (CABAC_TU_TS_FLAG set).
 *   CABAC_SUB_FINISH here means only the finish() stop-pattern check (arith_codec.cpp:68-73), as in cabac_hip_decode_device:
 *   there is no implied terminate bin.  The terminate bin is a side record, which is how cabac_hip_encode_residual_device writes
 *   it.
 *   RESULTS.  d_results[s] = {bits read, flags}.  CABAC_RES_UNDERRUN is reported alone, under the rules of cabac_hip_parse.h (from
 *   the read past byte_capacity on, blocks, side bins and n_bits are unspecified); CABAC_RES_RANGE applies to 16-bit coefficients
 *   as there and stops nothing; a first byte 0xFF is refused as there (nothing parsed, no side bin written, CABAC_RES_BAD_STOP,
 *   n_bits 8); byte_capacity 0 gives CABAC_RES_UNDERRUN with nothing read.
 *   Nothing outside the coded regions of the parsed blocks, the decoded records' bin bytes and the parsed blocks' info words is
 *   written.  Every loop is bounded by n_records and the block geometry alone: arbitrary bytes terminate.
 *   TWO IDENTITIES.
 *   I1. With every n_records == 0 and no CABAC_SUB_FINISH every output equals cabac_hip_residual_parse_device's.  With
 *       CABAC_SUB_FINISH that call equals this one with the side run [CABAC_REC_TRM] behind the blocks, where its
 *       CABAC_RES_BAD_STOP is "side bin 0, or CABAC_RES_BAD_STOP here".
 *   I2. With no blocks d_side_bins and d_results equal cabac_hip_decode_device's wherever that call's results carry no flag.
 *
 * The device form is asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host
 * synchronisation, no allocation that depends on the data, no kernel that waits for another workgroup.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call after the kinds listed in the other headers: kind 25, "unit parse".
 */
#ifndef CABAC_HIP_PARSE_UNIT_H
#define CABAC_HIP_PARSE_UNIT_H

#include "cabac_hip_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* coeff_bytes 4: d_coeff is int32_t, 2: int16_t (d_tu[t].coeff_offset counts elements of that type), as in the search headers.
 * d_tu_at, d_tu_info and d_side_bins may be NULL — d_side_bins only when every run is empty; d_records may be NULL when every
 * run is empty. */
int cabac_hip_parse_unit_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                const uint16_t *d_records, void *d_coeff, int coeff_bytes, uint8_t *d_side_bins,
                                uint32_t *d_tu_info, cabac_substream_result *d_results);

/* Host-pointer form (synchronous), staged like cabac_hip_residual_parse_batch: bytes_total, n_records_total and n_coeff_total
 * bound bytes, records / side_bins and coeff; tu_at (may be NULL) and tu_info (may be NULL) hold tile_first[n_sub] entries.  coeff
 * as there: int32_t keeps the caller's values where nothing is written, int16_t is output only (zero there).  side_bins keeps
 * the caller's values where no record was decoded.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for everything cabac_hip_residual_parse_batch refuses,
 * and for: a run that leaves n_records_total, a tile_first that decreases, a tu_at that decreases inside a substream or exceeds
 * its run length, and a bad side record (cabac_hip_last_error names the substream and the record).  Returns
 * CABAC_HIP_ERR_SUBSTREAM when a result flag is set. */
int cabac_hip_parse_unit_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                               uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                               const uint16_t *records, uint64_t n_records_total, void *coeff, int coeff_bytes,
                               uint64_t n_coeff_total, uint8_t *side_bins, uint32_t *tu_info, cabac_substream_result *results);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PARSE_UNIT_H */
