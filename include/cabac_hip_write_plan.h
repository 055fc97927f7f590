/*
 * cabac_hip_write_plan.h — C ABI of the plan write: the writer's counterpart of the plan parse (cabac_hip_parse_plan.h).  The SAME
 * plan — syntax elements in the device binariser's format, guards, CABAC_PE_COND / CABAC_PE_BLOCK_INFO entries, blocks behind
 * guards — together with the values of the real elements and the coefficients of the blocks, all in device memory, becomes coded
 * substreams with no host pass: the device evaluates every guard, binarises every side element that is coded, decides which blocks
 * are coded, and knows each block's scanPosLast when it decides whether mts_idx is written.  What it writes, the plan parse reads
 * back with the same plan.  An extension of the spliced-residual writer of cabac_hip.h (cabac_hip_encode_residual_device), in a
 * header of its own so that the declaration lists of the other headers stay what they are.
 *
 * This header uses CABAC_GUARD, the CABAC_GUARD_* comparisons, CABAC_RES_BAD_VALUE and CABAC_TU_INFO_NOT_CODED of
 * cabac_hip_parse_elements.h and CABAC_PE_COND / CABAC_PE_BLOCK_INFO of cabac_hip_parse_plan.h and does not repeat them: INCLUDE
 * THAT HEADER FIRST (both of them, the element parse's in front).
 *
 * DEFINITION OF THE RESULT.
 *   INPUTS.  Substream s is described by
 *     d_desc[s]      rec_offset / n_records count plan ELEMENTS, as in the plan parse; qp and init_id | CABAC_SUB_FINISH
 *                    [| CABAC_SUB_ALIGN_RBSP] as for cabac_hip_encode_residual_device; byte_offset / byte_capacity are ignored, as
 *                    they are there (the library sizes the byte slots itself);
 *     d_plan         the plan parse's format, unchanged: 2 x uint32_t per entry, kinds 0..10;
 *     d_values_in    d_values_in[rec_offset + i] is the value of real element i (kinds 0..8).  It is used only where the element is
 *                    a real one whose guard holds;
 *     d_tile_first, d_tu, d_tu_at, d_tu_guard, d_coeff, coeff_bytes (4: int32_t, 2: int16_t)   as in the plan parse; here d_coeff
 *                    is INPUT.  n_tu is the number of blocks, d_tile_first[n_sub].
 *   OUTPUTS.
 *     d_payload / payload_capacity / d_payload_offsets (n_sub + 1) / d_results   as in cabac_hip_encode_residual_device: the coded
 *                    substreams compacted in descriptor order, results[s] = {bits written, flags};
 *     d_values_out   (may be NULL, may equal d_values_in) receives the FILLED values: exactly what the plan parse's d_values
 *                    receives when it reads the payload — the real value where the element is coded, 0 where it is skipped, the
 *                    computed value at kinds 9 and 10;
 *     d_tu_info      (may be NULL) receives the plan parse's INFO WORD of every block: scanPosLast | CABAC_TU_INFO_MTS_VIOLATION
 *                    for a regular block, CABAC_TU_INFO_TS for a block written as transform skip (the binariser's own word holds
 *                    a position there; it is mapped), CABAC_TU_INFO_NOT_CODED for a skipped one.
 *   THE WALK is the plan parse's, on the writer's side: block positions at(t) = min(max(d_tu_at[t], at(t - 1)), n_records)
 *   (d_tu_at == NULL: behind the plan); for i = 0 .. n_records first every block with at(t) == i, in order, then entry i.  Guards,
 *   COND tests, BLOCK_INFO fields and nb(i) are evaluated on the FILLED values and on the info words defined above.  A skipped
 *   element or block contributes no bin.  A coded element contributes the bins cabac_hip_binarize_device makes of (word0, value).
 *   A coded block contributes the records of cabac_hip_residual_device (with CABAC_TU_TS_FLAG its transform_skip_flag first).
 *   Computed entries contribute no bin.  The coefficients and the descriptor of a SKIPPED block are not examined for content — an
 *   all-zero block behind a false cbf is the normal case —; their range is still checked where ranges are checked (the batch
 *   form).
 *   STOPS.  A stop codes nothing for that substream: zero payload bytes, n_bits 0 and exactly one flag.  The other substreams are
 *   not affected.  The stopped substream's entries of d_values_out and d_tu_info are unspecified, and nothing is written outside
 *   its own ranges of them.
 *   CABAC_RES_BAD_RECORD   a bad plan entry or a bad block guard.  The list is exactly the plan parse's (kind above 10; a ctxId
 *                          >= 379; EP_BINS numBins > 32; UNARY_EP maxSymbol > 32; TRUNC_BIN maxSymbol 0; REM_ABS outside
 *                          maxLog2TrDR 15..20, cutoff <= 32 - maxLog2TrDR, rice <= 14; reserved guard or test bits; back > i, for
 *                          a block back > at(t); join 3; a join with back2 0 or back2 > i; which >= nb(i); width 0; shift + width
 *                          > 32).  It depends on no value: a bad entry stops the substream also where its guard would skip it, and
 *                          takes precedence over CABAC_RES_BAD_VALUE.
 *   CABAC_RES_BAD_VALUE    (a) an ACTIVE real element (its guard holds) whose value is outside what its code carries.  The
 *                          domain per kind:
 *                            CTX_BIN, TRM   value <= 1
 *                            EP_BINS        value < 2^numBins
 *                            UNARY_MAX, UNARY_EP   value <= maxSymbol
 *                            TRUNC_BIN      value < maxSymbol
 *                            REM_ABS        value within the code word's range: at most
 *                                           ((2^(32 - maxLog2TrDR - cutoff) + cutoff - 1) << rice) + 2^maxLog2TrDR - 1
 *                            EXP_GOLOMB     count + prefix ones < 32, that is value < 2^32 - 2^count
 *                            ALIGN          carries no value: any
 *                          For every kind the domain is precisely the set of values the element parse reads back unflagged.
 *                          (b) a CODED block that is CABAC_TU_INFO_EMPTY or CABAC_TU_INFO_BAD_DESC.
 *   THREE IDENTITIES.
 *   W1. The payload and n_bits of a substream are what the reference's encoder makes of the record string of the walk above on
 *       the filled values (tests/parse_plan_model.py::fill / expand state it on the CPU; the oracle encodes the string).
 *   W2. A plan with no guard, no block guard and no computed entry gives, on any content, the payload, offsets, results and info
 *       words of cabac_hip_encode_residual_device when that call is fed cabac_hip_binarize_device's records of the same elements
 *       with word1 = value, and one splice per block at the record index of element at(t) (transform-skip blocks excepted in the
 *       info word alone, which is mapped as said above).
 *   W3. The plan parse's device form over the payload, with the same d_desc (byte ranges from the offsets), plan, d_tu, d_tu_at
 *       and d_tu_guard, returns d_values equal to d_values_out, d_tu_info equal to the written one, the coded region (top-left
 *       32 x 32) of every coded block equal to the input, and no flag.
 *
 * The device form is asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h, with the one exception
 * cabac_hip_encode_residual_device has: it waits for the ctx's stream ONCE in the middle, because the expanded sizes decide the
 * buffers and the launch geometry of the second half; the rest is queued on the stream when it returns.  No kernel waits for
 * another workgroup.  Intermediate buffers belong to the ctx and grow on demand.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call's own kernels after the kinds listed in the other headers: kind 28, "plan
 * write" (the resolve walk, the scan, the emit walk, the stops); the residual passes, the encode kernel and the assembly inside it
 * report under their own kinds, as in cabac_hip_encode_residual_device.
 */
#ifndef CABAC_HIP_WRITE_PLAN_H
#define CABAC_HIP_WRITE_PLAN_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_tu_at, d_tu_guard, d_values_out and d_tu_info may be NULL; d_tu and d_coeff when n_tu is 0; d_plan and d_values_in when every
 * plan is empty.  Returns CABAC_HIP_ERR_INVALID for a NULL that is needed, coeff_bytes other than 4 or 2, or a substream that
 * outgrows 32 bits of records (nothing is coded then). */
int cabac_hip_write_plan_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info);

/* Host-pointer form (synchronous), staged like cabac_hip_encode_batch_residual.  n_elements_total bounds plan (2 *
 * n_elements_total words), values_in and values_out; n_coeff_total bounds coeff; tu_at, tu_guard and tu_info (each may be NULL)
 * hold tile_first[n_sub] entries; values_out may be NULL and may equal values_in.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for everything the plan parse's host-pointer form refuses
 * about plan, guards, tile_first, tu_at and coefficient ranges: a NULL that is needed, coeff_bytes other than 4 or 2, an init_id
 * above 2, a plan that leaves n_elements_total, a tile_first that decreases, a tu_at that decreases inside a substream or exceeds
 * its plan length, a bad plan entry or block guard (cabac_hip_last_error names the substream and the element, or the block), and
 * coefficients out of range — of EVERY block, guarded ones included.  Returns CABAC_HIP_ERR_INVALID too when payload_capacity is
 * too small.  Returns CABAC_HIP_ERR_SUBSTREAM when a result flag is set. */
int cabac_hip_write_plan_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *plan,
                               const uint32_t *values_in, uint64_t n_elements_total, const uint32_t *tile_first,
                               const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard, const void *coeff,
                               int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                               uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *values_out, uint32_t *tu_info);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_WRITE_PLAN_H */
