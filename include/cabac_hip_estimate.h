/*
 * cabac_hip_estimate.h — C ABI of the fused residual estimator of libcabac_hip.so: transform-block coefficients to
 * fractional bits.  An extension of cabac_hip.h (same conventions: plain pointers and sizes, 0 or a negative
 * cabac_hip_status, no exception crosses the boundary), kept in a header of its own: the reference-side test libraries
 * (oracle/Makefile) are pinned to the content of cabac_hip.h, and nothing declared here changes what they were compiled
 * against.
 */
#ifndef CABAC_HIP_ESTIMATE_H
#define CABAC_HIP_ESTIMATE_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- coefficients -> fractional bits: cost transform blocks on the device (the estimator's side of row f2) ----
 * Replace: the rate-distortion search's use of the second writer an encoder owns — CABACWriter m_CABACEstimatorStd on a
 * BitEstimator_Std (cabac_writer.hpp:190-205, getCABACEstimator()): contexts assigned from the real coder's
 * (Ctx::operator=, contexts.hpp:254), resetBits(), residual_coding(tu, compID, cuCtx) (cabac_writer.cpp:2424-2525),
 * getEstFracBits() — for a batch of n_cand candidates in one launch, without bin records.
 * A CANDIDATE c is the run of blocks d_tu[d_cand_first[c] .. d_cand_first[c + 1]) (n_cand + 1 entries, as d_tile_first of the
 * parser), costed in order with the contexts carried from block to block — e.g. the Y, Cb and Cr blocks of one transform unit.
 * Candidates are independent of each other.  Candidate c starts from context set d_set[c] of d_state / d_rate, in the format of
 * cabac_hip_ctx_init_device and cabac_hip_estimate_from_device (379 entries per set: m_state[0] | m_state[1] << 16, m_rate),
 * followed by resetBits(); many candidates may share a set, and the sets are not modified.
 *   d_frac_bits[c]     cost of candidate c in 1/32768 bit (SCALE_BITS = 15)
 *   d_tu_frac_bits[t]  (may be NULL) the share of block t; the shares of a candidate sum to its total
 *   d_tu_info[t]       (may be NULL) exactly the word cabac_hip_residual_device reports for block t
 * DEFINITION OF THE RESULT: d_tu_frac_bits[t] is what cabac_hip_estimate_from_device answers for the records
 * cabac_hip_residual_device produces for d_tu[t], started from the contexts the candidate's earlier blocks left.  So every
 * cabac_tu_desc flag the binariser covers is covered (dependent quantisation, sign hiding, CABAC_TU_TS_FLAG, transform skip,
 * BDPCM, SBT zero-out, max_log2_tr_range, 64-wide blocks) and the range extensions are not, as there.  A block flagged
 * CABAC_TU_INFO_EMPTY or CABAC_TU_INFO_BAD_DESC costs 0 and leaves the contexts alone.
 * Regular and transform-skip / BDPCM blocks alike are costed by one fused kernel (cabac_residual_estimate.hip): the
 * binariser's walk with a cost lookup and a context update where it writes a record — the coefficients are read once and no
 * record exists anywhere; contexts carry through a candidate that mixes both kinds of block.
 * Asynchronous on the ctx's stream like the other *_device calls (stream ordering contract in cabac_hip.h), no host synchronisation
 * inside; scratch (the candidate order) belongs to the ctx.  n_cand == 0 is OK and launches nothing.  The device forms do not
 * see a bad d_cand_first: a run that goes backwards or past d_cand_first[n_cand] is clipped (it costs what is left of it). */
int cabac_hip_estimate_residual_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first,
                                       const cabac_tu_desc *d_tu, const int32_t *d_coeff, const uint32_t *d_state,
                                       const uint8_t *d_rate, const uint32_t *d_set, uint64_t *d_frac_bits,
                                       uint64_t *d_tu_frac_bits, uint32_t *d_tu_info);
/* The same with the coefficients as int16_t (d_tu[].coeff_offset counts int16_t then), as cabac_hip_encode_residual16_device */
int cabac_hip_estimate_residual16_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first,
                                         const cabac_tu_desc *d_tu, const int16_t *d_coeff, const uint32_t *d_state,
                                         const uint8_t *d_rate, const uint32_t *d_set, uint64_t *d_frac_bits,
                                         uint64_t *d_tu_frac_bits, uint32_t *d_tu_info);
/* Host-pointer form (synchronous).  coeff holds n_coeff_total coefficients of coeff_bytes bytes each (4: int32_t, 2: int16_t);
 * state / rate hold n_sets context sets; tus holds cand_first[n_cand] blocks; tu_frac_bits / tu_info (may be NULL) one entry
 * per block.  Returns CABAC_HIP_ERR_INVALID (nothing is costed) for a cand_first that is not non-decreasing, a block of a
 * candidate whose coefficients do not lie inside n_coeff_total, or a set[c] >= n_sets; CABAC_HIP_ERR_SUBSTREAM if a block of a
 * candidate is empty or has a bad descriptor (tu_info says which; the numbers still arrive). */
int cabac_hip_estimate_residual_batch(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                      const void *coeff, int coeff_bytes, uint64_t n_coeff_total, const uint32_t *state,
                                      const uint8_t *rate, uint32_t n_sets, const uint32_t *set, uint64_t *frac_bits,
                                      uint64_t *tu_frac_bits, uint32_t *tu_info);

/* cabac_hip_profile_read (cabac_hip.h) reports these calls as kind 12, "residual estimate", after the kinds listed there. */

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_ESTIMATE_H */
