/*
 * cabac_hip_search_unit.h — C ABI of the search rounds over candidates with side syntax: a candidate of a rate-distortion search is
 * a RECORD STRING WITH BLOCKS SPLICED IN (a transform unit with its cbf flags, mts_idx, lfnst_idx, transform_skip_flag and
 * cu_qp_delta; a split against a no-split; "all cbf zero", which has no block at all), costed in one fused walk, and the contexts it
 * leaves cover all 379 entries.  An extension of cabac_hip_search.h (same conventions, same context-set format, same IN-PLACE RULE,
 * same cost and pick), kept in a header of its own so that the declaration lists of the other headers stay what they are.
 *
 * Replace: what the reference's estimator — a full CABACWriter on a BitEstimator_Std — costs for one alternative: whatever the walk
 * emits, not only residual_coding.  The side bins cost bits that differ between the alternatives, and they adapt contexts that the
 * following blocks read (TransformSkipFlag, 310 / 311) and that the next position starts from (the cbf, MTS and LFNST contexts).
 * The writer's side has this shape already: cabac_hip_encode_residual_device takes host records with blocks spliced in at positions.
 *
 * DEFINITION OF THE RESULT.
 *   Candidate c owns the blocks d_tu[d_cand_first[c] .. d_cand_first[c + 1]) as in cabac_hip_estimate.h, and the SIDE RECORDS
 *   d_records[d_rec_first[c] .. d_rec_first[c + 1]) (records in the format of cabac_hip.h).  d_rec_first is uint64_t with n_cand + 1
 *   entries; a run that goes backwards or past d_rec_first[n_cand] is clipped to empty, or to what is left of it, as d_cand_first is
 *   clipped.  n_rec(c) is the length of the clipped run (at most 2^32 - 1: a longer run is cut there).
 *   BLOCK POSITIONS.  d_tu_at[t] (uint32_t, one per block) is the index into the candidate's own side run in front of which block t
 *   is inserted.  The effective position is at(t) = min(max(d_tu_at[t], at(t - 1)), n_rec(c)), where at() before the candidate's
 *   first block is 0: positions never go backwards and never pass the end of the run, and several blocks at one position keep their
 *   order.  d_tu_at == NULL puts every block behind the last side record.
 *   EXPANDED STRING.  The expanded string of c is its side records with, at every block's position, the records
 *   cabac_hip_residual_device produces for that block.  A block flagged CABAC_TU_INFO_EMPTY or CABAC_TU_INFO_BAD_DESC contributes
 *   nothing, as in cabac_hip_estimate.h.
 *   RESULTS.  d_frac_bits[c] is what cabac_hip_estimate_from_device answers for the expanded string from set d_set[c].
 *   d_tu_frac_bits[t] is the sum of the costs of block t's own bins within that string; d_tu_info[t] is the block's as in
 *   cabac_hip_estimate.h.  THE SET THE CANDIDATE LEAVES is its start set with update() (contexts.cpp:903-913) applied for every
 *   context-coded record of the expanded string, in order.  All 379 entries come from the walk (the states of the start set are read
 *   under the masks of the format: m_state[0] & 0x7FE0, rates 2..5 / 5..12 — every set cabac_hip_ctx_init_device or one of these
 *   calls wrote).
 *   RECORD KINDS ALLOWED IN SIDE RUNS.  Context-coded records, ids 0..378; CABAC_REC_EP; CABAC_REC_TRM, costing estFracBitsTrm
 *   (contexts.cpp:931-933); CABAC_REC_ALIGN, which rounds the running total — the blocks before it included — up to a whole bit
 *   (arith_codec.cpp:679-684).  Any other id, CABAC_REC_EST_RESETBITS and CABAC_REC_EST_RESTART included, is a BAD RECORD: then
 *   d_flags[c] = CABAC_RES_BAD_RECORD and d_frac_bits[c] = UINT64_MAX, the set the candidate would write and the per-block outputs of
 *   its own blocks are unspecified, and nothing else is touched.  d_flags[c] is 0 otherwise.  d_flags may be NULL.
 *   TWO IDENTITIES.  With no side records anywhere every output equals cabac_hip_estimate_residual_ctx_device's.  With no blocks the
 *   cost and the flags equal cabac_hip_estimate_from_device's.
 *   COST AND PICK of a round: as in cabac_hip_search.h.  A candidate with a bad record takes part with d_frac_bits = UINT64_MAX (its
 *   cost saturates); exclude it through d_dist if it must not be picked.
 *
 * All device forms are asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host synchronisation
 * inside, the scratch belongs to the ctx, no kernel waits on another workgroup.  The IN-PLACE RULE of cabac_hip_search.h applies
 * unchanged.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 19, "unit estimate"
 * (cabac_hip_estimate_unit_device); kind 20, "unit round estimate", kind 21, "unit round select", and kind 22, "unit round commit"
 * — a round reports its three parts as 20, 21, 22 in this order.
 */
#ifndef CABAC_HIP_SEARCH_UNIT_H
#define CABAC_HIP_SEARCH_UNIT_H

#include "cabac_hip_search.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. cost candidates with side records, and the contexts they leave ----
 * The arguments of cabac_hip_estimate_residual_ctx_device, with the coefficients as in cabac_hip_search_round_device (coeff_bytes 4:
 * int32_t, 2: int16_t), plus d_rec_first, d_records, d_tu_at and d_flags (see above; d_records may be NULL when every run is
 * empty).  d_tu_frac_bits, d_tu_info, d_tu_at and d_flags may be NULL.  d_out_set == NULL writes no set (d_out_state / d_out_rate
 * are then not used); otherwise candidate c with d_out_set[c] != CABAC_SEARCH_NO_SET writes the set it leaves as set d_out_set[c]
 * of d_out_state / d_out_rate, which may be d_state / d_rate under the in-place rule. */
int cabac_hip_estimate_unit_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                   const void *d_coeff, int coeff_bytes, const uint32_t *d_state, const uint8_t *d_rate,
                                   const uint32_t *d_set, const uint64_t *d_rec_first, const uint16_t *d_records,
                                   const uint32_t *d_tu_at, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info,
                                   uint32_t *d_flags, const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate);

/* ---- 2. one round in one call: estimate, select, commit ----
 * cabac_hip_search_round_device over such candidates: costs all n_cand candidates as part 1 does, picks per group as
 * cabac_hip_search_select_device does, and writes the set the picked candidate of group g leaves — all 379 entries from its walk —
 * as set d_group_out_set[g] of d_state / d_rate.  The commit walks the picked candidates a second time with their side records. */
int cabac_hip_search_unit_round_device(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                       const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                       uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set, const uint64_t *d_rec_first,
                                       const uint16_t *d_records, const uint32_t *d_tu_at, const uint32_t *d_group_out_set,
                                       const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                       uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, uint32_t *d_flags);

/* ---- 3. host-pointer form (synchronous) ----
 * The same round on host arrays, staged like cabac_hip_search_round_batch: records holds n_records_total side records, rec_first
 * n_cand + 1 entries, tu_at (may be NULL) cand_first[n_cand] entries.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for everything cabac_hip_search_round_batch refuses, and
 * for: a rec_first that is not non-decreasing or that ends past n_records_total, a tu_at that decreases inside a candidate or
 * exceeds its run length, and a bad side record (cabac_hip_last_error names the candidate and the record).  Returns
 * CABAC_HIP_ERR_SUBSTREAM as cabac_hip_search_round_batch does. */
int cabac_hip_search_unit_round_batch(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                      const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                      uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                      const uint16_t *records, uint64_t n_records_total, const uint64_t *rec_first,
                                      const uint32_t *tu_at, const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16,
                                      uint64_t *frac_bits, uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SEARCH_UNIT_H */
