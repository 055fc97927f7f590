/*
 * cabac_hip_search_plan.h — C ABI of the search rounds over plans: a candidate of a rate-distortion search is a PLAN (the plan
 * parse's: syntax elements in the device binariser's format, guards, CABAC_PE_COND / CABAC_PE_BLOCK_INFO entries, blocks behind
 * guards), the values of its real elements and its blocks' coefficients, all in device memory.  The device resolves it with the
 * plan write's walk into the unit-candidate form of cabac_hip_search_unit.h — side records, block positions in record units, and
 * block descriptors in which a skipped block is one the binariser rejects — and the existing unit estimate, select, commit and
 * winner log take it from there unchanged.  No host pass evaluates a guard or binarises a side element, and whether mts_idx is
 * costed is decided where the block's scanPosLast is known.  An extension of cabac_hip_search_unit.h (same candidates, same
 * context-set format, same IN-PLACE RULE, same cost and pick), in a header of its own so that the declaration lists of the other
 * headers stay what they are.
 *
 * Replace: the reference costs on BitEstimator_Std the very CABACWriter walk it later codes (cabac_writer.cpp:2219-2354,
 * :2424-2525); with this header the walk that is costed and the walk that is coded are the same plan here too.
 *
 * This header uses CABAC_GUARD, the CABAC_GUARD_* comparisons, CABAC_RES_BAD_VALUE and CABAC_TU_INFO_NOT_CODED of
 * cabac_hip_parse_elements.h and the CABAC_PE_* entry kinds of cabac_hip_parse_plan.h and does not repeat them: INCLUDE THAT HEADER
 * FIRST (both of them, the element parse's in front).
 *
 * DEFINITION OF THE RESULT.
 *   INPUTS.  Candidate c owns
 *     the blocks d_tu[d_cand_first[c] .. d_cand_first[c + 1]), as in cabac_hip_search_unit.h.  n_tu is the number of blocks the
 *                    per-block arrays hold and must be d_cand_first[n_cand]; no block index at or above n_tu is touched;
 *     the plan entries d_plan[2 * d_ent_first[c] ..): d_ent_first is uint64_t with n_cand + 1 entries, and a run that goes
 *                    backwards or past d_ent_first[n_cand] is clipped to empty, or to what is left of it, exactly as d_rec_first
 *                    is clipped in cabac_hip_search_unit.h (at most 2^32 - 1 entries: a longer run is cut there).  The format is
 *                    the plan parse's, unchanged: 2 x uint32_t per entry, kinds 0..10;
 *     d_values_in    indexed like the plan entries: d_values_in[d_ent_first[c] + i] is the value of real element i (kinds 0..8) of
 *                    the candidate's plan.  It is used only where the element is a real one whose guard holds;
 *     d_tu_at        (uint32_t per block, may be NULL: behind the plan) counts ENTRIES of the candidate's own plan;
 *     d_tu_guard     (uint32_t per block, may be NULL: no guard) as in the plan write;
 *     d_coeff, coeff_bytes (4: int32_t, 2: int16_t)   the blocks' coefficients.
 *   THE WALK is the plan write's, word for word, per candidate: block positions at(t) = min(max(d_tu_at[t], at(t - 1)), n) with n
 *   the candidate's entries and at() 0 in front of its first block; for i = 0 .. n first every block with at(t) == i, in order,
 *   then entry i.  Guards, COND tests, BLOCK_INFO fields and nb(i) are evaluated on the FILLED values and on the info words: scanPosLast |
 *   CABAC_TU_INFO_MTS_VIOLATION for a regular block, CABAC_TU_INFO_TS for a block written as transform skip, CABAC_TU_INFO_NOT_CODED
 *   for a skipped one.  tests/parse_plan_model.py::fill / expand state the walk on the CPU.  The coefficients and the descriptor of a
 *   SKIPPED block are not examined for content.
 *   THE RESOLVED FORM, in caller-owned arrays:
 *     d_rec_first    (uint64_t, n_cand + 1) and d_records (record_capacity records): candidate c's SIDE RUN
 *                    d_records[d_rec_first[c] .. d_rec_first[c + 1]) holds the bins of its coded side elements, in order: exactly
 *                    what cabac_hip_binarize_device makes of (word0, value).  Computed entries and skipped elements contribute no
 *                    record; blocks contribute none either, only their position;
 *     d_tu_at_out    (uint32_t per block) the block's effective position counted in RECORDS of the candidate's own run: the
 *                    number of side records in front of it;
 *     d_tu_out       (one cabac_tu_desc per block; not d_tu) the input descriptor where the block is coded; where it is skipped the
 *                    input descriptor with log2_width = log2_height = 7, which the binariser and the estimator reject (it
 *                    contributes nothing and no coefficient of it is read); coeff_offset is kept;
 *     d_values_out   (may be NULL, may equal d_values_in; then the plan ranges of different candidates must not overlap) the FILLED
 *                    values, and d_tu_info (may be NULL) the plan parse's info words, both as the plan write reports them;
 *     d_flags        (uint32_t per candidate) 0 or exactly one flag, and d_total (uint64_t[1], may be NULL) the number of records
 *                    the call needs.
 *   These arrays are, unchanged, the arguments d_rec_first, d_records, d_tu_at and d_tu of cabac_hip_estimate_unit_device,
 *   cabac_hip_search_unit_round_device and cabac_hip_search_log_append_device: that is the whole point of the format.  The
 *   expanded string of the resolved candidate (cabac_hip_search_unit.h) is the record string of the plan write's walk.
 *   STOPS.  Per candidate exactly one flag; the other candidates are not affected.
 *   CABAC_RES_BAD_RECORD   a bad plan entry or a bad block guard: the plan write's list (the plan parse's), with i counting the
 *                          candidate's own entries.  It depends on no value: a bad entry stops the candidate also where its guard
 *                          would skip it, and takes precedence over CABAC_RES_BAD_VALUE.
 *   CABAC_RES_BAD_VALUE    an ACTIVE real element whose value is outside the domain of its kind (the plan write's table), or a
 *                          CODED block that is CABAC_TU_INFO_EMPTY or CABAC_TU_INFO_BAD_DESC.
 *   A stopped candidate gets an EMPTY RUN, all its blocks rejected and d_tu_at_out 0.  Its ranges of d_values_out and d_tu_info are
 *   unspecified, and nothing is written outside them.
 *   CAPACITY IS ALL OR NOTHING PER CALL, as for the winner log.  If the needed total exceeds record_capacity, nothing is written to
 *   d_records, every d_rec_first entry is 0, every block is rejected at position 0, and every candidate that is not stopped
 *   otherwise gets CABAC_RES_OVERFLOW (so does, alone, a candidate whose own run would pass 2^32 - 1 records: it fits no capacity).
 *   d_total still reports the need.  The call returns CABAC_HIP_OK: it cannot know.
 *   THE MOST BINS a value in its domain makes, per element kind (csrc/cabac_se_code.h):
 *                            CTX_BIN, TRM, ALIGN   1
 *                            EP_BINS        numBins                         (at most 32)
 *                            UNARY_MAX      maxSymbol                       (at most 255)
 *                            UNARY_EP       maxSymbol                       (at most 32)
 *                            TRUNC_BIN      floor(log2(maxSymbol)) + 1      (at most 28)
 *                            EXP_GOLOMB     63 - count                      (count + prefix ones < 32: at most 63)
 *                            REM_ABS        max(32, cutoff + rice + max(0, 2 * (32 - cutoff - maxLog2TrDR) - 1))   (at most 47)
 *                            COND, BLOCK_INFO   0
 *   A CAPACITY THAT ALWAYS SUFFICES: 255 records per plan entry; 63 per entry where no UNARY_MAX element has a maxSymbol above 63;
 *   or the sum of the lines above over the entries, which is what the host-pointer form allocates.
 *
 * A ROUND (cabac_hip_search_plan_round_device) is resolve, estimate, select and commit in one call: what
 * cabac_hip_search_unit_round_device answers for the resolved candidates, with these differences.  A candidate with any flag takes
 * part with d_frac_bits = UINT64_MAX (its cost saturates; exclude it through d_dist if it must not be picked even where its group has
 * nothing else), and its d_flags word is the resolve's flag; the set a flagged candidate would leave is unspecified.  d_tu_info holds
 * the plan's info words (CABAC_TU_INFO_NOT_CODED for a skipped block), not the estimator's.  d_tu_frac_bits of a skipped block is 0.
 * The resolved form stays in the caller's arrays: append it to a winner log right after the round, in stream order, and plan
 * candidates reach bytes with no emit path of their own.
 *
 * The device forms are asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host wait inside, the
 * scratch belongs to the ctx, no kernel waits for another workgroup, no atomics on the data path.  A chain of rounds whose
 * candidates carry guarded side syntax runs on one stream with no host pass between them.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 29, "plan resolve"
 * (the count walk, the scan, the emit walk); the residual sizes pass in front of it reports under kind 5, as in the plan write.  A
 * round reports 5, 29 and then the unit round's estimate, select and commit: 5, 29, 20, 21, 22 in this order.
 */
#ifndef CABAC_HIP_SEARCH_PLAN_H
#define CABAC_HIP_SEARCH_PLAN_H

#include "cabac_hip_search_unit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. plan candidates into the unit-candidate form ----
 * d_tu_at, d_tu_guard, d_values_out, d_tu_info and d_total may be NULL; d_tu, d_coeff, d_tu_at_out and d_tu_out when n_tu is 0;
 * d_plan and d_values_in when every plan is empty; d_records when record_capacity is 0.  Returns CABAC_HIP_ERR_INVALID for a NULL
 * that is needed or a coeff_bytes other than 4 or 2. */
int cabac_hip_resolve_plan_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first, const uint64_t *d_ent_first,
                                  const uint32_t *d_plan, const uint32_t *d_values_in, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                  const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                  uint64_t *d_rec_first, uint16_t *d_records, uint64_t record_capacity, uint32_t *d_tu_at_out,
                                  cabac_tu_desc *d_tu_out, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t *d_flags,
                                  uint64_t *d_total);

/* ---- 2. one round in one call: resolve, estimate, select, commit ----
 * The arguments of cabac_hip_search_unit_round_device with the plan inputs of part 1 in place of its side records and block
 * positions, and behind them the resolved form as caller-owned outputs (d_rec_first, d_records / record_capacity, d_tu_at_out,
 * d_tu_out, d_values_out, d_total: as in part 1).  d_group_out_set, d_dist, d_tu_frac_bits, d_tu_info and d_flags may be NULL as
 * there.  The commit writes the set the picked candidate of group g leaves as set d_group_out_set[g] of d_state / d_rate under the
 * IN-PLACE RULE. */
int cabac_hip_search_plan_round_device(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                       const uint32_t *d_cand_first, uint32_t n_tu, const cabac_tu_desc *d_tu, const void *d_coeff,
                                       int coeff_bytes, uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set,
                                       const uint64_t *d_ent_first, const uint32_t *d_plan, const uint32_t *d_values_in,
                                       const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const uint32_t *d_group_out_set,
                                       const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                       uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, uint32_t *d_flags,
                                       uint64_t *d_rec_first, uint16_t *d_records, uint64_t record_capacity, uint32_t *d_tu_at_out,
                                       cabac_tu_desc *d_tu_out, uint32_t *d_values_out, uint64_t *d_total);

/* ---- 3. host-pointer form (synchronous) ----
 * The same round on host arrays, staged like cabac_hip_search_unit_round_batch: plan holds 2 * n_entries_total words, values_in and
 * values_out (may be NULL, may equal values_in) n_entries_total, ent_first n_cand + 1 entries, tu_at and tu_guard (each may be NULL)
 * cand_first[n_cand]; flags (may be NULL) n_cand words.  The resolved form stays on the device; the library sizes its record buffer
 * itself FROM THE BOUND above (the sum over the entries of the most bins each can make), so the call never overflows and never
 * retries.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for everything cabac_hip_search_round_batch refuses about
 * groups, candidates, sets and coefficient ranges, and for everything the plan write's host-pointer form refuses about plan,
 * guards, tu_at and ent_first: an ent_first that is not non-decreasing or that ends past n_entries_total, a tu_at that decreases
 * inside a candidate or exceeds its plan length, a bad plan entry or block guard (cabac_hip_last_error names the candidate and the
 * entry, or the block).  Returns CABAC_HIP_ERR_SUBSTREAM when a candidate has a flag (see flags[]); the values and info words of
 * such a candidate are unspecified. */
int cabac_hip_search_plan_round_batch(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                      const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                      uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                      const uint32_t *plan, const uint32_t *values_in, uint64_t n_entries_total,
                                      const uint64_t *ent_first, const uint32_t *tu_at, const uint32_t *tu_guard,
                                      const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16, uint64_t *frac_bits,
                                      uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info, uint32_t *flags,
                                      uint32_t *values_out);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SEARCH_PLAN_H */
