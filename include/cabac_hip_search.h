/*
 * cabac_hip_search.h — C ABI of the search rounds of libcabac_hip.so: cost a batch of candidates, keep the cheapest of every
 * group and carry the contexts it leaves, all on the device.  An extension of cabac_hip.h and cabac_hip_estimate.h (same
 * conventions: plain pointers and sizes, 0 or a negative cabac_hip_status, no exception crosses the boundary), kept in a header
 * of its own: the reference-side test libraries (oracle/Makefile) are pinned to the content of cabac_hip.h, and nothing declared
 * here changes what they were compiled against.
 *
 * Replace: what a rate-distortion search does around getCABACEstimator()->residual_coding(...) / getEstFracBits() for every
 * position — compare D + lambda * R of the alternatives, and go on from the winner's contexts (Ctx::operator=, contexts.hpp:254,
 * contexts.cpp:1096, between the estimator and the saved contexts; the TempCtx save-and-restore).  cabac_hip_estimate_residual_device
 * gives R for one flat batch and leaves the sets unmodified; the calls below close the loop, so that a caller's transform /
 * quantisation kernels and this library's costing alternate on ONE stream with no host round trip between positions.
 *
 * Context sets are in the format of cabac_hip_ctx_init_device and cabac_hip_estimate_from_device everywhere: 379 entries per
 * set, m_state[0] | m_state[1] << 16 in d_state, m_rate in d_rate.
 *
 * DEFINITION OF THE RESULT.
 *   THE SET A CANDIDATE LEAVES.  Start from the candidate's start set.  For every block of the candidate, in order, take the
 *   records cabac_hip_residual_device produces for it and apply update() (contexts.cpp:903-913) for every context-coded record.
 *   A block flagged CABAC_TU_INFO_EMPTY or CABAC_TU_INFO_BAD_DESC leaves the contexts alone, as it does for the cost; a candidate
 *   with no blocks leaves a copy of its start set.  All 379 entries are written: those residual coding cannot touch (0..85,
 *   292..309, 312..356) are copied from the start set.
 *   THE COST.  cost(c) = d_dist[c] + ((lambda_q16 * d_frac_bits[c]) >> 31): the product taken in 128 bits and floored, the sum
 *   saturating at 2^64 - 2.  lambda_q16 is lambda in distortion units per bit with 16 fractional bits; the other 15 bits of the
 *   shift are SCALE_BITS of d_frac_bits.  d_dist == NULL reads as all zeros, so lambda_q16 = 1 << 31 then compares plain
 *   frac_bits.  A candidate with d_dist[c] == UINT64_MAX is excluded.
 *   THE PICK.  A GROUP g is the run of candidates [d_group_first[g], d_group_first[g + 1]) (n_group + 1 entries, the shape of
 *   d_cand_first).  d_pick[g] is the candidate of the group with the smallest cost, the lowest index among equals; d_cost[g] its
 *   cost.  An empty group, or one with every candidate excluded, gives d_pick[g] = CABAC_SEARCH_NONE and d_cost[g] = UINT64_MAX.
 *
 * IN-PLACE RULE.  The sets a call writes live in arrays that may be the arrays the start sets are read from.  A set that is
 * written (group g's out set; for cabac_hip_estimate_residual_ctx_device every candidate is a group of its own)
 *   - may be a set that candidates of group g start from,
 *   - must not be a start set of any candidate of another group in the same call,
 *   - must not be another group's out set.
 * With that, K chains that each own one set (a CTU row, a tile, a substream) advance in place, round after round, with no extra
 * storage and no copies.  The device forms do not see a violation (the result of the sets involved is then undefined, nothing
 * else is touched); the host form refuses it.
 *
 * All device forms are asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host
 * synchronisation inside, the scratch belongs to the ctx, no kernel waits on another workgroup.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed there, in cabac_hip_estimate.h and in
 * cabac_hip_nal.h: kind 15, "residual estimate with contexts" (cabac_hip_estimate_residual_ctx_device / _ctx16_device),
 * kind 16, "search select" (cabac_hip_search_select_device, and the select part of a round), kind 17, "search round
 * estimate", and kind 18, "search round commit" — a round reports its three parts as 17, 16, 18 in this order.
 */
#ifndef CABAC_HIP_SEARCH_H
#define CABAC_HIP_SEARCH_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_SEARCH_NO_SET 0xFFFFFFFFu /* d_out_set / d_group_out_set entry: write no set */
#define CABAC_SEARCH_NONE 0xFFFFFFFFu   /* d_pick entry: the group has no candidate to pick */

/* ---- 1. the contexts a candidate leaves ----
 * Every argument of cabac_hip_estimate_residual_device with the same results in d_frac_bits, d_tu_frac_bits and d_tu_info, plus:
 * candidate c with d_out_set[c] != CABAC_SEARCH_NO_SET writes the set it leaves (see above) as set d_out_set[c] of d_out_state /
 * d_out_rate; one with CABAC_SEARCH_NO_SET writes nothing.  The output arrays may be the input arrays under the in-place rule.
 * Two candidates naming the same out set is the caller's error. */
int cabac_hip_estimate_residual_ctx_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first,
                                           const cabac_tu_desc *d_tu, const int32_t *d_coeff, const uint32_t *d_state,
                                           const uint8_t *d_rate, const uint32_t *d_set, uint64_t *d_frac_bits,
                                           uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, const uint32_t *d_out_set,
                                           uint32_t *d_out_state, uint8_t *d_out_rate);
/* The same with the coefficients as int16_t, as cabac_hip_estimate_residual16_device */
int cabac_hip_estimate_residual_ctx16_device(cabac_hip_ctx *ctx, uint32_t n_cand, const uint32_t *d_cand_first,
                                             const cabac_tu_desc *d_tu, const int16_t *d_coeff, const uint32_t *d_state,
                                             const uint8_t *d_rate, const uint32_t *d_set, uint64_t *d_frac_bits,
                                             uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, const uint32_t *d_out_set,
                                             uint32_t *d_out_state, uint8_t *d_out_rate);

/* ---- 2. pick the cheapest of each group ----
 * A segmented arg-min: groups of any size (0 to many thousands), no host-known maximum.  d_group_first[n_group] is read on the
 * device; a run that goes backwards or past it is clipped, as the estimator clips d_cand_first.  d_dist may be NULL. */
int cabac_hip_search_select_device(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *d_group_first,
                                   const uint64_t *d_frac_bits, const uint64_t *d_dist, uint64_t lambda_q16, uint32_t *d_pick,
                                   uint64_t *d_cost);

/* ---- 3. one round in one call: estimate, select, commit ----
 * Costs the n_cand candidates as cabac_hip_estimate_residual_device does (coeff_bytes 4: int32_t, 2: int16_t; d_set[c] per
 * candidate; d_frac_bits, and d_tu_frac_bits / d_tu_info if not NULL), picks per group as cabac_hip_search_select_device does,
 * and writes the set the picked candidate of group g leaves as set d_group_out_set[g] of d_state / d_rate — the arrays the start
 * sets live in — unless d_group_out_set[g] is CABAC_SEARCH_NO_SET or d_pick[g] is CABAC_SEARCH_NONE (then nothing is written for
 * g).  d_group_out_set may be NULL: no set is written.  n_cand is the host-known candidate count that sizes the grid;
 * d_group_first[n_group] is read on the device and clipped to n_cand.
 * The commit walks only the picked candidates a second time (about 1 / G of the estimate with G candidates per group), with
 * the exporting kernel of part 1.  Each start set is read before any write to it can land: the estimate pass has finished by
 * stream order, and the commit's kernel fills its local store from the start set, passes a barrier, and stores only at its end —
 * which under the in-place rule makes "group g's out set is one of its own start sets" safe. */
int cabac_hip_search_round_device(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                  const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                  uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set, const uint32_t *d_group_out_set,
                                  const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                  uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info);

/* ---- 4. host-pointer form (synchronous) ----
 * The same round on host arrays, staged through the ctx like cabac_hip_estimate_residual_batch: coeff holds n_coeff_total
 * coefficients of coeff_bytes bytes each; state / rate hold n_sets context sets and come back with the written sets updated;
 * tus holds cand_first[n_cand] blocks; group_out_set, dist, tu_frac_bits and tu_info may be NULL.
 * Returns CABAC_HIP_ERR_INVALID with nothing run and no output touched for: a group_first or cand_first that is not
 * non-decreasing, group_first[n_group] != n_cand, a set[c] or an out set (other than CABAC_SEARCH_NO_SET) >= n_sets, a block
 * whose coefficients do not lie inside n_coeff_total, two groups naming the same out set, and a violation of the in-place rule
 * (cabac_hip_last_error names it).  Returns CABAC_HIP_ERR_SUBSTREAM as cabac_hip_estimate_residual_batch does when a block of a
 * candidate is empty or has a bad descriptor (tu_info says which; every result still arrives). */
int cabac_hip_search_round_batch(cabac_hip_ctx *ctx, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                 const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                 uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                 const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16, uint64_t *frac_bits,
                                 uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SEARCH_H */
