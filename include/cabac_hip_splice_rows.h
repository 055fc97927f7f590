/*
 * cabac_hip_splice_rows.h — the splice pipeline (cabac_hip_encode_residual_device, cabac_hip.h) and the winner log's emit
 * (cabac_hip_search_emit.h) from and into context sets, and over the CTU rows of pictures coded with
 * entropy_coding_sync_enabled_flag: every row is a substream that starts from the contexts the row above holds after its first CTU
 * (CABACWriter synchronisation, slice.hpp:176-178).  The bin codec has these calls for bin records (cabac_hip_ctx_sets.h) and the
 * plan write has them for plans (cabac_hip_plan_rows.h); here they stand on the path a rate-distortion search takes from its
 * decisions to bytes: host records with coefficient blocks spliced in, and the log of the winners.  In a header of its own so that
 * the declaration lists of the other headers stay what they are.
 *
 * This header uses the splice format of cabac_hip.h, the log of cabac_hip_search_emit.h (included below), and the set format, "no
 * set" (0xFFFFFFFF), the rate rule and CABAC_RES_BAD_SET of cabac_hip_ctx_sets.h, and does not repeat them: INCLUDE THAT HEADER
 * FIRST (the context sets').  Every call takes the coefficients as const void *d_coeff with coeff_bytes 4 (int32_t) or 2 (int16_t);
 * another coeff_bytes returns CABAC_HIP_ERR_INVALID.
 *
 * THE HAND-OVER POINT — one definition for every call below.  Substream p has n host records; its splices are sorted by `at`; its
 * EXPANDED STRING is, for i = 0 .. n: first every block spliced at at == i, in the order of the list, then host record i (there is
 * no host record n).  A hand-over point is a PAIR:
 *   d_sync_at[p]      = k host records in front, clipped to n;
 *   d_sync_splice[p]  = the number of p's splices in front, clipped to [#{at < k}, #{at <= k}].
 * d_sync_splice == NULL means the upper end everywhere: every block at a position up to k goes in front — the rule of the plan
 * rows.  The LOWER END is what a CTU that begins with a block needs: the blocks spliced at position k belong to the CTU behind the
 * point.  (A record string has no place for the zero-bin marker that the plan rows use for this.)  k >= n with the upper end is the
 * end of the substream; k == 0 with the lower end is its start.
 * The hand-over contexts are update() (contexts.cpp:903-913) applied to the start set for every context-coded record of the expanded
 * string in front of that point.  Empty, bad-descriptor and rejected blocks contribute nothing: they have no records.  The
 * arithmetic coder's state is no part of it.
 *
 * ---- 1. The splice pipeline from and into sets ---------------------------------------------------------------------------------
 * cabac_hip_encode_residual_sets_device: the arguments of cabac_hip_encode_residual_device in the const void * / coeff_bytes form,
 * then the seven set arguments (n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate).
 * DEFINITION OF THE RESULT
 *  - Substream s is coded from set d_start_set[s]; from Ctx::init(desc.qp, desc.init_id & 3) when that is 0xFFFFFFFF or
 *    d_start_set is NULL.  One batch mixes both kinds.  The arithmetic coder always starts fresh.
 *  - A substream with d_out_set[s] other than 0xFFFFFFFF writes the contexts after the LAST record of its expanded string as set
 *    d_out_set[s] of d_out_state / d_out_rate: all 379 entries, rates as cabac_hip_ctx_init_device writes them.  A substream with no
 *    records and no splices writes a copy of its start set.
 *  - An index >= n_sets (other than 0xFFFFFFFF), start or out, codes nothing for that substream: its result is
 *    {0, CABAC_RES_BAD_SET}, it has no payload byte (its two offsets are equal) and writes no set.
 *  - With every start "no set" and d_out_set == NULL the payload, the offsets, the results, tu_info and bin_counts are bit-identical
 *    to the plain call's.
 * IN-PLACE RULE, rate rule: as in the sets calls of the bin codec.  The out arrays may be the start arrays; an out set may be the
 * substream's own start set provided no other substream of the call starts from it.
 * The call still waits for the ctx's stream ONCE in the middle, as the plain call does, and refuses what it refuses.
 *
 * ---- 2. Spliced rows -----------------------------------------------------------------------------------------------------------
 * cabac_hip_encode_residual_rows_device: the plain call's arguments (const void * / coeff_bytes), then
 *   n_level, level_first   LEVEL ORDER, exactly as in the WPP encode of the bin codec: the descriptors are sorted so that level l is
 *                          the range [level_first[l], level_first[l + 1]); level_first is HOST memory, n_level + 1 entries,
 *                          non-decreasing, level_first[0] = 0, level_first[n_level] = n_sub.  Row r of every picture is level r.
 *   d_sync_from[s]         0xFFFFFFFF (substream s starts from Ctx::init), or the index of a substream in an EARLIER level
 *   d_sync_at, d_sync_splice   the hand-over pair of every substream (device memory; d_sync_splice may be NULL)
 * Substream s is coded from the hand-over contexts of substream d_sync_from[s]; everything else is the plain call's.  With one
 * level and no link every output is bit-identical to the plain call's.
 * After the block-records pass one kernel turns every substream's pair into an index into its expanded string — two bisections of
 * the substream's sorted splices and the running sums of the splice plan; no atomics, no waiting for another workgroup — and the
 * WPP encode schedule takes the encode launch's place: one context-advance launch per non-final level over the rows cut at that
 * index, writing ctx-owned slots, then ONE encode launch of all rows from their slots.  There is NO SECOND HOST WAIT.
 * Links are checked on the device as there: a link that does not point into an earlier level gives {0, CABAC_RES_BAD_SET} and no
 * payload byte for the substream that has it; substreams linked to it are coded from unspecified contexts; nothing out of bounds
 * is touched.
 * cabac_hip_encode_residual_rows_batch: the host-pointer form (synchronous), everything in host memory (sync_splice may be NULL),
 * staged as ONE chunk.  It returns CABAC_HIP_ERR_INVALID, with nothing run and no output touched, for everything the plain
 * host-pointer form refuses on the host and, with cabac_hip_last_error naming the substream, for a level_first that is not
 * non-decreasing from 0 to n_sub, a link into the same or a later level, or a link >= n_sub.  (Coefficients out of range and a
 * damaged splice list are found by the device as in the plain form: CABAC_HIP_ERR_INVALID too, no output touched, nothing coded.)
 * sync_from, sync_at and sync_splice hold n_sub words each:
 * the C form cannot see a shorter array; the Python binding refuses one the same way.  CABAC_HIP_ERR_SUBSTREAM when a result flag is
 * set or a block is empty or badly described.
 *
 * ---- 3. Marks in the winner log ------------------------------------------------------------------------------------------------
 * cabac_hip_search_log_mark_device(log, n, d_chain): asynchronous on the ctx's stream, no host wait, no allocation.  For each of
 * the n listed chains the log notes its present cursors — side records so far, blocks so far — as that chain's hand-over pair.
 * Issued after the append of a row's first CTU, the mark is the point the row below starts from; the pair is always consistent,
 * because a later entry's blocks stand at or behind the records in front of it.  A later mark of the same chain REPLACES the
 * earlier one; cabac_hip_search_log_reset_device clears every mark to "end of chain"; an unmarked chain hands over its final
 * contexts.  A chain index >= n_chain (0xFFFFFFFF included) is skipped.  A mark after an append that was dropped for capacity marks
 * the unchanged cursors.  The marks are two per-chain words inside the log: the view and the two pinned structs do not change.
 *
 * ---- 4. The log's emit from sets and in rows -----------------------------------------------------------------------------------
 * cabac_hip_search_log_encode_sets_device: the log's emit with the seven set arguments over the chains (chain k is substream k), as
 * in part 1.  cabac_hip_search_log_encode_rows_device: the log's emit with n_level, level_first (HOST memory) and d_sync_from as in
 * part 2; the chains are in level order and the hand-over pair of a chain is its mark.  With no sets, respectively one level and
 * no link, every output is bit-identical to the plain emit's.  Both WAIT FOR THE STREAM TWICE, as that call does, and refuse an
 * overflowed log as it does.  The log is not consumed.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 37, "hand-over index"
 * (the kernel of part 2); kind 38, "log mark"; kind 39, "the encode launch of a spliced call with sets".  The other kernels report
 * as they do in the plain calls and in the WPP encode.
 */
#ifndef CABAC_HIP_SPLICE_ROWS_H
#define CABAC_HIP_SPLICE_ROWS_H

#include "cabac_hip_search_emit.h"

#ifdef __cplusplus
extern "C" {
#endif

int cabac_hip_encode_residual_sets_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                          const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                          const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes, uint8_t *d_payload,
                                          uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                          uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_sets, const uint32_t *d_state,
                                          const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                          uint32_t *d_out_state, uint8_t *d_out_rate);

int cabac_hip_encode_residual_rows_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                          const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                          const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes, uint8_t *d_payload,
                                          uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                          uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_level, const uint32_t *level_first,
                                          const uint32_t *d_sync_from, const uint32_t *d_sync_at, const uint32_t *d_sync_splice);
int cabac_hip_encode_residual_rows_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                         uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                         const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                                         uint8_t *payload, uint64_t payload_capacity, uint64_t *payload_offsets,
                                         cabac_substream_result *results, uint32_t *tu_info, uint32_t *bin_counts, uint32_t n_level,
                                         const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at,
                                         const uint32_t *sync_splice);

int cabac_hip_search_log_mark_device(cabac_search_log *log, uint32_t n, const uint32_t *d_chain);

int cabac_hip_search_log_encode_sets_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                            uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                            uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_sets, const uint32_t *d_state,
                                            const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                            uint32_t *d_out_state, uint8_t *d_out_rate);
int cabac_hip_search_log_encode_rows_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                            uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                            uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_level, const uint32_t *level_first,
                                            const uint32_t *d_sync_from);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SPLICE_ROWS_H */
