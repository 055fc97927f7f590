/*
 * cabac_hip_plan_rows.h — the plan parse (cabac_hip_parse_plan.h) and the plan write (cabac_hip_write_plan.h) from and into
 * context sets, and over the CTU rows of pictures coded with entropy_coding_sync_enabled_flag: every row is a substream that
 * starts from the contexts the row above holds after its first CTU (CABACWriter / CABACReader synchronisation,
 * slice.hpp:176-178).  The bin codec has these calls for bin records (cabac_hip_ctx_sets.h); here they stand one layer higher,
 * on plans of syntax elements and coefficient blocks, so that a WPP picture is parsed into values and coefficients, and written
 * from a plan, on the device.  An extension of cabac_hip_parse.h, in a header of its own so that the declaration lists of the
 * other headers stay what they are.
 *
 * This header uses the plan format, CABAC_GUARD and CABAC_RES_BAD_VALUE of cabac_hip_parse_elements.h, CABAC_PE_COND /
 * CABAC_PE_BLOCK_INFO of cabac_hip_parse_plan.h, and the set format, "no set" (0xFFFFFFFF) and CABAC_RES_BAD_SET of
 * cabac_hip_ctx_sets.h, and does not repeat them: INCLUDE THOSE HEADERS FIRST (the element parse's, the plan parse's and the
 * context sets', in this order).
 *
 * THE HAND-OVER POINT — one definition for both directions.  A substream's plan has n entries; its blocks stand at the clipped
 * positions at(t) of the plan parse; the walk codes, for i = 0 .. n, first every block with at(t) == i, then entry i.  For a
 * hand-over index k, clipped to n:
 *   the hand-over contexts are the contexts the walk holds when it ARRIVES at entry k: after the entries 0 .. k - 1 and after
 *   every block with at(t) <= k — the blocks the walk codes in front of entry k, skipped ones included (they touch nothing).
 *   k >= n: after the last block of the substream.  k == 0 with no block at position 0: the start contexts.
 * In records: update() (contexts.cpp:903-913) applied to the start set for every context-coded record of the substream's expanded
 * record string (tests/parse_plan_model.py::expand) in front of that point.  The arithmetic coder's state is no part of it.
 * THE ZERO-BIN MARKER.  The hand-over index of a row names the first entry of its second CTU.  A CTU that BEGINS WITH A BLOCK has
 * no entry in front of that block, and the index of the entry behind the block would take the block along.  Such a CTU is
 * separated from its predecessor by an EP_BINS entry with numBins 0: the marker is entry k, the block stands at position k + 1.
 * The marker reads and writes no bin and touches no context; the blocks at positions up to k belong to the CTU in front.
 *
 * ---- 1. Plan parse from and into sets ---------------------------------------------------------------------------------------
 * cabac_hip_plan_parse_sets_device: the arguments of the plan parse's device form, the seven set arguments of
 * cabac_hip_ctx_sets.h (n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate) and d_out_at:
 *   d_out_at[s]   the hand-over index of substream s, in plan entries (d_out_at == NULL: the end of every substream)
 * DEFINITION OF THE RESULT
 *  - Substream s starts from set d_start_set[s]; from Ctx::init(desc.qp, desc.init_id & 3) when that is 0xFFFFFFFF or
 *    d_start_set is NULL.  One batch mixes both kinds.  The arithmetic decoder always starts fresh.
 *  - Values, coefficients, info words and results are otherwise defined exactly as for the plan parse.  With every start "no set"
 *    and d_out_set == NULL every output is bit-identical to the plan parse's device form, on any bytes.
 *  - A substream with d_out_set[s] other than 0xFFFFFFFF writes its hand-over contexts as set d_out_set[s] of d_out_state /
 *    d_out_rate: all 379 entries; the rate written is the context's window sizes (what cabac_hip_ctx_init_device writes).
 *  - An index >= n_sets (other than 0xFFFFFFFF), start or out, parses nothing for that substream: its result is
 *    {0, CABAC_RES_BAD_SET}; no value, coefficient, info word or set is written.  The check is made once per substream.
 *  - The out set is UNSPECIFIED (and everything stays memory-safe) when the substream stops with CABAC_RES_BAD_RECORD or
 *    CABAC_RES_BAD_VALUE in front of the hand-over point, and when it reports CABAC_RES_UNDERRUN: the walk learns of an underrun
 *    only at its end, when the set has been written.  CABAC_RES_BAD_STOP and CABAC_RES_RANGE do not affect the out set (a
 *    substream refused at its first byte parses nothing and hands over its start contexts).
 *  - Rates of start sets: as in cabac_hip_ctx_sets.h (they must hold what cabac_hip_ctx_init_device writes).
 * IN-PLACE RULE: as in cabac_hip_ctx_sets.h.  The out arrays may be the start arrays; an out set may be the substream's own start
 * set, provided no other substream of the call starts from it; it must not be another substream's start set or out set.  (Every
 * substream reads its start set before it parses; no substream waits for another.)
 * The call is asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h; it needs no library scratch and
 * no host wait, and no kernel waits for another workgroup.
 *
 * ---- 2. Rows parsed -----------------------------------------------------------------------------------------------------------
 * cabac_hip_plan_parse_rows_device: the arguments of the plan parse, then
 *   n_level, level_first   LEVEL ORDER, exactly as in cabac_hip_ctx_sets.h: the descriptors are sorted so that level l is the range
 *                          [level_first[l], level_first[l + 1]); level_first is HOST memory, n_level + 1 entries, non-decreasing,
 *                          level_first[0] = 0, level_first[n_level] = n_sub.  Row r of every picture in flight is level r.
 *   d_sync_from[s]         0xFFFFFFFF (substream s starts from Ctx::init), or the index of a substream in an EARLIER level
 *   d_sync_at[p]           the hand-over index of substream p, in plan entries (device memory)
 * Substream s starts from the hand-over contexts of substream d_sync_from[s]; everything else is as for the plan parse.  With one
 * level and no link the outputs are the plan parse's.
 * The call is a schedule of ordinary launches on the ctx stream with no host wait inside and no kernel that waits for another
 * workgroup: for every non-empty level ONE launch of the kernel of part 1 over that level's substreams; each substream starts
 * from the slot of its link in a ctx-owned scratch of n_sub sets and writes its own slot at its hand-over point; the last level
 * writes none.  Every substream is parsed exactly once — no prefix is parsed twice.
 * Links are checked on the device: a link that does not point into an earlier level gives {0, CABAC_RES_BAD_SET} for the
 * substream that has it, which parses nothing; substreams linked to it parse from unspecified contexts; nothing out of bounds is
 * touched.  A row that stops or underruns in front of its hand-over point hands over unspecified contexts.
 * cabac_hip_plan_parse_rows_batch: the host-pointer form (synchronous), everything in host memory, staged as the plan parse's
 * host-pointer form stages it, in ONE chunk.  It returns CABAC_HIP_ERR_INVALID, with nothing run and no output touched, for
 * everything that form refuses, and, with cabac_hip_last_error naming the substream, for a level_first that is not non-decreasing
 * from 0 to n_sub, a link into the same or a later level, or a link >= n_sub; CABAC_HIP_ERR_SUBSTREAM when a result flag is set.
 *
 * ---- 3. Plan write from sets and in rows --------------------------------------------------------------------------------------
 * cabac_hip_plan_write_sets_device: the arguments of the plan write's device form and the seven set arguments, over the substreams
 * of the call.  Substream s is coded from set d_start_set[s]; the out set is the contexts after the last record of its expanded
 * string.  A stopped substream (CABAC_RES_BAD_VALUE / CABAC_RES_BAD_RECORD) writes no set; an index >= n_sets gives
 * {0, CABAC_RES_BAD_SET} and no payload byte for that substream.  With every start "no set" and d_out_set == NULL the payload, the
 * offsets, the results, the filled values and the info words are bit-identical to the plan write's.
 * cabac_hip_plan_write_rows_device / cabac_hip_plan_write_rows_batch: the plan write plus n_level, level_first (HOST memory),
 * d_sync_from and d_sync_at (plan entries), as in part 2.  Substream s is coded from the hand-over contexts of d_sync_from[s]: the
 * emit walk of the plan write notes, per substream, the index into its expanded record string that corresponds to its hand-over
 * point (the records of the coded blocks in front of it counted), and the WPP encode schedule of cabac_hip_ctx_sets.h — the
 * context-advance prefix passes per level, then one encode launch — takes the encode launch's place with that index.  What these
 * calls write, the rows parse reads back with the same plan, levels and links.  The device form still waits for the ctx's stream
 * ONCE in the middle, as the plan write does; the payload, the offsets, the filled values, the info words and the results are as
 * there.  A stopped row hands over unspecified contexts.  The batch form refuses what the plan write's host-pointer form refuses
 * and what part 2's refuses about level_first and links.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 34, "plan parse with
 * sets"; kind 35, "a level of a rows parse" (one entry per level launch); kind 36, "the encode launch of a plan write with sets".
 * The other kernels of the writing calls report as they do in the plan write and in the WPP encode call.
 */
#ifndef CABAC_HIP_PLAN_ROWS_H
#define CABAC_HIP_PLAN_ROWS_H

#include "cabac_hip_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

int cabac_hip_plan_parse_sets_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                     const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                     const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                     uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                     const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, const uint32_t *d_out_at);

int cabac_hip_plan_parse_rows_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                     const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                     const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                     uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_level,
                                     const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at);
int cabac_hip_plan_parse_rows_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                    uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                                    const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                                    int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                                    cabac_substream_result *results, uint32_t n_level, const uint32_t *level_first,
                                    const uint32_t *sync_from, const uint32_t *sync_at);

int cabac_hip_plan_write_sets_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                     const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                     const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                     uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                     cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                     const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate);
int cabac_hip_plan_write_rows_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                     const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                     const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                     uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                     cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_level,
                                     const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at);
int cabac_hip_plan_write_rows_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *plan,
                                    const uint32_t *values_in, uint64_t n_elements_total, const uint32_t *tile_first,
                                    const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard, const void *coeff,
                                    int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                                    uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *values_out, uint32_t *tu_info,
                                    uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PLAN_ROWS_H */
