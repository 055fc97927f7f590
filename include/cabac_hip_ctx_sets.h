/*
 * cabac_hip_ctx_sets.h — the bin codec from and into context sets, and WPP substreams on top of it.
 *
 * cabac_hip_encode_device / cabac_hip_decode_device (cabac_hip.h) start every substream from Ctx::init(qp, init_id) and do
 * not say what contexts they leave.  The calls below take and give context sets — 379 entries, m_state[0] | m_state[1] << 16
 * in d_state and m_rate in d_rate, the format of cabac_hip_ctx_init_device and of every other call that reads or writes sets —
 * so that a substream can start where another one stood: the contexts a search chain owns, a set brought up to date from the
 * records that were really coded, and the hand-over between the CTU rows of a picture under entropy_coding_sync_enabled_flag
 * (every CTU row is a substream that starts from the contexts the row above has after its first CTU: CABACWriter /
 * CABACReader synchronisation, slice.hpp:176-178; Ctx::operator=, contexts.hpp:254).
 *
 * Profile kinds (cabac_hip_profile_read): kind 30 encode with sets, kind 31 decode with sets, kind 32 context advance,
 * kind 33 the prefix passes of a WPP call (one entry per level launch; the final pass of a WPP call is a kind 30 / kind 31 entry).
 */
#ifndef CABAC_HIP_CTX_SETS_H
#define CABAC_HIP_CTX_SETS_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_CTX_NO_SET 0xFFFFFFFFu
#define CABAC_RES_BAD_SET 0x40u /* a start or out set index >= n_sets: the substream codes nothing */

/* ---- 1. sets in, sets out (device pointers, asynchronous on the ctx stream) ------------------------------------------
 * The seven set arguments, the same for the three calls:
 *   n_sets                    the number of sets d_state / d_rate and d_out_state / d_out_rate hold (379 entries each per set)
 *   d_state, d_rate           the start sets
 *   d_start_set[s]            the set substream s starts from, or CABAC_CTX_NO_SET (d_start_set == NULL: all of them so)
 *   d_out_set[s]              the set substream s writes, or CABAC_CTX_NO_SET (d_out_set == NULL: all of them so)
 *   d_out_state, d_out_rate   where out sets are written (may be NULL when d_out_set is)
 *
 * DEFINITION OF THE RESULT
 *  - Substream s starts from set d_start_set[s]; if that is CABAC_CTX_NO_SET, from Ctx::init(desc.qp, desc.init_id & 3).
 *    One batch mixes both kinds.  The arithmetic coder always starts fresh (start(), arith_codec.cpp:329-337 / :60-66).
 *  - Bytes, n_bits, flags and bins are otherwise defined exactly as for cabac_hip_encode_device / cabac_hip_decode_device.
 *    With every start set CABAC_CTX_NO_SET and d_out_set == NULL the results are bit-identical to those calls.
 *  - A substream with d_out_set[s] != CABAC_CTX_NO_SET writes the contexts it has after its last record as set d_out_set[s]
 *    of d_out_state / d_out_rate: all 379 entries; the rate written is the context's window sizes (what
 *    cabac_hip_ctx_init_device writes for that context).
 *  - n_records == 0 writes a copy of the start set (the init set when the start is CABAC_CTX_NO_SET).
 *  - d_out_set == NULL: nothing is written.  A substream whose out set is CABAC_CTX_NO_SET touches no set.
 *  - A substream with CABAC_RES_BAD_RECORD or CABAC_RES_UNDERRUN leaves its out set unspecified and touches nothing else.
 *  - An index >= n_sets (other than CABAC_CTX_NO_SET), start or out, codes nothing for that substream: its result is
 *    {0, CABAC_RES_BAD_SET}, no set is written, no byte, no bin, and no memory outside the arguments is touched.  The check is
 *    made once per substream.
 *  - Rates: the window sizes of a context depend on the context id only (the fourth row of the init table).  A start set's
 *    d_rate must hold what cabac_hip_ctx_init_device writes; every set this library writes does.  With other rates the calls
 *    are undefined but memory-safe.
 *
 * IN-PLACE RULE: the out arrays may be the start arrays.  An out set may be the substream's own start set, provided no other
 * substream of the call starts from it; it must not be another substream's start set or out set.  (Every substream reads its
 * start set before it codes and writes its out set behind its last record; no substream waits for another.)
 *
 * The calls go through the dispatch of the plain calls (cabac_hip_set_variant; the geometry chosen by batch size, for the
 * decoder on the device): every geometry takes sets.
 */
int cabac_hip_encode_sets_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_sets, const uint32_t *d_state,
                                 const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set, uint32_t *d_out_state,
                                 uint8_t *d_out_rate);
int cabac_hip_decode_sets_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_sets,
                                 const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                 const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate);
/* Context advance: update() (contexts.cpp:903-913) for every context-coded record of the run, in order, on the start set; EP,
 * TRM and ALIGN records are passed over; any other id is rejected (CABAC_RES_BAD_RECORD in d_flags[s], the out set then
 * unspecified).  Nothing is coded: only rec_offset, n_records, qp and init_id of the descriptors are read.  d_flags (may be
 * NULL) receives 0, CABAC_RES_BAD_RECORD or CABAC_RES_BAD_SET per substream.  Brings a set up to date from the records of a
 * substream that has been coded.                                                                                          */
int cabac_hip_ctx_advance_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 uint32_t n_sets, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                 const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, uint32_t *d_flags);

/* ---- 2. WPP: substreams that start from another substream's contexts --------------------------------------------------
 * LEVEL ORDER: the descriptors are sorted so that level l is the range [level_first[l], level_first[l + 1]) (level_first: HOST
 * memory, n_level + 1 entries, non-decreasing, level_first[0] = 0, level_first[n_level] = n_sub).  Row r of every picture in
 * flight is level r; a substream links only into an EARLIER level.
 *   d_sync_from[s]   CABAC_CTX_NO_SET (substream s starts from Ctx::init), or the index of a substream in an earlier level
 *   d_sync_at[p]     the number of records of substream p after which its contexts are handed over, clipped to its n_records;
 *                    0 hands over p's own start contexts.  Device memory: the records may have been produced on the device.
 * Substream s starts from the contexts d_sync_from[s] has after its first d_sync_at[d_sync_from[s]] records; the arithmetic
 * coder starts fresh, as always.  Everything else is as for cabac_hip_encode_device / cabac_hip_decode_device.
 *
 * The call is a schedule of ordinary launches on the ctx stream with no host wait inside and no kernel that waits for
 * another workgroup: for every level but the last one launch over the level's substreams cut to their first sync_at records
 * (encode: the context advance; decode: the sets decoder — the bins are not known until decoded), each writing its contexts
 * to a slot of a ctx-owned scratch (slot = substream index), then one launch of all n_sub substreams from their slots.  When
 * the call's work completes the caller's buffers hold the results of that last launch only.
 * A link that does not point into an earlier level makes the substream that has it code nothing: {0, CABAC_RES_BAD_SET};
 * substreams that link to it code from unspecified contexts; nothing out of bounds is touched.                              */
int cabac_hip_encode_wpp_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_level, const uint32_t *level_first,
                                const uint32_t *d_sync_from, const uint32_t *d_sync_at);
int cabac_hip_decode_wpp_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_level,
                                const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at);
/* Host-pointer forms (synchronous): everything in host memory, staged as cabac_hip_encode_batch / cabac_hip_decode_batch stage
 * it but as ONE chunk (chunks would cut links).  They return CABAC_HIP_ERR_INVALID, with nothing run and cabac_hip_last_error
 * naming the substream, for a level_first that is not non-decreasing from 0 to n_sub, a link into the same or a later level,
 * or a link >= n_sub; CABAC_HIP_ERR_SUBSTREAM when a result flag is set.                                                   */
int cabac_hip_encode_wpp_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total, cabac_substream_result *results,
                               uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at);
int cabac_hip_decode_wpp_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total, uint8_t *bins,
                               cabac_substream_result *results, uint32_t n_level, const uint32_t *level_first,
                               const uint32_t *sync_from, const uint32_t *sync_at);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_CTX_SETS_H */
