/*
 * cabac_hip_search_emit.h — C ABI of the winner log: the candidates a rate-distortion search picked, kept on the device round by
 * round and coded into substreams at the end.  An extension of cabac_hip_search_unit.h (same conventions, same candidate format,
 * same clipping), kept in a header of its own so that the declaration lists of the other headers stay what they are.
 *
 * Replace: what the encoder does with the alternative it chose — it runs the CABACWriter once more over the winner, this time on the
 * real bin encoder.  A round of cabac_hip_search_unit_round_device answers d_pick[g], an index into that round's candidate arrays,
 * which the next position overwrites.  The log COPIES the picked candidates (side records, block descriptors, block positions and
 * coefficients) behind one another on the device, with no host round trip between positions, and cabac_hip_search_log_encode_device
 * hands the whole to the pipeline of cabac_hip_encode_residual_device.  The logged coefficients are also what the caller's
 * reconstruction kernels need next: cabac_hip_search_log_view shows them.
 *
 * DEFINITION OF THE RESULT.
 *   A CHAIN of context sets (a CTU row, a tile, a substream) is the unit that owns one coded substream; a log has n_chain of them.
 *   APPEND.  Group g of a call appends nothing when d_pick[g] == CABAC_SEARCH_NONE, d_pick[g] >= n_cand, d_group_chain[g] ==
 *   CABAC_SEARCH_NO_CHAIN or d_group_chain[g] >= n_chain.  Every other group appends one ENTRY for candidate c = d_pick[g], in
 *   group order, behind the entries the log holds:
 *     its side run d_records[d_rec_first[c] .. d_rec_first[c + 1]), clipped exactly as cabac_hip_search_unit.h clips it (n_rec
 *     records); its blocks d_tu[d_cand_first[c] .. d_cand_first[c + 1]), clipped the same way (n_tu blocks);
 *     for each block its EFFECTIVE position at(t) = min(max(d_tu_at[t], at(t - 1)), n_rec), 0 in front of the first block
 *     (d_tu_at == NULL: every block behind the run, at(t) = n_rec) — the log stores at(t), not d_tu_at[t];
 *     for each block its w * h coefficients, the blocks of an entry behind one another, and its descriptor with coeff_offset REBASED
 *     to where the coefficients lie in the log's coefficient array.  A block with log2_width or log2_height above 6 copies no
 *     coefficient and keeps the rest of its descriptor (its coeff_offset is where its coefficients would have started).
 *   An entry with no record and no block is legal.  d_records may be NULL when every run is empty.
 *   ONE GROUP PER CHAIN: within one call a chain may be named by at most one appending group — the IN-PLACE RULE of
 *   cabac_hip_search.h seen from the log (one group per chain per round).  The device form cannot see a violation: that chain's log
 *   is then undefined (encoding it may return CABAC_HIP_ERR_INVALID), and nothing else is touched or overrun.
 *   CAPACITY: A CALL IS ALL OR NOTHING.  If the entries, records, blocks or coefficients of a call do not all fit the capacities the
 *   log was created with, or a chain's record count would pass 2^32 - 1, NOTHING of the call is appended: counters and arrays stay
 *   as they were, and the sticky flag CABAC_SEARCH_LOG_OVERFLOW is set in the log's counters together with one
 *   CABAC_SEARCH_LOG_OVER_* bit per capacity that was too small.  The call still returns CABAC_HIP_OK: it cannot know.
 *   EMIT.  The substream of chain k is the concatenation, in append order, of the EXPANDED STRINGS (cabac_hip_search_unit.h) of the
 *   chain's entries, coded from cabac's start state for (d_desc[k].qp, d_desc[k].init_id).  payload, offsets, results, tu_info (one
 *   word per LOGGED block, in log order) and bin_counts are exactly what cabac_hip_encode_residual_device gives for that record
 *   string and those splices.  A chain with no entries is an empty record string.  As there, only the top-left 32 x 32 of a 64-wide
 *   or 64-tall block is coded (cabac_hip.h); the log holds all w * h coefficients, and what lies outside that region is the
 *   caller's to keep zero, as the codec does.
 *
 * HEAD AND TAIL SYNTAX (slice-start records, the terminate bin of end_of_slice, ...) is appended the same way: a group with ONE
 * candidate that has side records and no blocks, whose d_pick points at that candidate.
 *
 * cabac_hip_search_log_reset_device and cabac_hip_search_log_append_device are asynchronous on the ctx's stream under the STREAM
 * ORDERING CONTRACT of cabac_hip.h: no host synchronisation inside, appends never allocate (the scratch of a call depends on
 * n_group only and belongs to the ctx), no kernel waits on another workgroup.
 * cabac_hip_search_log_encode_device WAITS FOR THE STREAM TWICE: once for the log's counters (they size the launches), then once
 * inside the pipeline of cabac_hip_encode_residual_device, as that call does.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 23, "log append"
 * (the three launches of cabac_hip_search_log_append_device), and kind 24, "log place" (the front of
 * cabac_hip_search_log_encode_device; the kinds of cabac_hip_encode_residual_device follow it).
 */
#ifndef CABAC_HIP_SEARCH_EMIT_H
#define CABAC_HIP_SEARCH_EMIT_H

#include "cabac_hip_search_unit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_SEARCH_NO_CHAIN 0xFFFFFFFFu /* d_group_chain[g]: the group's winner is not logged */

/* cabac_search_log_counters.flags */
#define CABAC_SEARCH_LOG_OVERFLOW 0x1u            /* a call did not fit and was dropped as a whole (sticky until reset) */
#define CABAC_SEARCH_LOG_OVER_ENTRIES 0x10u       /* ... because of entry_capacity                                      */
#define CABAC_SEARCH_LOG_OVER_RECORDS 0x20u       /* ... record_capacity                                                */
#define CABAC_SEARCH_LOG_OVER_BLOCKS 0x40u        /* ... tu_capacity                                                    */
#define CABAC_SEARCH_LOG_OVER_COEFFS 0x80u        /* ... coeff_capacity                                                 */
#define CABAC_SEARCH_LOG_OVER_CHAIN_RECORDS 0x100u /* ... a chain's record count would pass 2^32 - 1                    */

typedef struct cabac_search_log cabac_search_log;

typedef struct cabac_search_log_counters {
  uint64_t n_entry;  /* entries in the log                 */
  uint64_t n_record; /* side records in the log            */
  uint64_t n_tu;     /* blocks in the log                  */
  uint64_t n_coeff;  /* coefficients in the log            */
  uint32_t flags;    /* CABAC_SEARCH_LOG_*                 */
  uint32_t reserved;
} cabac_search_log_counters;

typedef struct cabac_search_log_entry {
  uint64_t rec_first;       /* its first side record in the log's records                       */
  uint32_t chain;           /* the chain it belongs to                                          */
  uint32_t n_rec;           /* side records                                                     */
  uint32_t n_tu;            /* blocks                                                           */
  uint32_t tu_first;        /* its first block in the log's descriptors / positions             */
  uint32_t chain_rec_first; /* side records of its chain's entries in front of it               */
  uint32_t chain_tu_first;  /* blocks of its chain's entries in front of it                     */
} cabac_search_log_entry;

/* const device pointers into the log (valid until the log is destroyed) and what it was created with; read them on the ctx's
 * stream, or after synchronising with it */
typedef struct cabac_search_log_view {
  const cabac_search_log_counters *d_counters;
  const cabac_search_log_entry *d_entries; /* d_counters->n_entry entries, in append order                            */
  const uint16_t *d_records;               /* d_counters->n_record records                                            */
  const cabac_tu_desc *d_tu;               /* d_counters->n_tu descriptors, coeff_offset counting into d_coeff        */
  const uint32_t *d_tu_at;                 /* per logged block its effective position in its entry's run              */
  const void *d_coeff;                     /* d_counters->n_coeff coefficients of coeff_bytes bytes each              */
  uint64_t record_capacity, coeff_capacity;
  uint32_t n_chain, entry_capacity, tu_capacity;
  int32_t coeff_bytes;
} cabac_search_log_view;

/* ---- 1. a log and its teardown ----
 * A log of n_chain (>= 1) chains with device arrays of the given fixed capacities; coeff_bytes is 4 (int32_t) or 2 (int16_t).  No
 * array grows later.  The log is owned by the ctx: cabac_hip_destroy destroys the logs that are left (their handles are dead
 * then).  Both calls wait for the ctx's stream (allocation and release are not stream ordered). */
int cabac_hip_search_log_create(cabac_hip_ctx *ctx, uint32_t n_chain, uint32_t entry_capacity, uint64_t record_capacity,
                                uint32_t tu_capacity, uint64_t coeff_capacity, int coeff_bytes, cabac_search_log **log);
int cabac_hip_search_log_destroy(cabac_search_log *log);

/* ---- 2. empty the log (asynchronous) ---- counters, flags and the chains' cursors to zero */
int cabac_hip_search_log_reset_device(cabac_search_log *log);

/* ---- 3. append the picked candidates of one round (asynchronous) ----
 * d_pick, d_group_chain: n_group words each.  The candidate arrays are those of cabac_hip_search_unit_round_device (d_cand_first
 * n_cand + 1 words, d_rec_first n_cand + 1 uint64_t; d_records and d_tu_at may be NULL as above); they may be overwritten in stream
 * order right after the call.  Returns CABAC_HIP_ERR_INVALID for a coeff_bytes that is not the log's. */
int cabac_hip_search_log_append_device(cabac_search_log *log, uint32_t n_group, const uint32_t *d_pick, const uint32_t *d_group_chain,
                                       uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff,
                                       int coeff_bytes, const uint64_t *d_rec_first, const uint16_t *d_records, const uint32_t *d_tu_at);

/* ---- 4. look into the log ---- */
int cabac_hip_search_log_view(const cabac_search_log *log, cabac_search_log_view *view);

/* ---- 5. code every chain's log into its substream ----
 * d_desc: n_chain descriptors of which only qp and init_id | CABAC_SUB_* are read.  The outputs are those of
 * cabac_hip_encode_residual_device with n_sub = n_chain and n_tu = the blocks in the log (d_tu_info, d_bin_counts may be NULL).
 * Waits for the stream twice (see above).  With CABAC_SEARCH_LOG_OVERFLOW set it codes nothing and returns CABAC_HIP_ERR_INVALID;
 * cabac_hip_last_error names the capacities that overflowed.  The log is not consumed: it can be encoded again (with another qp,
 * say) and appended to afterwards. */
int cabac_hip_search_log_encode_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                       uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                       uint32_t *d_tu_info, uint32_t *d_bin_counts);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SEARCH_EMIT_H */
