/*
 * cabac_hip_workspace.h — a FIXED WORKSPACE for the calls that turn a slice into bytes: while a ctx's workspace is fixed, the
 * nine device forms listed below queue their work on the ctx's stream and return.  They perform no host synchronisation, no
 * allocation, no free and no blocking copy; what the host used to decide after its wait is decided on the device and reported in
 * device memory.  A ctx whose workspace was never fixed (or was released) takes the path it always took: nothing below applies.
 * In a header of its own so that the declaration lists of the other headers stay what they are; it includes cabac_hip.h only, and
 * names the calls of the other headers in comments.
 *
 * THE NINE CALLS
 *   the splice pipeline   cabac_hip_encode_residual_device, cabac_hip_encode_residual16_device (cabac_hip.h),
 *                         cabac_hip_encode_residual_sets_device, cabac_hip_encode_residual_rows_device (cabac_hip_splice_rows.h)
 *   the plan write        cabac_hip_write_plan_device (cabac_hip_write_plan.h), cabac_hip_plan_write_sets_device,
 *                         cabac_hip_plan_write_rows_device (cabac_hip_plan_rows.h)
 *   the log's emit        cabac_hip_search_log_encode_device (cabac_hip_search_emit.h),
 *                         cabac_hip_search_log_encode_sets_device, cabac_hip_search_log_encode_rows_device
 *                         (cabac_hip_splice_rows.h)
 * Their headers say that they wait for the ctx's stream "ONCE in the middle", that the log's emit will "WAIT FOR THE STREAM
 * TWICE", and that they return CABAC_HIP_ERR_INVALID for a damaged splice list, a substream past 2^32 records and an overflowed
 * log.  WHILE A WORKSPACE IS FIXED those sentences read: the call does not wait at all; the three conditions are found on the
 * device, VOID the call (below) and are reported in the status, and the call returns CABAC_HIP_OK — it cannot know.
 *
 * WHAT IS CHECKED ON THE HOST, before anything is queued: n_sub (the log's n_chain) and n_tu (the log's tu_capacity; n_splice
 * must equal n_tu, as always) against cabac_workspace_sizes, the log's record_capacity against log_records, and a rows call
 * against CABAC_WS_ROWS.  A call that exceeds the fixed sizes returns CABAC_HIP_ERR_INVALID (cabac_hip_last_error says which
 * size): nothing is queued, no output is touched, the waits counter does not move.  No library buffer of the plan write grows
 * with its entry count, and the device forms cannot see that count on the host: n_entries is the caller's statement and is not
 * checked.
 *
 * A GOOD CALL.  Every output is bit for bit what the same call produces on a ctx without a fixed workspace: payload,
 * payload_offsets, results, tu_info, bin_counts, values_out, out sets.
 *
 * A VOIDED CALL.  Behind the sizes pass, as the tail of the scan kernel, THE GATE compares the totals found on the device — the
 * records of all expanded strings, the bytes of all byte slots (7 bits per record, plus 8 bytes, rounded up to 16 per substream)
 * — with expanded_records and slot_bytes, and looks at the conditions above.  If a total exceeds its room or a condition holds,
 * the call is VOIDED and writes
 *   {n_bits = 0, flags = CABAC_RES_OVERFLOW} into every d_results[s],
 *   0 into d_payload_offsets[0 .. n_sub],
 *   its flags and, when the totals are sound, its needs into the status,
 * and nothing else of the caller's that matters: no payload byte, no out set, no values_out word (also with d_values_out ==
 * d_values_in), nothing to the log.  d_tu_info and d_bin_counts may hold anything, inside their arrays.  The caller can fix a
 * larger workspace and repeat the call with the same arrays.  No kernel behind the gate reads or writes outside the workspace or
 * the caller's arrays.  THE STATUS IS THE AUTHORITY on whether a call was voided: a lone CABAC_RES_OVERFLOW also comes from a
 * payload_capacity or, in the bin codec, a slot that was too tight.
 *
 * THE LOG'S EMIT reads the log's counters on the device; its launches are sized from the capacities the log was created with
 * (n_tu of the sizes >= tu_capacity, log_records >= record_capacity).  The unused tail of the log's block list is handed to the
 * binariser as descriptors it rejects (it looks at them and writes nothing), and the splice kernels read the number of logged
 * blocks from device memory; the time of the emit therefore follows entry_capacity and tu_capacity, not the entries and blocks
 * logged.  d_tu_info receives one word per LOGGED block, as always.  A log whose append was dropped for capacity
 * (CABAC_WS_LOG_OVERFLOW) or whose counters exceed its capacities (CABAC_WS_LOG_DAMAGED) voids the call.
 *
 * THE HOST-POINTER FORMS of these pipelines (cabac_hip_encode_batch_residual, cabac_hip_encode_batch_residual16,
 * cabac_hip_encode_residual_rows_batch, cabac_hip_write_plan_batch, cabac_hip_plan_write_rows_batch) share the buffers and are
 * synchronous anyway: while the workspace is fixed they return CABAC_HIP_ERR_INVALID and cabac_hip_last_error names
 * cabac_hip_workspace_release.  EVERY OTHER ENTRY POINT works as before.  The scratch of the search rounds, the parsers, the
 * estimators and the log's append is NOT part of the fixed workspace: it still grows on demand, on the first call of each size
 * (the waits counter shows it), and is stable afterwards.
 *
 * The status is STREAM-ORDERED: cabac_hip_workspace_status_device queues a copy on the ctx's stream, so what arrives reflects
 * every call queued before it.  n_calls counts the fixed-mode calls that reached the device since the fix, in order from 0.
 *
 * cabac_hip_profile_read (cabac_hip.h): the gate runs as the tail of the scan and a voided call's results are written by the
 * assembly's scan, so both report with those (the splice kernels, the plan write, the assembly), and the log's place pass sized from
 * capacities reports as the log's place pass does.  The two kernels that exist on this path alone report as kind 40, "workspace":
 * the live out sets of a call with sets, and the copy of d_tu_info for the logged blocks in the log's emit.
 */
#ifndef CABAC_HIP_WORKSPACE_H
#define CABAC_HIP_WORKSPACE_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cabac_workspace_sizes.flags */
#define CABAC_WS_ROWS 0x1u /* also what the WPP schedule of the rows forms needs: one context set per substream */

/* cabac_workspace_status.flags */
#define CABAC_WS_OVER_RECORDS 0x1u   /* the expanded records found on the device exceed expanded_records                     */
#define CABAC_WS_OVER_SLOTS 0x2u     /* the byte slots found on the device exceed slot_bytes                                 */
#define CABAC_WS_BAD_SPLICES 0x4u    /* splice list: not sorted, outside its substream, or a block not spliced exactly once  */
#define CABAC_WS_RECORDS_32BIT 0x8u  /* a substream outgrows 32 bits of records                                              */
#define CABAC_WS_LOG_OVERFLOW 0x10u  /* the log overflowed (an append was dropped)                                           */
#define CABAC_WS_LOG_DAMAGED 0x20u   /* the log's counters exceed its capacities                                             */

#define CABAC_WS_NONE_VOIDED 0xFFFFFFFFu /* cabac_workspace_status.first_voided: no call was voided */

typedef struct cabac_workspace_sizes {
  uint32_t n_sub;            /* most substreams (chains, for the log's emit) of one call                      */
  uint32_t n_tu;             /* most blocks of one call; for the log's emit at least the log's tu_capacity    */
  uint64_t n_entries;        /* most plan entries of one call (plan write); 0 if never used                   */
  uint64_t expanded_records; /* most records of all expanded strings of one call together                     */
  uint64_t slot_bytes;       /* most bytes of all byte slots of one call together                             */
  uint64_t log_records;      /* most side records the log's emit lays out; at least the log's record_capacity */
  uint32_t flags;            /* CABAC_WS_ROWS                                                                 */
  uint32_t reserved;         /* 0 */
} cabac_workspace_sizes;

typedef struct cabac_workspace_status {
  uint64_t records_needed;    /* largest total of expanded records any call since the fix asked for */
  uint64_t slot_bytes_needed; /* the same for the byte slots                                        */
  uint32_t flags;             /* CABAC_WS_* above, ORed over the calls since the fix                */
  uint32_t n_calls;           /* fixed-mode calls queued since the fix                              */
  uint32_t n_voided;          /* of them, voided                                                    */
  uint32_t first_voided;      /* number (from 0) of the first voided call; CABAC_WS_NONE_VOIDED     */
} cabac_workspace_status;

/* Host arithmetic only, no ctx, no GPU: a pair (expanded records, slot bytes) that no call with at most n_sub substreams,
 * n_host_records host records (for the plan write: bins of its plan elements; for the log's emit: side records) in all, n_tu
 * blocks and n_coded_coeff coefficients in those blocks together (w * h of each; the coded region, at most 32 x 32, is enough)
 * can exceed:
 *   expanded_records = n_host_records + the sum of CABAC_TU_MAX_RECORDS over the blocks = n_host_records + 33 n_tu + 38 n_coded_coeff
 *   slot_bytes       = (7 expanded_records + 7) / 8 + 24 n_sub      (a slot: 7 bits per record, 8 bytes, rounded up to 16)
 * Callers who know their data fix less and look at the status.  Returns CABAC_HIP_ERR_INVALID for a null pointer or a bound past
 * 2^60. */
int cabac_hip_workspace_bound(uint32_t n_sub, uint64_t n_host_records, uint32_t n_tu, uint64_t n_coded_coeff, uint64_t *expanded_records,
                              uint64_t *slot_bytes);

/* Fix the workspace.  May block and allocate: it waits for the ctx's stream, grows every library buffer the nine calls touch to
 * what *sizes asks for (the pinned block included), resets the status in device memory and switches the ctx to fixed mode.
 * Calling it again while fixed waits for the ctx's stream and replaces the sizes (buffers only grow).  CABAC_HIP_ERR_INVALID for
 * reserved != 0, unknown flags or sizes past 2^60 (n_entries is range-checked and otherwise ignored: it sizes no
 * buffer); CABAC_HIP_ERR_NOMEM leaves the ctx on the on-demand path. */
int cabac_hip_workspace_fix(cabac_hip_ctx *ctx, const cabac_workspace_sizes *sizes);

/* Waits for the ctx's stream and puts the ctx back on the on-demand path.  The buffers stay.  Harmless on a ctx that is not
 * fixed. */
int cabac_hip_workspace_release(cabac_hip_ctx *ctx);

/* Queue a copy of the status on the ctx's stream into d_out: device memory, or pinned host memory, of the caller's.  No wait.
 * CABAC_HIP_ERR_INVALID on a ctx whose workspace is not fixed. */
int cabac_hip_workspace_status_device(cabac_hip_ctx *ctx, cabac_workspace_status *d_out);

/* The synchronous form: waits for the ctx's stream.  After a release it answers the status as the release found it. */
int cabac_hip_workspace_status(cabac_hip_ctx *ctx, cabac_workspace_status *out);

/* A host-side counter that never decreases: the blocking operations the library has issued for this ctx since cabac_hip_init —
 * every hipStreamSynchronize, hipEventSynchronize, hipMalloc, hipFree, hipHostMalloc and hipHostFree, counted where it is issued
 * (the library issues no hipDeviceSynchronize and no synchronous hipMemcpy).  What an integrator reads to find out which of their
 * calls still block. */
int cabac_hip_workspace_waits(cabac_hip_ctx *ctx, uint64_t *n);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_WORKSPACE_H */
