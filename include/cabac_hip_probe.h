/*
 * cabac_hip_probe.h — probe points: written and estimated bits INSIDE a substream.
 *
 * The codec answers "how many bits so far?" at the end of a substream only: CABAC_SUB_PROBE (cabac_hip.h) gives
 * getNumWrittenBits() after the last record, cabac_hip_estimate_device one total per substream.  An encoder needs the count after
 * every CTU — written bits decide where a slice ends under a byte budget and feed per-CTU statistics, estimated bits after every
 * CTU are what CTU-level rate control consumes.  The calls below report the running totals at caller-chosen positions in one
 * launch.  An extension of cabac_hip.h (same conventions), in a header of its own because the reference-side test libraries
 * are pinned to the content of cabac_hip.h.  ("Probe", not "mark": a mark is the winner log's hand-over point,
 * cabac_hip_splice_rows.h.)
 *
 * PROBE LISTS (the same for all calls)
 *   d_probe_first   n_sub + 1 ascending uint32_t, starting at 0: substream s owns probes d_probe_first[s] .. d_probe_first[s + 1]
 *   d_probe_at[p]   k: "after the first k records" of the substream that owns probe p; k is clipped to n_records
 *   n_probe         the number of entries d_probe_at and the output hold (d_probe_first[n_sub] <= n_probe)
 * Within a substream the positions are non-decreasing; duplicates are allowed; zero probes for a substream is fine; n_probe == 0
 * is fine.  The device forms do not see a list that breaks these rules: the values of such a substream are unspecified, and
 * nothing outside the arguments is read or written.
 *
 * THE SETS (n_sets, d_state, d_rate, d_start_set) are the start sets of cabac_hip_ctx_sets.h: substream s starts from set
 * d_start_set[s] of d_state / d_rate (379 entries per set); d_start_set == NULL or CABAC_CTX_NO_SET means Ctx::init(desc.qp,
 * desc.init_id & 3).  Nothing is written to a set.  (CABAC_CTX_NO_SET and CABAC_RES_BAD_SET are that header's; this one needs
 * cabac_hip.h only.)
 *
 * ---- 1. Written bits ------------------------------------------------------------------------------------------------------
 * DEFINITION OF THE RESULT: d_bits[p] is results[s].n_bits of cabac_hip_encode_device with CABAC_SUB_PROBE on substream s cut
 * to its first k records; with a start set it is the same answer from cabac_hip_encode_sets_device.  That is
 * BinEncoderBase::getNumWrittenBits() (arith_codec.cpp:482-485) at that point.  k = 0 gives 0.  Nothing is coded and no byte is
 * written: only rec_offset, n_records, qp and init_id & 3 of the descriptors are read.
 * d_flags[s] (d_flags may be NULL) is 0, CABAC_RES_BAD_RECORD or CABAC_RES_BAD_SET.  With CABAC_RES_BAD_RECORD the substream's
 * values are unspecified; with CABAC_RES_BAD_SET (a start index >= n_sets) they are 0.  Either way no other substream is affected
 * and nothing outside the arguments is touched.
 * The count needs no carry state: getNumWrittenBits() is every bit shifted out of `low` so far, wherever it is by now (stored,
 * buffered, an outstanding 0xFF, still in low), and a carry moves no bit.  So the kernel (cabac_probe.hip) runs the range half of
 * the encoder's chain only and sums the shifts; the dispatched encoders are untouched.
 * Asynchronous on the ctx's stream, no host wait inside, no scratch.  n_sub == 0 is OK and launches nothing.
 *
 * ---- 2. Estimated bits ----------------------------------------------------------------------------------------------------
 * DEFINITION OF THE RESULT: d_frac_bits[p] (1/32768 bit) is what cabac_hip_estimate_device answers for substream s cut to its
 * first k records; with a start set it is the answer of cabac_hip_estimate_from_device.  So CABAC_REC_ALIGN,
 * CABAC_REC_EST_RESETBITS and CABAC_REC_EST_RESTART act exactly as there.  d_flags as in part 1.  The kernel is a probe
 * instantiation of the estimator's walk: a step that holds a probe is summed in record order, every other step is unchanged.
 *
 * ---- 3. Written bits across spliced blocks --------------------------------------------------------------------------------
 * cabac_hip_encode_residual_probes_device is cabac_hip_encode_residual_device (cabac_hip.h; the coefficients as const void * with
 * coeff_bytes 4 or 2, as in cabac_hip_splice_rows.h) that also answers probes.  A probe is a PAIR (k, m) = (d_probe_at[p],
 * d_probe_splice[p]) with exactly the meaning of the hand-over pair in cabac_hip_splice_rows.h: k host records in front, and m of
 * the substream's splices in front.  m is clipped to [#{at < k}, #{at <= k}]; d_probe_splice == NULL means the upper end
 * everywhere.  Pairs are non-decreasing in (k, m).  d_bits[p] is getNumWrittenBits() after the part of the EXPANDED string in
 * front of that point.  Payload, offsets, results, tu_info and bin_counts are bit-identical to the plain call's.
 * The probes become positions in the expanded strings (one thread per probe) and the kernel of part 1 runs on the expanded
 * descriptors and records the pipeline holds, behind the block-records pass, on the ctx's stream: no host wait is added to the
 * one the plain call has; the positions are scratch of the ctx.  Default path only: on a ctx whose workspace is fixed
 * (cabac_hip_workspace.h) the call returns CABAC_HIP_ERR_INVALID with nothing queued.  Sets, rows, the log's emit and the plan write
 * have no probe form.
 *
 * ---- Host-pointer forms -----------------------------------------------------------------------------------------------------
 * cabac_hip_written_bits_batch and cabac_hip_estimate_probes_batch: synchronous, everything in host memory, staged as
 * cabac_hip_estimate_batch stages (state / rate hold n_sets sets; bits / frac_bits hold n_probe entries; flags may be NULL).  They
 * return CABAC_HIP_ERR_INVALID, with nothing run and no output touched, for a probe_first that does not ascend from 0 (or ends
 * behind n_probe), positions that go backwards inside a substream, a set index >= n_sets (other than CABAC_CTX_NO_SET), records
 * out of range or an init_id above 2; CABAC_HIP_ERR_SUBSTREAM when a flag is set (the numbers still arrive).
 * cabac_hip_encode_residual_probes_batch: cabac_hip_encode_batch_residual with the probe arguments; it refuses the same probe
 * lists the same way (probe_splice is not checked on the host: it is clipped), and everything the plain form refuses.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports these calls after the kinds listed in the other headers: kind 45, "written-bits
 * walk" (parts 1 and 3); kind 46, "estimate with probes"; kind 47, "probe index of a spliced call".
 */
#ifndef CABAC_HIP_PROBE_H
#define CABAC_HIP_PROBE_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int cabac_hip_written_bits_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                  const uint32_t *d_probe_first, const uint32_t *d_probe_at, uint32_t n_probe, uint32_t n_sets,
                                  const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set, uint32_t *d_bits,
                                  uint32_t *d_flags);
int cabac_hip_estimate_probes_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                     const uint32_t *d_probe_first, const uint32_t *d_probe_at, uint32_t n_probe, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                     uint64_t *d_frac_bits, uint32_t *d_flags);
int cabac_hip_encode_residual_probes_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc,
                                            const uint16_t *d_records, const uint32_t *d_splice_first, const cabac_splice *d_splices,
                                            uint32_t n_splice, uint32_t n_tu, const cabac_tu_desc *d_tu, const void *d_coeff,
                                            int coeff_bytes, uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                            cabac_substream_result *d_results, uint32_t *d_tu_info, uint32_t *d_bin_counts,
                                            const uint32_t *d_probe_first, const uint32_t *d_probe_at, const uint32_t *d_probe_splice,
                                            uint32_t n_probe, uint32_t *d_bits);

int cabac_hip_written_bits_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                 uint64_t n_records_total, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe,
                                 uint32_t n_sets, const uint32_t *state, const uint8_t *rate, const uint32_t *start_set, uint32_t *bits,
                                 uint32_t *flags);
int cabac_hip_estimate_probes_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                    uint64_t n_records_total, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe,
                                    uint32_t n_sets, const uint32_t *state, const uint8_t *rate, const uint32_t *start_set,
                                    uint64_t *frac_bits, uint32_t *flags);
int cabac_hip_encode_residual_probes_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                           uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices,
                                           uint32_t n_tu, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                           uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity, uint64_t *payload_offsets,
                                           cabac_substream_result *results, uint32_t *tu_info, uint32_t *bin_counts,
                                           const uint32_t *probe_first, const uint32_t *probe_at, const uint32_t *probe_splice,
                                           uint32_t n_probe, uint32_t *bits);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PROBE_H */
