/*
 * cabac_hip_piece_encoder.h — which encoder codes the pieces: a per-ctx choice between two kernels that write the same thing.
 *
 * The pieces calls (cabac_hip_pieces.h) and the plan write continued from a coder state (cabac_hip_plan_continue.h) were built on
 * the in-wave encoder, one wave per four substreams, where a row's whole coder state sits in the row's registers.  The encoder
 * the dispatch picks for a one-call batch is the lane-serial one (v7: context waves, a chain wave with one substream per lane,
 * a low wave and an output wave), about three times as fast on a full batch.  Its coder state is spread over three waves — the
 * chain wave's range, the low wave's low and pending shifts, the output wave's buffered unit, count and position — but each
 * part is loaded before the first workgroup barrier and is final behind the last, and the flush discipline is the same (posts
 * after bins 3, 7, 11, 15 of the piece's own steps, whole units cut from low, the carry on the buffered unit).  So it has a
 * pieces form too, and this header selects it.
 *
 * WHICH CALLS FOLLOW THE SETTING
 *   cabac_hip_encode_pieces_device              (cabac_hip_pieces.h)
 *   the encode leg of cabac_hip_plan_continue_write_device   (cabac_hip_plan_continue.h)
 * and nothing else.  Both keep ignoring cabac_hip_set_variant and keep their profile kinds.  cabac_hip_decode_pieces_device does
 * not look at it.
 *
 * THE SETTING (per ctx; THE DEFAULT IS 4: a ctx on which the setter is never called behaves as before this header)
 *   4   the in-wave encoder, one wave per four substreams
 *   7   the lane-serial encoder: sixteen substreams per workgroup from 1 024 substreams in the call, four below that
 *   0   by the batch: 7 from a threshold number of substreams in the call, 4 below it (the threshold is a measured constant
 *       of the library; results never depend on it)
 * ANY OTHER VALUE IS REFUSED with CABAC_HIP_ERR_INVALID and changes nothing.
 *
 * DEFINITION
 *  - D1: under every setting the bytes in the slots, the results, the out sets and all 32 bytes of every out state are those of
 *    setting 4, for every way of cutting a substream into pieces: fresh, continued, empty, final and only-finishing pieces, refused
 *    and flagged states, slots that overflow.  Everything cabac_hip_pieces.h and cabac_hip_plan_continue.h define holds unchanged.
 *  - D2: therefore a state written under one setting continues under any other, on this ctx or another, before or after a copy
 *    to the host and back; the setting may change between any two calls.
 *  - The in-place rule of the coder states (the out array may be the in array) holds under every setting: a state is read before the
 *    first workgroup barrier of the kernel and written behind the last, by the one lane that owns the substream.
 *  - A substream whose state is refused or comes with flags codes nothing under every setting; beside it, in the same workgroup,
 *    its neighbours code as if it were not there.
 *
 * NOT COVERED: the v6 encoder, the decoders (one geometry, as before), the splice pipeline, the winner log, host-pointer forms,
 * the C++ shim.
 */
#ifndef CABAC_HIP_PIECE_ENCODER_H
#define CABAC_HIP_PIECE_ENCODER_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* variant: 4 (the default), 7, or 0 = by the batch.  Takes effect with the next call on this ctx; launches already on the stream
 * are not affected.  Returns CABAC_HIP_OK, or CABAC_HIP_ERR_INVALID (no ctx, or any other value: the setting stays as it was). */
int cabac_hip_piece_encoder_set(cabac_hip_ctx *ctx, int variant);

/* The value set (4, 7 or 0); a negative error code without a ctx. */
int cabac_hip_piece_encoder_get(const cabac_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PIECE_ENCODER_H */
