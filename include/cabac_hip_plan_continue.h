/*
 * cabac_hip_plan_continue.h — the plan write in pieces: a substream's plan write continued from a coder state.
 *
 * The plan write (cabac_hip_write_plan.h) and its sets form (cabac_hip_plan_rows.h) turn a plan, the values of its real elements
 * and the blocks' coefficients into coded bytes with no host pass over the bins, but they code start() .. finish() in one call
 * and hand back a compacted payload.  The encoder in pieces (cabac_hip_pieces.h) hands the arithmetic coder across a call
 * boundary, but it takes bin records.  The call below is the plan write whose output is the CALLER'S SLOT and whose coder comes
 * from and goes to a coder state, so that the loop "write a CTU's plan, read state.bits, choose the next CTU's values, continue
 * where the encoder stands" runs on the device: a rate controller that changes the later elements because of the bits written so
 * far, an encoder that emits CTU rows while the next ones are still being searched.
 *
 * This header uses the plan format, CABAC_GUARD and CABAC_RES_BAD_VALUE of cabac_hip_parse_elements.h, CABAC_PE_COND /
 * CABAC_PE_BLOCK_INFO of cabac_hip_parse_plan.h, the stops of cabac_hip_write_plan.h, the set format, "no set" (0xFFFFFFFF), the
 * IN-PLACE RULE and CABAC_RES_BAD_SET of cabac_hip_ctx_sets.h, cabac_hip_plan_write_sets_device of cabac_hip_plan_rows.h, and
 * cabac_coder_state, CABAC_CODER_* and CABAC_RES_BAD_STATE of cabac_hip_pieces.h, and does not repeat them: INCLUDE THOSE HEADERS
 * FIRST (the element parse's, the plan parse's, the plan write's, the context sets', the plan rows' and the pieces', in this
 * order).
 *
 * cabac_hip_plan_continue_write_device: the arguments of cabac_hip_plan_write_sets_device with
 *   d_bytes       in place of d_payload, payload_capacity and d_payload_offsets: the slot base, used as
 *                 cabac_hip_encode_pieces_device uses it.  Unlike the plan write, this call USES the descriptor's byte_offset (a
 *                 multiple of 16) and byte_capacity: substream s is coded into d_bytes[byte_offset .. byte_offset + byte_capacity)
 * and behind the seven set arguments
 *   d_coder_in    an array of cabac_coder_state (cabac_hip_pieces.h), one per substream: the states the substreams continue
 *                 from; NULL: every substream is fresh
 *   d_coder_out   an array of cabac_coder_state: where the states behind the pieces are written; NULL: no state is written.
 *                 May be d_coder_in.
 * (void pointers in the prototype, because this header includes cabac_hip.h alone.)
 *
 * THE STATE is the bin encoder's CABAC_CODER_ENC state of cabac_hip_pieces.h, byte for byte.  One format: a state written by
 * cabac_hip_encode_pieces_device continues here, and the reverse.
 *
 * DEFINITION OF THE RESULT
 *  - PIECES AND DESCRIPTORS.  The pieces of a substream are consecutive runs of its plan entries with the blocks that stand among
 *    them; the cuts are those of the plan parse in pieces (tests/plan_resume_model.py: is_cut, spans_of).  All piece descriptors
 *    carry the same byte_offset, byte_capacity, qp and init_id & 3.  Each piece has its own rec_offset / n_records (plan entries),
 *    its own tile_first[s] .. tile_first[s + 1] (blocks), and tu_at relative to the piece.  Filled values go to
 *    d_values_out[rec_offset + i] and info words to d_tu_info[t], as always.
 *  - REFERENCES.  Guards, CABAC_PE_COND back references and CABAC_PE_BLOCK_INFO see the piece alone: the value ring and the info
 *    ring start empty in every piece, and a reference in front of the piece is CABAC_RES_BAD_RECORD, exactly as a reference in
 *    front of the substream is in the plan write.  The caller has the earlier values and builds the next plan from them.
 *  - A descriptor WITHOUT CABAC_SUB_FINISH is a non-final piece.  Nothing is flushed; the state behind the piece goes to
 *    d_coder_out[s] as a CABAC_CODER_ENC state, byte for byte the state cabac_hip_encode_pieces_device writes behind the same
 *    expanded records; the contexts behind the piece go to the out set; results[s].n_bits == state.bits, what
 *    getNumWrittenBits() answers so far — the number a rate controller reads.
 *  - A descriptor WITH CABAC_SUB_FINISH (and CABAC_SUB_ALIGN_RBSP as usual) is the final piece: finish() runs on the state, the
 *    result is the whole substream's, the out state is CABAC_CODER_CLOSED.
 *  - EMPTY PIECES.  n_records == 0 with no block is legal in both kinds: a non-final one passes the state through (a fresh one
 *    comes out as the CABAC_CODER_ENC state of start()), a final one only finishes — "end the slice here".  CABAC_SUB_PROBE is
 *    ignored.
 *  - C1.  For a valid unit whose references stay inside their pieces, and for every way of cutting, pieces of one entry, of one
 *    block and no entry, and of nothing included: the slot behind the last piece, the last result, the last out set, d_values_out
 *    and d_tu_info equal what ONE cabac_hip_plan_write_sets_device call on the concatenated plan gives (its payload bytes of
 *    the substream, from the first piece's start set).  Behind every non-final piece the first bytes_final bytes of the slot
 *    already are the final bytes.  All of this is exact.
 *  - C2, one state format.  Each state written behind a piece equals, as 32 bytes, the state cabac_hip_encode_pieces_device
 *    writes behind the same prefix of the expanded record string (tests/parse_plan_model.py::expand) under the same cuts, and
 *    either call continues from the other's state to the same bytes.
 *  - C3.  With all states fresh and every descriptor final the slot bytes, results, out sets, values and info words equal those
 *    of cabac_hip_plan_write_sets_device.
 *  - STOPS.  A piece whose own walk finds a bad entry, a value outside its element's code or a coded block without a coefficient
 *    stops with CABAC_RES_BAD_RECORD / CABAC_RES_BAD_VALUE, by the rules and the precedence of cabac_hip_write_plan.h applied to
 *    the piece.  The stopped piece codes nothing of itself, is not finished (whatever its descriptor says) and writes no out
 *    set, no value, no info word and no byte.
 *    It returns {0, flag} and writes the in state with the flag added as the out state (a fresh in state comes out as the
 *    CABAC_CODER_ENC state of start(), flagged): the bytes up to bytes_final stay what they were.
 *  - FLAGS ARE STICKY in state.flags: the two stops, and CABAC_RES_OVERFLOW and CABAC_RES_BAD_SET as the encoder in pieces raises
 *    them (a non-final piece raises CABAC_RES_OVERFLOW as soon as bytes_final + 2 * (buffered and outstanding units) >
 *    byte_capacity, so piecewise and one-slot coding flag the same substreams; nothing outside the slot is ever written).  A later
 *    piece whose in state has flags returns {0, flags} and copies the state.  It writes no value, info word, byte or set.
 *  - A STATE IS DATA FROM MEMORY: the checks of cabac_hip_encode_pieces_device run where it is loaded, before the walk writes
 *    anything.  Refused with {0, CABAC_RES_BAD_STATE} and nothing else written (no value, info word, byte, set or state):
 *      an unknown kind, a CABAC_CODER_DEC state, or CABAC_CODER_CLOSED;
 *      (a state that passes this and has flags is copied as said above, without a further look)
 *      range outside 256..510; pend > 15; low >= 2^(10 + pend); bits != 8 * bytes_final + 16 * nbuf + pend; an odd bytes_final;
 *      bytes_final + 2 * nbuf > byte_capacity (pend: the shifts not yet a whole unit; nbuf: priv[3]).
 *  - IN PLACE.  d_coder_out may be d_coder_in (every substream reads its state before anything of it is written).  d_values_out
 *    may be d_values_in.  The IN-PLACE RULE of the sets applies.
 *  - THE HOST.  The call waits for the ctx's stream once in the middle, as the plan write does: the sizes decide the record
 *    scratch.  It allocates only library scratch, and no workgroup waits for another.  It is not one of the calls that queue
 *    without a wait while the ctx's workspace is fixed (cabac_hip_workspace.h): while it is fixed the call returns
 *    CABAC_HIP_ERR_INVALID before anything is queued.
 *
 * Launched like the plan write (four substreams per workgroup in the two walks) and the encoder in pieces (four substreams per
 * wave).  There is no host-pointer form, no rows form and nothing in the C++ shim, as for the calls of cabac_hip_pieces.h
 * (DESIGN.md section 8).
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call's coding launch after the kinds listed in the other headers: kind 51,
 * "plan write continued", once per call; its walks and its block passes are reported as the plan write's are.
 */
#ifndef CABAC_HIP_PLAN_CONTINUE_H
#define CABAC_HIP_PLAN_CONTINUE_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int cabac_hip_plan_continue_write_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                         const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu,
                                         const cabac_tu_desc *d_tu, const uint32_t *d_tu_at, const uint32_t *d_tu_guard,
                                         const void *d_coeff, int coeff_bytes, uint8_t *d_bytes, cabac_substream_result *d_results,
                                         uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_sets, const uint32_t *d_state,
                                         const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                         uint32_t *d_out_state, uint8_t *d_out_rate, const void *d_coder_in, void *d_coder_out);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PLAN_CONTINUE_H */
