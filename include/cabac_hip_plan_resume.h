/*
 * cabac_hip_plan_resume.h — the plan parse in pieces: a substream's plan walk resumed from a coder state.
 *
 * The plan parse (cabac_hip_parse_plan.h) and its sets form (cabac_hip_plan_rows.h) turn coded bytes into syntax-element values
 * and coefficient blocks in one walk per substream.  A plan has no jumps and no loops, so a reader that learns the elements of
 * the next coding unit from the values of this one — split flags, prediction modes, cbf values — cannot hand the whole plan over
 * in advance.  The sets form hands the CONTEXTS of a substream across a call boundary, but "the arithmetic decoder always starts
 * fresh".  The call below also takes and gives the decoder itself, so that the loop "parse a CTU's plan, look at the values,
 * build the next plan, continue where the decoder stands" runs with no prefix parsed twice, and a WPP hand-over is a cut at the
 * hand-over point.
 *
 * This header uses the plan format, CABAC_GUARD and CABAC_RES_BAD_VALUE of cabac_hip_parse_elements.h, CABAC_PE_COND /
 * CABAC_PE_BLOCK_INFO of cabac_hip_parse_plan.h, the set format, "no set" (0xFFFFFFFF), the IN-PLACE RULE and CABAC_RES_BAD_SET
 * of cabac_hip_ctx_sets.h, cabac_hip_plan_parse_sets_device of cabac_hip_plan_rows.h, and cabac_coder_state, CABAC_CODER_* and
 * CABAC_RES_BAD_STATE of cabac_hip_pieces.h, and does not repeat them: INCLUDE THOSE HEADERS FIRST (the element parse's, the plan
 * parse's, the context sets', the plan rows' and the pieces', in this order).
 *
 * cabac_hip_plan_resume_parse_device: the arguments of cabac_hip_plan_parse_sets_device without d_out_at, then
 *   d_coder_in    an array of cabac_coder_state (cabac_hip_pieces.h), one per substream: the states the substreams continue
 *                 from; NULL: every substream is fresh
 *   d_coder_out   an array of cabac_coder_state: where the states behind the pieces are written; NULL: no state is written.
 *                 May be d_coder_in.
 * (void pointers in the prototype, because this header includes cabac_hip_parse.h alone.)
 *
 * THE STATE is the bin decoder's CABAC_CODER_DEC state of cabac_hip_pieces.h, byte for byte: bits = S, the bits shifted so far;
 * priv = range | value (16 bits) | mark | 0; bytes_final = 0.  One format: a state written by cabac_hip_decode_pieces_device
 * continues here, and the reverse.
 *
 * DEFINITION OF THE RESULT
 *  - PIECES AND DESCRIPTORS.  The pieces of a substream are consecutive runs of its plan entries with the blocks that stand among
 *    them.  All piece descriptors carry the same byte_offset, byte_capacity, qp and init_id & 3.  Each piece has its own
 *    rec_offset / n_records (plan entries), its own tile_first[s] .. tile_first[s + 1] (blocks), and tu_at relative to the
 *    piece.  Values go to d_values[rec_offset + i], as always.
 *  - REFERENCES.  Guards, CABAC_PE_COND back references and CABAC_PE_BLOCK_INFO see the piece alone: the value ring and the info
 *    ring start empty in every piece, and a reference in front of the piece is CABAC_RES_BAD_RECORD, exactly as a reference in
 *    front of the substream is in the plan parse.  The caller has the earlier values and builds the next plan from them.
 *  - A descriptor WITHOUT CABAC_SUB_FINISH is a non-final piece: no stop check; the state behind the piece goes to
 *    d_coder_out[s]; the contexts behind the piece go to the out set; results[s].n_bits is what the plan parse reports for that
 *    prefix without CABAC_SUB_FINISH (S + 8).
 *  - A descriptor WITH CABAC_SUB_FINISH is the final piece: the stop check runs on the cumulative S, the result is the whole
 *    substream's, the out state is CABAC_CODER_CLOSED (flags as reported, bits = S, everything else 0).
 *  - EMPTY PIECES.  n_records == 0 with no block is legal in both kinds: a non-final one passes the state through (a fresh one
 *    comes out as the CABAC_CODER_DEC state of start()), a final one only finishes — "end the slice here".
 *  - The out set is behind the piece, always.  There is no d_out_at: a WPP hand-over is a cut.
 *  - R1.  For plans whose references stay inside their pieces, and any bytes: the values, coefficients, info words, last result
 *    and last out set of the pieces equal those of ONE cabac_hip_plan_parse_sets_device call on the concatenated plan (d_out_at
 *    == NULL), for every way of cutting, pieces of one entry, of one block and no entry, and of nothing included — up to the
 *    piece that raises a sticky flag (below): the one call walks on behind an underrun and learns of it at its end, the pieces
 *    behind the one that reports it parse nothing.
 *  - R2.  With all states fresh and every descriptor final every output is bit-identical to cabac_hip_plan_parse_sets_device
 *    (d_out_at == NULL).
 *  - R3, one state format.  For the expanded record string of a valid unit (tests/parse_plan_model.py::expand) and a cut in front
 *    of an element, not behind a terminate bin 1: the state cabac_hip_decode_pieces_device writes behind the records in front of
 *    the cut equals, as 32 bytes, the state this call writes there, and each call continues from the other's state to the same
 *    final result.  Behind a terminate bin 1 the continuation holds, not the byte equality: the state is MARKED (priv[2] = 1),
 *    range 256..511 (the decoder's range - 2 with bit 8 set, so that 254 / 255 travel as 510 / 511 and are taken back when
 *    loaded), value below (range + 2) << 7.  Nothing but finish() may follow a marked state, and finish() depends on S alone.
 *    The decoder's marked states are accepted as well.
 *  - FLAGS.  CABAC_RES_BAD_RECORD, CABAC_RES_BAD_VALUE, CABAC_RES_UNDERRUN and CABAC_RES_BAD_SET are sticky in state.flags.  A
 *    later piece whose in state has flags parses nothing: it returns {0, flags} and copies the state, and writes no value,
 *    coefficient, info word or set.  CABAC_RES_RANGE is reported by the piece whose block raised it; it is not stored and stops
 *    nothing.  CABAC_RES_BAD_STOP is reported by the final piece only — the one exception is the fresh start on the byte 0xFF,
 *    refused as the plan parse refuses it ({8, CABAC_RES_BAD_STOP}, the start contexts handed over) and sticky.
 *    CABAC_RES_UNDERRUN is reported by the piece in which S crosses the capacity and from then on.
 *  - A STATE IS DATA FROM MEMORY: it is validated when it is loaded, before anything depends on its values.  Refused with
 *    {0, CABAC_RES_BAD_STATE} and nothing else written (no value, coefficient, info word, set or state):
 *      an unknown kind, a CABAC_CODER_ENC state, or CABAC_CODER_CLOSED;
 *      (a state that passes this and has flags is copied as said above, without a further look)
 *      range outside 256..510 (511 when marked);
 *      a value not below range << 7 ((range + 2) << 7 when marked);
 *      a mark above 1;
 *      a state without flags whose 2 + (bits >> 3) > byte_capacity: no flagless decoder stands there, the underrun would have been
 *      flagged.  With it every byte offset computed from S lies inside the slot or is fed zeros, as in the plan parse.
 *  - The call allocates nothing and waits for nothing; no workgroup waits for another.  It is asynchronous on the ctx's stream
 *    under the STREAM ORDERING CONTRACT of cabac_hip.h.  d_coder_out may be d_coder_in (every substream reads its state before
 *    it parses).  The IN-PLACE RULE of the sets applies.
 *
 * Launched like the sets form: four substreams per workgroup from 1 024 substreams up, one below.  There is no host-pointer form
 * and nothing in the C++ shim, as for the calls of cabac_hip_pieces.h.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call after the kinds listed in the other headers: kind 50, "plan parse resumed".
 */
#ifndef CABAC_HIP_PLAN_RESUME_H
#define CABAC_HIP_PLAN_RESUME_H

#include "cabac_hip_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

int cabac_hip_plan_resume_parse_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                       const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                       const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                       uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_sets,
                                       const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                       const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, const void *d_coder_in,
                                       void *d_coder_out);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PLAN_RESUME_H */
