/*
 * cabac_hip_pieces.h — the bin codec in pieces: the arithmetic coder's state handed from one call to the next.
 *
 * cabac_hip_encode_sets_device / cabac_hip_decode_sets_device (cabac_hip_ctx_sets.h) hand the CONTEXTS of a substream across a
 * call boundary, but the arithmetic coder always starts fresh: a substream is coded start() .. finish() in one call.  The two
 * calls below also take and give the coder itself — low, range, the buffered 16-bit unit and the outstanding 0xFFFF units of the
 * encoder (BinEncoderBase, arith_codec.cpp:329-357, :524-546, in base 2^16 as the kernels keep it); range, value and the bit
 * position of the decoder (BinDecoderBase, :60-73) — so that a substream can be coded as consecutive runs of its records: a reader
 * that learns the records of the next CTU from the bins of this one, a rate controller that changes the later records because of
 * the bits written so far, an encoder that emits CTU rows while the next ones are still being searched.
 *
 * cabac_hip.h says of CABAC_SUB_FINISH "REQUIRED — a substream is coded start() .. finish() in one call": that is the rule of the
 * calls of that header and of every other one.  For the two calls below a descriptor without it is a piece that is not the last.
 *
 * The set format, "no set" (0xFFFFFFFF), the IN-PLACE RULE and CABAC_RES_BAD_SET are those of cabac_hip_ctx_sets.h and are not
 * repeated here: INCLUDE THAT HEADER where the sets are built.
 *
 * Profile kinds (cabac_hip_profile_read): kind 48 encode in pieces, kind 49 decode in pieces.
 */
#ifndef CABAC_HIP_PIECES_H
#define CABAC_HIP_PIECES_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_RES_BAD_STATE 0x80u /* a coder state that is refused (below): the substream codes nothing, nothing is written */

#define CABAC_CODER_FRESH 0u  /* start(): what an all-zero struct is */
#define CABAC_CODER_ENC 1u    /* an encoder between two pieces */
#define CABAC_CODER_DEC 2u    /* a decoder between two pieces */
#define CABAC_CODER_CLOSED 3u /* behind the last piece */

/* One per substream, indexed by substream.  The first four words are the caller's to read; the other four belong to the coder
 * (copy them, store them, send them over a network — a state copied to the host and back continues identically — but do not
 * make them up).                                                                                                            */
typedef struct cabac_coder_state {
  uint32_t kind;        /* CABAC_CODER_* */
  uint32_t flags;       /* the sticky CABAC_RES_* of the pieces so far: BAD_RECORD, UNDERRUN, BAD_SET, OVERFLOW */
  uint32_t bits;        /* encode: what getNumWrittenBits() (arith_codec.cpp:482-485) answers so far; decode: the bits shifted so
                           far.  CLOSED: the last piece's n_bits                                                                */
  uint32_t bytes_final; /* encode: the bytes at the front of the substream's slot that are stored and will not change (even);
                           CLOSED: the bytes of the finished substream.  decode: 0                                             */
  uint32_t priv[4];     /* encode: low | range + (pend << 16) | buffered unit | buffered + outstanding units
                           decode: range | value (16 bits) | 1 behind a terminate bin 1 | 0                                    */
} cabac_coder_state;

/* ---- the two calls (device pointers, asynchronous on the ctx stream) -----------------------------------------------------
 * They allocate nothing, wait for nothing, and no workgroup waits for another.  The seven set arguments mean exactly what they
 * mean in cabac_hip_encode_sets_device / cabac_hip_decode_sets_device: contexts travel between pieces as sets, piece i's out
 * set being piece i + 1's start set (the IN-PLACE RULE allows an out set to be the substream's own start set).
 *   d_coder_in    the states the substreams continue from; NULL: every substream is fresh
 *   d_coder_out   where the states behind the pieces are written; NULL: no state is written.  May be d_coder_in.
 *
 * DEFINITION OF THE RESULT
 * The pieces of a substream are consecutive runs of its records.  All pieces carry the same byte_offset, byte_capacity, qp and
 * init_id & 3; each has its own rec_offset / n_records.  Decoded bins go to d_bins[rec_offset + i], as always.
 *  - A descriptor WITHOUT CABAC_SUB_FINISH is a non-final piece.  Nothing is flushed; the state behind its last record is
 *    written to d_coder_out[s].  encode: results[s].n_bits is what CABAC_SUB_PROBE answers for all records of the substream so
 *    far (= state.bits).  decode: results[s].n_bits is what cabac_hip_decode_device reports for that prefix without FINISH.
 *    CABAC_SUB_PROBE itself is ignored by these calls.
 *  - A descriptor WITH CABAC_SUB_FINISH (and CABAC_SUB_ALIGN_RBSP as usual) is the last piece: finish() runs on the state
 *    (decode: the stop check), the result is the whole substream's, the out state is CABAC_CODER_CLOSED.
 *  - n_records == 0 is legal in both kinds: a non-final piece of no records passes the state through (a fresh one comes out as
 *    the ENC / DEC state of start()), a final piece of no records only finishes — "end the slice here".
 *  - P1, encode: for a substream whose one-call result has no flag, the slot behind the last piece and the last piece's result
 *    equal those of cabac_hip_encode_sets_device on the concatenated records from the first piece's start set, for every way of
 *    cutting, pieces of one record included.  Behind every non-final piece the first bytes_final bytes of the slot already are
 *    the final bytes, and bits - 8 * bytes_final is exactly the part still buffered, outstanding or inside low.  (WHICH bytes
 *    are final behind a piece depends on where the cuts were: a piece hands over every whole 16-bit unit it has, a carry that
 *    arrives later lands on the buffered unit.)
 *  - P2, decode: the bins of all pieces equal the one-call bins, and so do the last result and the last out set.
 *  - P3: with all states fresh and every descriptor final both calls are bit-identical to the sets calls under forced variant 4
 *    (cabac_hip_set_variant(ctx, 4, 4)).
 *  - FLAGS ARE STICKY.  A piece that raises CABAC_RES_BAD_RECORD, CABAC_RES_UNDERRUN, CABAC_RES_BAD_SET or CABAC_RES_OVERFLOW
 *    writes them into state.flags.  A later piece whose in state has flags codes nothing, returns {0, flags} and copies the
 *    state.  A non-final encode piece raises CABAC_RES_OVERFLOW as soon as bytes_final + 2 * (buffered and outstanding units) >
 *    byte_capacity — all of that will be written — so piecewise and one-call coding flag the same substreams.  The bytes of a
 *    flagged substream are unspecified inside its slot; nothing outside the slot is ever written.  CABAC_RES_UNDERRUN is
 *    reported by the piece in which the read happens and from then on; CABAC_RES_BAD_STOP by the final piece only.
 *  - A STATE IS DATA FROM MEMORY: it is validated when it is loaded, before any loop that depends on it.  Refused with
 *    {0, CABAC_RES_BAD_STATE}, nothing coded and nothing else written (no byte, bin, set or state):
 *      an unknown kind, a decoder state given to encode or the reverse, or CABAC_CODER_CLOSED;
 *      (a state that passes this and has flags is copied as said above, without a further look)
 *      range outside 256..510;
 *      encode: pend > 15, low >= 2^(10 + pend), bits != 8 * bytes_final + 16 * nbuf + pend, an odd bytes_final, or
 *              bytes_final + 2 * nbuf > byte_capacity (pend: the shifts not yet a whole unit; nbuf: priv[3]);
 *      decode: a value not below range << 7.  The one exception is the state behind a terminate bin 1, which the coder marks
 *              (priv[2]): decodeBinTrm leaves value at or above the scaled range there (arith_codec.cpp:184-185) and nothing
 *              but finish() follows; such a state may have range 511 and must have value < (range + 2) << 7.
 *
 * The calls do not go through the dispatch and ignore cabac_hip_set_variant: they are instantiations of the in-wave geometries
 * (encode: one wave per four substreams; decode: four such waves per workgroup), where a row's whole coder state sits in the
 * row's registers.  Not covered: the v6 / v7 encoders, the 4- and 64-lane decode geometries, the parsers, the splice pipeline,
 * the winner log, host-pointer forms.
 */
int cabac_hip_encode_pieces_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                   uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_sets, const uint32_t *d_state,
                                   const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set, uint32_t *d_out_state,
                                   uint8_t *d_out_rate, const cabac_coder_state *d_coder_in, cabac_coder_state *d_coder_out);
int cabac_hip_decode_pieces_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                   const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_sets,
                                   const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                   const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate,
                                   const cabac_coder_state *d_coder_in, cabac_coder_state *d_coder_out);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PIECES_H */
