/*
 * cabac_hip_parse.h — the residual parser's contract on empty, damaged and refused input.
 *
 * An addendum to the description of cabac_hip_residual_parse_device / _parse16_device / _parse_batch / _parse_batch16 in
 * cabac_hip.h (which declares them; this header declares nothing new).  tests/test_gpu_residual_parse_large.py holds the
 * device to every sentence below.
 *
 * What is written.  Of block t only the coded top-left min(w, 32) x min(h, 32) at d_tu[t].coeff_offset, zeros included.
 * Nothing else: not the rest of a 64-wide / tall block, not the elements between, in front of or behind the blocks, not a
 * refused block nor the blocks behind it (their d_tu_info words are not written either).  The host forms copy the whole
 * buffer: cabac_hip_residual_parse_batch keeps the caller's values there, cabac_hip_residual_parse_batch16 returns zeros.
 *
 * Empty substreams.  A substream may hold no block (d_tile_first[s] == d_tile_first[s + 1]): only the terminate bin and
 * the stop pattern are read (with CABAC_SUB_FINISH; n_bits as after any other substream).  With byte_capacity 0 the
 * result is CABAC_RES_UNDERRUN — the decoder's start() already reads two bytes — and nothing of d_bytes is touched.
 *
 * Arbitrary bytes.  The parse is defined for any input: every loop of the walk is bounded by the block geometry alone
 * ("Bounds"), and the result is what the reference's reader would decode up to the point where it
 * throws.
 *   - CABAC_RES_UNDERRUN is reported alone: instead of the stop check (readByte throws before finish() is reached, also
 *     when the input runs out inside the terminate bin) and instead of CABAC_RES_BAD_RECORD, whether the refused block
 *     lies behind the one in which the input ran out or is refused by a coded transform_skip_flag that was itself read
 *     past the end.  The blocks from the one in which the input ran out on are parsed from zeros (the last dword's bytes
 *     behind byte_capacity as they lie in memory) up to a refused block or the end; their values, their d_tu_info and
 *     n_bits are unspecified, and so is CABAC_RES_RANGE of the int16 forms unless a block before them sets it.
 *   - After CABAC_RES_BAD_RECORD (a block the parser does not cover: log2 size above 6, channel above 1,
 *     max_log2_tr_range outside 15..20 and not 0, transform skip beyond 32 x 32) the terminate bin and the stop pattern are not
 *     read; n_bits counts the bits read up to that block, a coded transform_skip_flag included.
 *   - CABAC_RES_RANGE does not stop anything: the stop check is made and reported beside it.
 *   - One start is refused as a whole — no block parsed, nothing written, CABAC_RES_BAD_STOP with or without
 *     CABAC_SUB_FINISH, n_bits 8 as after start() —: a first byte 0xFF (byte_capacity >= 2).  No arithmetic coder writes
 *     it (the first nine bits of its output are its value, below the initial range 510), and the reference's decoder,
 *     which does not check, would run with its value outside its range from the first bin on.
 */
#ifndef CABAC_HIP_PARSE_H
#define CABAC_HIP_PARSE_H

#include "cabac_hip.h"

#endif
