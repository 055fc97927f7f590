/*
 * cabac_hip_parse_plan.h — C ABI of the plan parse: the element parse (cabac_hip_parse_elements.h) with two more entry kinds that
 * read no bin and COMPUTE a value: a condition on earlier values, joined by AND / OR with another one, and a field of the result
 * of a block walked earlier.  A guard stays one comparison on one value; everything richer becomes a value that a guard can
 * test.  With them a whole transform unit is read in one walk: cu_qp_delta behind cbf_y || cbf_cb || cbf_cr, tu_cbf_cr on the
 * context tu_cbf_cb selects (two guarded alternatives merged by an OR), mts_idx behind "luma coded, not transform skip,
 * scanPosLast > 0, no MTS violation", an LFNST condition over the last positions of three blocks.  Still no jumps and no loops:
 * the plan is walked forwards once, and the coding-tree recursion stays with the caller.  An extension of cabac_hip_parse.h, in
 * a header of its own so that the declaration lists of the other headers stay what they are.
 *
 * This header uses CABAC_GUARD, the CABAC_GUARD_* comparisons, CABAC_RES_BAD_VALUE and CABAC_TU_INFO_NOT_CODED of
 * cabac_hip_parse_elements.h and does not repeat them: INCLUDE THAT HEADER FIRST.
 *
 * DEFINITION OF THE RESULT.
 *   Everything is as in cabac_hip_parse_elements.h unless stated here: the substream descriptors, the plan of 2 x uint32_t
 *   entries, the block positions at(t), the walk, the guard word (reserved bits 15..10 must be zero), the values of kinds 0..8 and
 *   of skipped elements, bad entries, the Exp-Golomb bound, OUT OF RANGE, underrun, and what is written.
 *   THE INFO WORD of a block is the word d_tu_info[t] receives, whether or not d_tu_info is NULL:
 *   scanPosLast | CABAC_TU_INFO_MTS_VIOLATION for a regular block, CABAC_TU_INFO_TS for a block parsed as transform skip,
 *   CABAC_TU_INFO_NOT_CODED for a skipped block.
 *   nb(i) is the number of blocks of the substream with at(t) <= i: the blocks walked in front of element i, skipped ones
 *   included.
 *   KIND 9, CABAC_PE_COND.
 *     word0 bits  3..0   kind = 9
 *           bits 11..4   back2
 *           bits 13..12  join    0 none, 1 AND, 2 OR
 *           others       ignored
 *     word1              a TEST in the guard word's format (back, cmp, reserved bits, imm); it is not a guard of the entry
 *   T = 1 when the test's back is 0, else T = (value(i - back) cmp imm).  join 0: value(i) = T, back2 is ignored.  join 1:
 *   value(i) = T && value(i - back2) != 0.  join 2: value(i) = T || value(i - back2) != 0.  A COND entry is never skipped, reads
 *   no bin and touches no context.  Bad entries: nonzero reserved test bits; back > i; join 3; join != 0 with back2 0 or
 *   back2 > i.
 *   KIND 10, CABAC_PE_BLOCK_INFO.
 *     word0 bits  3..0   kind = 10
 *           bits  7..4   which
 *           bits 12..8   shift
 *           bits 18..13  width
 *           others       ignored
 *     word1              an ordinary guard
 *   value(i) = (info word of block nb(i) - 1 - which >> shift) & (2^width - 1), the blocks counted within the substream: which 0
 *   is the block walked last in front of element i.  Skipped by its guard the value is 0.  The entry reads no bin and touches no
 *   context.  Bad entries: which >= nb(i); width 0; shift + width > 32; a bad guard.  As for every entry, whether it is bad
 *   depends on no decoded value: nb(i) follows from d_tu_at, d_tile_first and n_records alone.
 *   KINDS 11..15 are bad.
 *   Values of kinds 9 and 10 are stored in d_values like any other and can be tested by later guards, tests and block guards.  A
 *   COND or BLOCK_INFO entry is never "met OUT OF RANGE": it reads no bin.  Where the values an entry refers to are unspecified
 *   (after an underrun, behind a first element met OUT OF RANGE), its value is unspecified.
 *   TWO IDENTITIES.
 *   P1. A plan with no entry of kind 9 or 10 gives, on any bytes, every output of the element parse's device form: values,
 *       coefficients, info words and results, stops at bad entries included (kind 9 or 10 replaced by kind 15 gives the same
 *       stop).
 *   P2. Take a plan in which every COND has join 0 and every reference to a COND is a guard != 0 with back_guard + back_test
 *       <= 255.  Rewrite each COND into EP_BINS with numBins 0, and each guard on a COND into that COND's own test with back set
 *       to back_guard + back_test.  The rewritten plan, run through the element parse's device form, gives the same outputs
 *       except at the COND slots of d_values — on any bytes: it is the same walk and the same arithmetic.
 *   After an underrun both identities are required only to report CABAC_RES_UNDERRUN alone on both sides.
 *
 * The device form is asynchronous on the ctx's stream under the STREAM ORDERING CONTRACT of cabac_hip.h: no host
 * synchronisation, no allocation that depends on the data, no kernel that waits for another workgroup.  It needs no library
 * scratch.
 *
 * cabac_hip_profile_read (cabac_hip.h) reports the call after the kinds listed in the other headers: kind 27, "plan parse".
 */
#ifndef CABAC_HIP_PARSE_PLAN_H
#define CABAC_HIP_PARSE_PLAN_H

#include "cabac_hip_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the two computed entry kinds (word0 bits 3..0) */
#define CABAC_PE_COND 9u
#define CABAC_PE_BLOCK_INFO 10u

#define CABAC_JOIN_NONE 0u
#define CABAC_JOIN_AND 1u
#define CABAC_JOIN_OR 2u
/* word0 of a COND entry; its word1 is CABAC_GUARD(back, cmp, imm), read as a test */
#define CABAC_PE_COND_WORD0(join, back2) (CABAC_PE_COND | (((uint32_t)(back2) & 0xFFu) << 4) | (((uint32_t)(join) & 3u) << 12))
/* word0 of a BLOCK_INFO entry */
#define CABAC_PE_BLOCK_INFO_WORD0(which, shift, width) \
  (CABAC_PE_BLOCK_INFO | (((uint32_t)(which) & 0xFu) << 4) | (((uint32_t)(shift) & 0x1Fu) << 8) | (((uint32_t)(width) & 0x3Fu) << 13))

/* Parameters, types and NULL rules of the element parse's device form. */
int cabac_hip_parse_plan_device(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results);

/* Host-pointer form (synchronous), staged as the element parse's.  Returns CABAC_HIP_ERR_INVALID with nothing run and no output
 * touched for everything that form refuses, and for the bad entries of kinds 9 and 10 and kinds above 10 (cabac_hip_last_error
 * names the substream and the element).  Returns CABAC_HIP_ERR_SUBSTREAM when a result flag is set. */
int cabac_hip_parse_plan_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                               uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                               const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                               int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                               cabac_substream_result *results);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_PARSE_PLAN_H */
