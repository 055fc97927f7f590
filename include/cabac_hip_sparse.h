/*
 * cabac_hip_sparse.h — C ABI of the sparse coefficient transport of libcabac_hip.so: transform blocks as lists of their non-zero
 * coefficients, expanded to and compacted from the dense blocks the binariser reads and the parser writes, on the device and on
 * the host.  An extension of cabac_hip.h (same conventions: plain pointers and sizes, 0 or a negative cabac_hip_status, no
 * exception crosses the boundary), kept in a header of its own like every extension since the NAL one.
 *
 * Why: quantised residual data is almost all zeros (the benchmark's residual tiles: 3.2 % non-zero, 2.7 per block), and the two
 * host-pointer forms that move dense blocks, cabac_hip_encode_batch_residual16 and cabac_hip_residual_parse_batch16, are bound
 * by PCIe.  The forms below move 4 bytes per non-zero coefficient and one 32-bit word per block instead of 2 bytes per
 * coefficient; by bytes the two meet at 50 % non-zero.
 *
 * DEFINITION OF THE RESULT.
 * A block is a cabac_tu_desc, unchanged: coeff_offset places it in a dense array of n_coeff_total elements (int16_t for
 * coeff_bytes 2, int32_t for coeff_bytes 4), raster, stride = width w = 1 << log2_width, height h = 1 << log2_height.
 * The non-zero coefficients of block t are entries[ent_first[t] .. ent_first[t + 1]); ent_first is uint32_t[n_tu + 1],
 * ascending from 0.  An entry is one uint32_t,
 *     pos | (uint32_t)(uint16_t)level << 16,     pos = y * w + x,     level an int16_t.
 * Blocks with max_log2_tr_range above 15 are not carried in this form.
 *
 * cabac_sparse_status: n_entries is the size of the complete result, also when it did not fit (for EXPAND: the length of the
 * list as it was read, min(ent_first[n_tu], the n_entries given)); flags are CABAC_SPARSE_*; first_bad is the lowest block index
 * that raised CABAC_SPARSE_RANGE or a CABAC_SPARSE_BAD_* flag, else 0xFFFFFFFF.
 *
 * A GOOD block has log2_width <= 6, log2_height <= 6 and lies inside the dense array (coeff_offset + w * h <= n_coeff_total).
 * Every other block raises CABAC_SPARSE_BAD_BLOCK, is skipped and has no entries.  Good blocks must not overlap one another.
 *
 * EXPAND (entries -> dense).  Every one of the w * h elements of every good block is written: 0, or the level of its entry
 * (sign-extended for coeff_bytes 4).  Of two entries with the same pos one is taken.  Nothing outside the good blocks' own
 * elements is written.  An entry with pos >= w * h is dropped and raises CABAC_SPARSE_BAD_POS.  A block whose ent_first[t] is
 * above ent_first[t + 1] has no entries, and one whose ent_first[t + 1] is above n_entries is clipped to n_entries; both raise
 * CABAC_SPARSE_BAD_FIRST (the block is still written).
 *
 * COMPACT (dense -> entries).  The coded region of a block — x < min(w, 32), y < min(h, 32), what the binariser reads and the
 * parser writes — is scanned, and its non-zero elements become entries in ascending pos.  Elements outside the coded region
 * are not read.  From 32-bit blocks a level outside int16_t is stored truncated, as cabac_hip_residual_parse16_device does, and
 * raises CABAC_SPARSE_RANGE.  With more entries than entry_capacity the rest is dropped, nothing is written past the capacity and
 * CABAC_SPARSE_OVERFLOW is raised; ent_first and n_entries stay those of the full result.
 *
 * FOUR IDENTITIES, which the tests check:
 *   S1. Compact of expand returns each block's entries sorted by pos, with the same firsts — for distinct positions inside
 *       the coded region and non-zero levels.
 *   S2. Expand of compact reproduces the coded region and zeros the rest of the block.
 *   S3. cabac_hip_sparse_encode_batch gives, bit for bit, every output of cabac_hip_encode_batch_residual16 on the expanded
 *       blocks: payload, offsets, results, tu_info, bin_counts and the return code.  An empty block reports
 *       CABAC_TU_INFO_EMPTY on both.
 *   S4. cabac_hip_sparse_parse_batch gives results and tu_info of cabac_hip_residual_parse_batch16, and the compact of its
 *       coefficients — damaged streams included; blocks behind a stop have no entries.
 */
#ifndef CABAC_HIP_SPARSE_H
#define CABAC_HIP_SPARSE_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cabac_sparse_status {
  uint64_t n_entries; /* size of the complete result, also when it did not fit */
  uint32_t flags;     /* CABAC_SPARSE_* */
  uint32_t first_bad; /* lowest block that raised RANGE or a BAD_* flag, else 0xFFFFFFFF */
} cabac_sparse_status;

#define CABAC_SPARSE_OVERFLOW 0x1u   /* compact: more entries than entry_capacity (the rest is dropped) */
#define CABAC_SPARSE_RANGE 0x2u      /* compact from 32-bit blocks: a level outside int16_t, stored truncated */
#define CABAC_SPARSE_BAD_POS 0x4u    /* expand: pos >= w * h; the entry is dropped */
#define CABAC_SPARSE_BAD_FIRST 0x8u  /* expand: ent_first descends or passes n_entries; clipped */
#define CABAC_SPARSE_BAD_BLOCK 0x10u /* both: log2 size > 6, or the block does not lie inside n_coeff_total; skipped */
#define CABAC_SPARSE_NO_BAD 0xFFFFFFFFu

/* ---- on the host: compact and expand on the CPU, no ctx and no GPU needed ----
 * What a C caller with dense blocks uses to reach the sparse forms below.  coeff_bytes is 2 or 4.  Both return CABAC_HIP_OK
 * with everything else said in *status (an overflow included: what fits is delivered), and CABAC_HIP_ERR_INVALID for a null
 * pointer, another coeff_bytes or n_coeff_total >= 2^32. */
int cabac_hip_sparse_pack_host(uint32_t n_tu, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                               uint32_t *ent_first, uint32_t *entries, uint64_t entry_capacity, cabac_sparse_status *status);
int cabac_hip_sparse_unpack_host(uint32_t n_tu, const cabac_tu_desc *tus, const uint32_t *ent_first, const uint32_t *entries,
                                 uint64_t n_entries, void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                                 cabac_sparse_status *status);

/* ---- device forms ----
 * Asynchronous on the ctx's stream like the other *_device calls (STREAM ORDERING CONTRACT in cabac_hip.h): no host
 * synchronisation inside, no workgroup waits for another.  The scratch (one word per sixteen blocks) belongs to the ctx and is
 * sized from n_tu alone: it grows on the first call of a size, and cabac_hip_workspace_waits does not move on a second
 * call of the same size.  All pointers are device memory; *d_status receives the cabac_sparse_status.  Input and
 * output must not overlap.  n_coeff_total >= 2^32 is refused on the host (firsts are 32-bit).
 * expand: d_ent_first has n_tu + 1 words, d_entries n_entries_max; a zero launch over the blocks' elements, then a scatter
 * launch — stream order between the two is the ordering.  cabac_hip_profile_read reports the call as kind 41, "coefficient
 * expand".
 * compact: d_ent_first receives n_tu + 1 words, d_entries at most entry_capacity; a count launch, a scan of the counts and a
 * write launch that walks the blocks again.  Reported as kind 42, "coefficient compact". */
int cabac_hip_sparse_expand_device(cabac_hip_ctx *ctx, uint32_t n_tu, const cabac_tu_desc *d_tu, const uint32_t *d_ent_first,
                                   const uint32_t *d_entries, uint64_t n_entries_max, void *d_coeff, int coeff_bytes,
                                   uint64_t n_coeff_total, cabac_sparse_status *d_status);
int cabac_hip_sparse_compact_device(cabac_hip_ctx *ctx, uint32_t n_tu, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                    uint64_t n_coeff_total, uint32_t *d_ent_first, uint32_t *d_entries, uint64_t entry_capacity,
                                    cabac_sparse_status *d_status);

/* ---- host-pointer forms (synchronous) ----
 * cabac_hip_sparse_encode_batch: cabac_hip_encode_batch_residual16 with (ent_first, entries, n_entries_total) in place of the
 * dense coefficients; n_coeff_total still sizes the dense array the blocks' coeff_offset point into, which exists on the device
 * only.  Checked on the host (by up to eight threads for a large batch) while the lists are on the wire, before the pipeline
 * runs and before any output is touched: ent_first ascending from 0 to n_entries_total, every pos < w * h, no block with
 * max_log2_tr_range above 15 — otherwise CABAC_HIP_ERR_INVALID, with cabac_hip_last_error naming the block.  Then the lists
 * are expanded into the library's 16-bit coefficient buffer and the unchanged pipeline of cabac_hip_encode_residual16_device
 * runs (S3).  It uses that pipeline's buffers: while a fixed workspace is in force (cabac_hip_workspace.h) it is refused like
 * the pipeline's other host-pointer forms. */
int cabac_hip_sparse_encode_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                  uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                  const cabac_tu_desc *tus, const uint32_t *ent_first, const uint32_t *entries,
                                  uint64_t n_entries_total, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                                  uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *tu_info,
                                  uint32_t *bin_counts);
/* cabac_hip_sparse_parse_batch: cabac_hip_residual_parse_batch16 with (ent_first, entries, entry_capacity, status) in place of
 * the dense coefficients (S4): the library's dense buffer is zeroed, the unchanged parser runs, its blocks are compacted, and the
 * status, the n_tu + 1 firsts and exactly status->n_entries entries come back, with two waits.  A capacity that is too small
 * returns CABAC_HIP_ERR_INVALID with status->n_entries telling the need; firsts, results and tu_info are delivered and no
 * entries.  Otherwise CABAC_HIP_ERR_SUBSTREAM if any result flag is set (everything is delivered).  It is not a fixed-workspace call
 * and is not refused while one is in force. */
int cabac_hip_sparse_parse_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                 uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, uint32_t *ent_first,
                                 uint32_t *entries, uint64_t entry_capacity, uint64_t n_coeff_total, uint32_t *tu_info,
                                 cabac_substream_result *results, cabac_sparse_status *status);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_SPARSE_H */
