/*
 * cabac_hip_rec10.h — C ABI of the packed bin records of libcabac_hip.so ("rec10"): ten bits per record instead of sixteen on
 * the way to the device, packed and unpacked on the host and on the device, and the host-pointer encode and decode calls that
 * take their records in this form.  An extension of cabac_hip.h (same conventions: plain pointers and sizes, 0 or a negative
 * cabac_hip_status, no exception crosses the boundary), kept in a header of its own like every extension since the NAL one.
 *
 * Why: a bin record is a 9-bit context id and a bin; bits 14..9 are zero by definition (cabac_hip.h).  The host-pointer forms
 * cabac_hip_encode_batch and cabac_hip_decode_batch are bound by PCIe, and the records are most of what they send.  Ten bits
 * instead of sixteen take 37.5 % off those bytes.
 *
 * DEFINITION OF THE RESULT.
 * Records are grouped by their index r in records[], the same global index that desc[s].rec_offset counts; where substreams
 * start plays no part.  Block b covers records 64 b .. 64 b + 63 and is 80 bytes at byte offset 80 b:
 *     bytes  0 .. 63   byte i = bits 7..0 of the id of record 64 b + i
 *     bytes 64 .. 71   little-endian uint64_t, bit i = bit 8 of that id
 *     bytes 72 .. 79   little-endian uint64_t, bit i = the record's bin (bit 15 of the record)
 * CABAC_REC10_BYTES(n) = ((n + 63) / 64) * 80 bytes hold n records.  Records behind n in the last block are packed as zero.
 * A packed buffer is readable for all of CABAC_REC10_BYTES(n) bytes.  Device pointers to packed data are 16-byte aligned; a
 * misaligned one is refused with CABAC_HIP_ERR_INVALID from the pointer value alone.
 * Every 80-byte pattern is a valid block: it unpacks to 64 records with bits 14..9 zero.  Ids 379 .. 0x1FA survive packing and
 * still produce CABAC_RES_BAD_RECORD in the kernels.  A record with any of bits 14..9 set cannot be represented, and packing
 * refuses it: the packed path never turns a bad record into a good one.
 * The 64-bit planes are chosen for the wave: on the device a block is one 64-lane ballot per plane when one lane packs one
 * record, and one bit test per record when unpacking; blocks are 16-byte aligned, so both directions use 16-byte accesses.
 *
 * FOUR IDENTITIES, which the tests check:
 *   R1. unpack_host(pack_host(r)) == r for every r with clear reserved bits and every n, and cabac_rec10_put / cabac_rec10_get
 *       agree with both.
 *   R2. unpack_device == unpack_host on arbitrary packed bytes and arbitrary [first, first + n).
 *   R3. pack_device == pack_host byte for byte, zero tail included, and the same first bad index.
 *   R4. Each rec10 batch form returns, for pack_host(r), exactly the bytes, offsets, bins, results and status that its u16 form
 *       returns for r.
 */
#ifndef CABAC_HIP_REC10_H
#define CABAC_HIP_REC10_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CABAC_REC10_BLOCK_RECORDS 64u
#define CABAC_REC10_BLOCK_BYTES 80u
#define CABAC_REC10_BYTES(n) ((((uint64_t)(n) + 63u) / 64u) * 80u)
#define CABAC_REC10_RESERVED_BITS 0x7E00u /* bits 14..9 of a record: packing refuses a record that has one set */

typedef struct cabac_rec10_status {
  uint64_t first_bad; /* smallest index of a record with reserved bits set, else UINT64_MAX */
  uint32_t flags;     /* CABAC_REC10_* */
  uint32_t reserved;  /* 0 */
} cabac_rec10_status;

#define CABAC_REC10_BAD_BITS 0x1u /* pack: a record had reserved bits set; they are dropped in the output */
#define CABAC_REC10_OVERFLOW 0x2u /* pack: packed_capacity below CABAC_REC10_BYTES(n_records); nothing is written */

/* ---- one record at a time: what a recorder uses to write the format directly and never pay for a pack pass ----
 * Read-modify-write on the three places of record r; the reserved bits of `record` are dropped.  A buffer that starts as zeros
 * and receives its records through cabac_rec10_put is what cabac_hip_rec10_pack_host makes of them. */
static inline void cabac_rec10_put(uint8_t *packed, uint64_t r, uint16_t record) {
  uint8_t *blk = packed + (r >> 6) * CABAC_REC10_BLOCK_BYTES;
  const unsigned i = (unsigned)(r & 63u);
  const uint8_t bit = (uint8_t)(1u << (i & 7u));
  uint8_t *hi = blk + 64 + (i >> 3), *bin = blk + 72 + (i >> 3);
  blk[i] = (uint8_t)(record & 0xFFu);
  *hi = (uint8_t)((record & 0x100u) ? (*hi | bit) : (*hi & ~bit));
  *bin = (uint8_t)((record & 0x8000u) ? (*bin | bit) : (*bin & ~bit));
}
static inline uint16_t cabac_rec10_get(const uint8_t *packed, uint64_t r) {
  const uint8_t *blk = packed + (r >> 6) * CABAC_REC10_BLOCK_BYTES;
  const unsigned i = (unsigned)(r & 63u);
  const unsigned hi = (blk[64 + (i >> 3)] >> (i & 7u)) & 1u, bin = (blk[72 + (i >> 3)] >> (i & 7u)) & 1u;
  return (uint16_t)(blk[i] | hi << 8 | bin << 15);
}

/* ---- on the host: no ctx and no GPU needed ----
 * bytes: *bytes = CABAC_REC10_BYTES(n_records).
 * pack_host: all CABAC_REC10_BYTES(n_records) bytes are written, the zero tail of the last block included.  A
 * packed_capacity below that returns CABAC_HIP_ERR_INVALID and nothing is written; *first_bad is then UINT64_MAX.  A record
 * with reserved bits set returns CABAC_HIP_ERR_INVALID too, with *first_bad the smallest such index (the output is written
 * with those bits dropped, as the device form does); otherwise *first_bad is UINT64_MAX.  first_bad may be NULL.
 * unpack_host: writes records first .. first + n - 1 to records[first ..] and nothing else. */
int cabac_hip_rec10_bytes(uint64_t n_records, uint64_t *bytes);
int cabac_hip_rec10_pack_host(const uint16_t *records, uint64_t n_records, uint8_t *packed, uint64_t packed_capacity,
                              uint64_t *first_bad);
int cabac_hip_rec10_unpack_host(const uint8_t *packed, uint64_t first, uint64_t n, uint16_t *records);

/* ---- device forms ----
 * Asynchronous on the ctx's stream like the other *_device calls (STREAM ORDERING CONTRACT in cabac_hip.h): no host
 * synchronisation inside, nothing is allocated, no workgroup waits for another.  All pointers are device memory; input and
 * output must not overlap.
 * unpack: writes d_records[first .. first + n) and nothing else; first is arbitrary.  The blocks that hold those records are
 * read whole.  One launch; cabac_hip_profile_read reports it as kind 43, "record unpack".
 * pack: the call resets *d_status on the stream itself, then one launch writes all CABAC_REC10_BYTES(n_records) bytes.  A
 * record with reserved bits set raises CABAC_REC10_BAD_BITS with the smallest offending index in first_bad (an atomic minimum
 * from the vector unit); the bits are dropped in the output.  A packed_capacity that is short raises CABAC_REC10_OVERFLOW
 * and nothing is written.  Reported as kind 44, "record pack". */
int cabac_hip_rec10_unpack_device(cabac_hip_ctx *ctx, const uint8_t *d_packed, uint64_t first, uint64_t n, uint16_t *d_records);
int cabac_hip_rec10_pack_device(cabac_hip_ctx *ctx, const uint16_t *d_records, uint64_t n_records, uint8_t *d_packed,
                                uint64_t packed_capacity, cabac_rec10_status *d_status);

/* ---- host-pointer forms (synchronous) ----
 * cabac_hip_encode_batch, cabac_hip_encode_batch_payload, cabac_hip_decode_batch and cabac_hip_decode_batch_packed with
 * (packed, packed_bytes) in place of the 16-bit records (R4).  packed_bytes below CABAC_REC10_BYTES(n_records_total) is
 * refused with CABAC_HIP_ERR_INVALID before anything is queued.  Everything else is the 16-bit forms': the same checks of
 * the descriptors, the same chunks, streams and events, the same drain on an error return and the same error texts.  For each
 * chunk the blocks that hold its records go up (pinned memory is DMA'd where it lies, pageable memory goes through the
 * bounce ring) and a record unpack launch runs on the chunk's stream in front of its encode or decode launch; a block that two
 * chunks share may go up twice, but every chunk unpacks its own records only.
 * decode: bins_packed != 0 delivers the bins eight to a byte, (n_records_total + 7) / 8 bytes; 0 one per byte.  The bin
 * plane of the input is ignored. */
int cabac_hip_rec10_encode_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                 uint64_t packed_bytes, uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total,
                                 cabac_substream_result *results);
int cabac_hip_rec10_encode_batch_payload(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                         uint64_t packed_bytes, uint64_t n_records_total, uint8_t *payload, uint64_t payload_capacity,
                                         uint64_t *payload_offsets, cabac_substream_result *results);
int cabac_hip_rec10_decode_batch(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                 uint64_t packed_bytes, uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total,
                                 uint8_t *bins, int bins_packed, cabac_substream_result *results);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_REC10_H */
