/*
 * cabac_hip_nal.h — C ABI of the emulation prevention of libcabac_hip.so: a segmented byte string (the payload and the
 * n_seg + 1 offsets cabac_hip_assemble_device produces) to NAL payload bytes and back, on the device.  An extension of
 * cabac_hip.h (same conventions: plain pointers and sizes, 0 or a negative cabac_hip_status, no exception crosses the
 * boundary), kept in a header of its own: the reference-side test libraries (oracle/Makefile) are pinned to the content of
 * cabac_hip.h, and nothing declared here changes what they were compiled against.
 *
 * DEFINITION OF THE RESULT.  The reference counts the bytes an escape would insert (OutputBitstream::
 * countStartCodeEmulations, bit_stream.cpp:157-181) and carries the positions of removed ones (InputBitstream::
 * m_emulationPreventionByteLocation, bit_stream.hpp:106, :159-164); the routines that insert and remove them belong to VTM's
 * NAL writer and NALread, which are not part of it.  So the two walks below, not VTM, are the contract.
 *
 * ESCAPE.  Walk the whole payload once, carrying z, the number of consecutive zero bytes just written, starting at 0.
 * Before a byte b with z == 2 && b <= 3 emit 03 and set z = 0.  Then emit b and set z = (b == 0) ? z + 1 : 0.
 *   - The walk runs across segment boundaries: the result is the escape of the concatenation.
 *   - Nothing is appended after the last byte.  A payload whose last byte is 00 only sets CABAC_NAL_TRAILING_ZERO (RBSP data
 *     ends in its stop bit; cabac_zero_words are not written here).
 *   - An inserted byte belongs to the segment of the byte it precedes:
 *       nal_offsets[s] = offsets[s] + (insertions in front of raw positions < offsets[s]).
 *   - The number of insertions inside a string equals countStartCodeEmulations() of it.  Substreams coded with
 *     CABAC_SUB_ALIGN_RBSP end in a non-zero byte, so z is 0 at every boundary and the growth of segment s,
 *     (nal_offsets[s + 1] - nal_offsets[s]) - (offsets[s + 1] - offsets[s]), is what cabac_hip_count_emulations_device reports
 *     for substream s.  The entry points of the slice header are the differences of nal_offsets.
 *   - Worst case one insertion per two input bytes: cabac_hip_nal_escape_bound(n) = n + n / 2.
 * UNESCAPE.  Walk the NAL bytes with z the number of consecutive zero bytes just read.  A byte 03 met with z == 2 is dropped,
 * its position is recorded and z = 0.  Every other byte is copied and sets z = (b == 0) ? z + 1 : 0.
 *   - offsets[s] = nal_offsets[s] - (removals at NAL positions < nal_offsets[s]).
 *   - Unescape of escape is the identity on bytes and offsets.
 *   - locations[k] = (position of the k-th removed byte in the NAL string) + loc_base, as uint32_t: ready for
 *     InputBitstream::setEmulationPreventionByteLocation.
 *   - Input no escape produces is copied as the walk says and flagged: CABAC_NAL_FORBIDDEN for a byte <= 02 behind two or more
 *     zeros, CABAC_NAL_BAD_ESCAPE for a dropped 03 followed by a byte > 03.  A string that ends in 00 00 03 is legal.
 */
#ifndef CABAC_HIP_NAL_H
#define CABAC_HIP_NAL_H

#include "cabac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cabac_nal_status {
  uint64_t out_bytes; /* size of the complete result, also when it did not fit */
  uint32_t n_changed; /* bytes inserted (escape) / removed (unescape); saturates at 2^32 - 1 */
  uint32_t flags;     /* CABAC_NAL_* */
} cabac_nal_status;

/* result longer than the capacity: bytes beyond it are dropped, nothing is written past it, out_bytes / offsets / n_changed
 * are still those of the full result */
#define CABAC_NAL_OVERFLOW 0x1u
#define CABAC_NAL_TRAILING_ZERO 0x2u  /* escape: the payload's last byte is 00 (the caller owes a trailing 03) */
#define CABAC_NAL_FORBIDDEN 0x4u      /* unescape: 00 00 {00,01,02} in the input */
#define CABAC_NAL_BAD_ESCAPE 0x8u     /* unescape: a removed 03 is followed by a byte > 03 */
#define CABAC_NAL_LOC_OVERFLOW 0x10u  /* unescape: more removals than loc_capacity (the first loc_capacity are recorded) */
#define CABAC_NAL_INPUT_CLIPPED 0x20u /* the input is longer than the *_bytes_max the host gave: only that much was read */

/* n_bytes + n_bytes / 2: the largest escape of n_bytes bytes (reached by an all-zero string of odd length) */
size_t cabac_hip_nal_escape_bound(uint64_t n_bytes);

/* ---- device forms ----
 * The length of the input is d_offsets[n_seg] (d_nal_offsets[n_seg] for unescape), read ON THE DEVICE: nothing is synchronised
 * and nothing is copied to the host.  The host passes an upper bound it does know, payload_bytes_max / nal_bytes_max — e.g. the
 * payload_capacity it gave cabac_hip_assemble_device — from which the grid and the scratch are sized; the bound may be several
 * times the real length (a piece of the grid behind the real length reads one word and returns).  A real length above the bound is
 * clipped to it and sets CABAC_NAL_INPUT_CLIPPED; offsets beyond it are clipped likewise.  The offsets are ascending, the
 * first one is 0.  Empty segments are valid.  n_seg == 0 with a NULL offsets pointer is valid and only writes an all-zero
 * status.  Input and output must not overlap.  d_nal_offsets / d_offsets receive n_seg + 1 entries, *d_status (device memory)
 * the cabac_nal_status; offsets, out_bytes and n_changed are those of the complete result also when it overflows the capacity.
 * Offsets are 64-bit; locations are 32-bit, so a location list of a NAL string that (with loc_base) passes 4 GiB wraps —
 * the device form does not see that, the host form refuses it.
 * Asynchronous on the ctx's stream like the other *_device calls (STREAM ORDERING CONTRACT in cabac_hip.h), no host
 * synchronisation inside; the scratch (per-KiB summaries and their scans) belongs to the ctx.  cabac_hip_profile_read reports
 * these calls as kind 13, "nal escape", and kind 14, "nal unescape", after the kinds listed in cabac_hip.h and
 * cabac_hip_estimate.h. */
int cabac_hip_nal_escape_device(cabac_hip_ctx *ctx, uint32_t n_seg, const uint64_t *d_offsets, const uint8_t *d_payload,
                                uint64_t payload_bytes_max, uint8_t *d_nal, uint64_t nal_capacity, uint64_t *d_nal_offsets,
                                cabac_nal_status *d_status);
/* d_locations may be NULL (no list, no CABAC_NAL_LOC_OVERFLOW) */
int cabac_hip_nal_unescape_device(cabac_hip_ctx *ctx, uint32_t n_seg, const uint64_t *d_nal_offsets, const uint8_t *d_nal,
                                  uint64_t nal_bytes_max, uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_offsets,
                                  uint32_t *d_locations, uint64_t loc_capacity, uint32_t loc_base, cabac_nal_status *d_status);

/* ---- host-pointer forms (synchronous; *status in host memory) ----
 * The same on host arrays: offsets[0 .. n_seg] ascending from 0, payload / nal holding offsets[n_seg] bytes.  An overflow of
 * nal_capacity / payload_capacity / loc_capacity is reported in status->flags as by the device forms (the call returns
 * CABAC_HIP_OK; what fits is delivered).  CABAC_HIP_ERR_INVALID for offsets that are not ascending from 0, and for a location
 * list of a NAL string whose last position plus loc_base does not fit 32 bits. */
int cabac_hip_nal_escape_batch(cabac_hip_ctx *ctx, uint32_t n_seg, const uint64_t *offsets, const uint8_t *payload, uint8_t *nal,
                               uint64_t nal_capacity, uint64_t *nal_offsets, cabac_nal_status *status);
int cabac_hip_nal_unescape_batch(cabac_hip_ctx *ctx, uint32_t n_seg, const uint64_t *nal_offsets, const uint8_t *nal,
                                 uint8_t *payload, uint64_t payload_capacity, uint64_t *offsets, uint32_t *locations,
                                 uint64_t loc_capacity, uint32_t loc_base, cabac_nal_status *status);

/* Records in, NAL-ready payload out: exactly what cabac_hip_encode_batch_payload followed by the escape of its payload gives,
 * with no host pass over the bytes (upload, encode, assemble, escape, one download).  nal_offsets[0 .. n_sub]: the entry
 * points.  A result that does not fit nal_capacity returns CABAC_HIP_ERR_INVALID with status->out_bytes telling the size
 * needed (nal_offsets, results and status are delivered, no bytes); CABAC_HIP_ERR_SUBSTREAM as cabac_hip_encode_batch. */
int cabac_hip_encode_batch_nal(cabac_hip_ctx *ctx, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, uint8_t *nal, uint64_t nal_capacity, uint64_t *nal_offsets,
                               cabac_substream_result *results, cabac_nal_status *status);

#ifdef __cplusplus
}
#endif
#endif /* CABAC_HIP_NAL_H */
