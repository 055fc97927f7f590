// The packed bin records on the CPU (declared in include/cabac_hip_rec10.h): cabac_hip_rec10_bytes, cabac_hip_rec10_pack_host and
// cabac_hip_rec10_unpack_host, the block layout of the header's DEFINITION OF THE RESULT written out.  No HIP include and no ctx:
// a plain C++ compiler builds this file alone (the sanitizer test does), and callers without a GPU can use it.
#include <cstdint>
#include <cstring>

#include "cabac_hip_rec10.h"

namespace {

// one block from up to 64 records (the rest of the block is zero); returns the OR of the records
uint32_t pack_block(const uint16_t *rec, uint32_t n, uint8_t *blk) {
  uint64_t hi = 0, bin = 0;
  uint32_t seen = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t r = rec[i];
    seen |= r;
    blk[i] = uint8_t(r);
    hi |= uint64_t((r >> 8) & 1u) << i;
    bin |= uint64_t(r >> 15) << i;
  }
  if (n < CABAC_REC10_BLOCK_RECORDS) std::memset(blk + n, 0, CABAC_REC10_BLOCK_RECORDS - n);
  for (uint32_t k = 0; k < 8; k++) {  // little-endian whatever the host is
    blk[64 + k] = uint8_t(hi >> (8 * k));
    blk[72 + k] = uint8_t(bin >> (8 * k));
  }
  return seen;
}

uint64_t plane(const uint8_t *p) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; k++) v |= uint64_t(p[k]) << (8 * k);
  return v;
}

}  // namespace

extern "C" {

int cabac_hip_rec10_bytes(uint64_t n_records, uint64_t *bytes) {
  if (!bytes) return CABAC_HIP_ERR_INVALID;
  *bytes = CABAC_REC10_BYTES(n_records);
  return CABAC_HIP_OK;
}

int cabac_hip_rec10_pack_host(const uint16_t *records, uint64_t n_records, uint8_t *packed, uint64_t packed_capacity,
                              uint64_t *first_bad) {
  if (first_bad) *first_bad = UINT64_MAX;
  if (n_records && (!records || !packed)) return CABAC_HIP_ERR_INVALID;
  if (packed_capacity < CABAC_REC10_BYTES(n_records)) return CABAC_HIP_ERR_INVALID;
  uint64_t bad = UINT64_MAX;
  for (uint64_t lo = 0; lo < n_records; lo += CABAC_REC10_BLOCK_RECORDS) {
    const uint32_t n = uint32_t(n_records - lo < CABAC_REC10_BLOCK_RECORDS ? n_records - lo : CABAC_REC10_BLOCK_RECORDS);
    const uint32_t seen = pack_block(records + lo, n, packed + (lo >> 6) * CABAC_REC10_BLOCK_BYTES);
    if ((seen & CABAC_REC10_RESERVED_BITS) && bad == UINT64_MAX)
      for (uint32_t i = 0; i < n; i++)
        if (records[lo + i] & CABAC_REC10_RESERVED_BITS) {
          bad = lo + i;
          break;
        }
  }
  if (first_bad) *first_bad = bad;
  return bad == UINT64_MAX ? CABAC_HIP_OK : CABAC_HIP_ERR_INVALID;
}

int cabac_hip_rec10_unpack_host(const uint8_t *packed, uint64_t first, uint64_t n, uint16_t *records) {
  if (n && (!packed || !records)) return CABAC_HIP_ERR_INVALID;
  if (n > UINT64_MAX - first) return CABAC_HIP_ERR_INVALID;
  const uint64_t end = first + n;
  for (uint64_t r = first; r < end;) {
    const uint8_t *blk = packed + (r >> 6) * CABAC_REC10_BLOCK_BYTES;
    const uint64_t hi = plane(blk + 64), bin = plane(blk + 72);
    const uint64_t stop = ((r >> 6) + 1) << 6 < end ? ((r >> 6) + 1) << 6 : end;
    for (; r < stop; r++) {
      const uint32_t i = uint32_t(r & 63u);
      records[r] = uint16_t(blk[i] | ((hi >> i) & 1u) << 8 | ((bin >> i) & 1u) << 15);
    }
  }
  return CABAC_HIP_OK;
}

}  // extern "C"
