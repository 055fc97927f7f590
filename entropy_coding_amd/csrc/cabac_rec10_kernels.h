// Internal launch interface between the packed-record kernels (cabac_rec10.hip) and the C ABI (cabac_capi.cpp).
#ifndef CABAC_REC10_KERNELS_H
#define CABAC_REC10_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip_rec10.h"

namespace cabac {

// packed (16-byte aligned) -> records[first .. first + n): one launch, eight records per lane
hipError_t launch_rec10_unpack(hipStream_t st, const uint8_t *packed, uint64_t first, uint64_t n, uint16_t *records);
// records[0 .. n) -> packed (16-byte aligned): the status reset, then one launch over all CABAC_REC10_BYTES(n) bytes; with a
// packed_capacity that is short only the reset runs, and it leaves CABAC_REC10_OVERFLOW behind
hipError_t launch_rec10_pack(hipStream_t st, const uint16_t *records, uint64_t n, uint8_t *packed, uint64_t packed_capacity,
                             cabac_rec10_status *status);

}  // namespace cabac
#endif
