// Internal launch interface between the emulation-prevention kernels (cabac_nal.hip) and the C ABI (cabac_capi.cpp).
#ifndef CABAC_NAL_KERNELS_H
#define CABAC_NAL_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip_nal.h"

namespace cabac {

// scratch: nal_scratch_bytes(bytes_max) bytes of device memory a launch may overwrite (chunk summaries and their scans), sized
// from the bound the host knows, like the grids; the length itself (offsets[n_seg]) is read on the device
size_t nal_scratch_bytes(uint64_t bytes_max);
hipError_t launch_nal_escape(hipStream_t st, uint32_t n_seg, const uint64_t *offsets, const uint8_t *payload, uint64_t payload_bytes_max,
                             uint8_t *nal, uint64_t nal_capacity, uint64_t *nal_offsets, cabac_nal_status *status, void *scratch);
hipError_t launch_nal_unescape(hipStream_t st, uint32_t n_seg, const uint64_t *nal_offsets, const uint8_t *nal, uint64_t nal_bytes_max,
                               uint8_t *payload, uint64_t payload_capacity, uint64_t *offsets, uint32_t *locations, uint64_t loc_capacity,
                               uint32_t loc_base, cabac_nal_status *status, void *scratch);

}  // namespace cabac
#endif
