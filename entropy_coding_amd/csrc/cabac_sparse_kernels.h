// Internal launch interface between the sparse coefficient transport's kernels (cabac_sparse.hip) and the C ABI (cabac_capi.cpp).
#ifndef CABAC_SPARSE_KERNELS_H
#define CABAC_SPARSE_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip_sparse.h"

namespace cabac {

// scratch: sparse_scratch_bytes(n_tu) bytes of device memory a launch may overwrite (the error words and one count per
// workgroup of sixteen blocks), sized from n_tu alone
size_t sparse_scratch_bytes(uint32_t n_tu);
// entries -> dense: the error words cleared, the zero launch, the scatter launch (4 or 16 lanes per block, by the mean length of
// a block's list), the status
hipError_t launch_sparse_expand(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const uint32_t *ent_first, const uint32_t *entries,
                                uint64_t n_entries_max, void *coeff, int coeff_bytes, uint64_t n_coeff_total, cabac_sparse_status *status,
                                void *scratch);
// dense -> entries: the count launch, the scan (firsts' bases and the status), the write launch
hipError_t launch_sparse_compact(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tu, const void *coeff, int coeff_bytes,
                                 uint64_t n_coeff_total, uint32_t *ent_first, uint32_t *entries, uint64_t entry_capacity,
                                 cabac_sparse_status *status, void *scratch);

}  // namespace cabac
#endif
