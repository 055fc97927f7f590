// The fixed workspace (cabac_hip_workspace.h): what the host used to decide after its wait in the middle of the splice pipeline,
// the plan write and the winner log's emit is decided on the device.  Most of it lives where the work already was:
//   splice_scan_gate_kernel (cabac_splice.hip)   the scan over the substreams, with THE GATE as its tail: good or VOIDED, the
//                                                status, a voided call's tables emptied
//   splice_expand_kernel<true>, splice_sync_index_kernel<true>: one word read at their top; the binariser's records pass
//                                                finds no block in the order the gate emptied
//   sizes_scan_kernel<true> (cabac_assemble.hip) a voided call's results, {0, CABAC_RES_OVERFLOW}; its sizes are all 0
//   log_place_*_fixed_kernel (cabac_search_emit.hip)   the log's place pass from counters that stay on the device
// The headline encode kernels take no part: the descriptors of a voided call (empty, zero-capacity slots) make them harmless.
// Here: the two kernels that exist on the fixed path alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_kernels.h"

namespace cabac {

__global__ __launch_bounds__(256) void ws_out_sets_kernel(const WsState *__restrict__ ws, uint32_t n_sub, const uint32_t *__restrict__ out_set,
                                                          uint32_t *__restrict__ out_set_live) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < n_sub) out_set_live[s] = ws->voided != 0u ? 0xffffffffu : out_set[s];
}

__global__ __launch_bounds__(256) void ws_log_info_kernel(const WsState *__restrict__ ws, uint32_t cap, const uint32_t *__restrict__ src,
                                                          uint32_t *__restrict__ dst) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < cap && t < ws->log_tu) dst[t] = src[t];
}

hipError_t launch_ws_out_sets(hipStream_t st, const WsState *ws, uint32_t n_sub, const uint32_t *out_set, uint32_t *out_set_live) {
  if (n_sub) hipLaunchKernelGGL(ws_out_sets_kernel, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, ws, n_sub, out_set, out_set_live);
  return hipGetLastError();
}

hipError_t launch_ws_log_info(hipStream_t st, const WsState *ws, uint32_t cap, const uint32_t *src, uint32_t *dst) {
  if (cap) hipLaunchKernelGGL(ws_log_info_kernel, dim3((cap + 255u) / 256u), dim3(256), 0, st, ws, cap, src, dst);
  return hipGetLastError();
}

}  // namespace cabac
