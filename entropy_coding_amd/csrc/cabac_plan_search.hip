// The plan resolve of the search rounds (cabac_hip_search_plan.h): a candidate given as a plan, the values of its real elements
// and its blocks' coefficients -> the unit-candidate form of cabac_hip_search_unit.h, which the unit estimate, the select, the
// commit and the winner log take unchanged.
//
//   residual sizes pass (cabac_residual.hip)  ->  the info word of every block, whatever its guard will say
//   plan_resolve_count_kernel   per candidate: the walk for its counts — side records needed, the stop
//   plan_resolve_scan_kernel    across candidates: rec_first, the total, and the capacity decision (all or nothing), on the device
//   plan_resolve_emit_kernel    the same walk again, now writing: the coded elements' bins by OUTPUT position, per block the side
//                               records in front of it and its descriptor (one the binariser rejects where it is skipped), the
//                               filled values, the info words; a stopped candidate or a call that does not fit gets the empty form
//   plan_flag_cost_kernel       a flagged candidate costs UINT64_MAX (between the unit estimate and the select)
//
// The walk is cabac_plan_walk.h's, one wave per candidate; this file says where a candidate's plan lies and where its results go.
// A candidate's run holds its elements' bins alone: a block adds nothing to it, only its position.  No atomics, no kernel waits
// for another workgroup, every loop is bounded by the candidate's entries, its blocks and the number of candidates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_hip_parse_elements.h"
#include "cabac_hip_parse_plan.h"
#include "cabac_kernels.h"
#include "cabac_plan_walk.h"

namespace cabac {

namespace {

// the plan resolve as cabac_plan_walk.h sees it: a unit is a candidate, its run is its side records
struct PsIo {
  static constexpr bool kBlocksInRun = false;
  uint32_t n_units;
  const uint32_t *cand_first;
  const uint64_t *ent_first;
  const uint32_t *plan, *values;
  uint32_t n_tu;
  const cabac_tu_desc *tus;
  const uint32_t *tu_at, *tu_guard, *tu_n_records /* not read */, *tu_info;
  uint32_t *cnt, *flags;  // first walk writes, second walk reads
  const uint64_t *rec_first;
  uint32_t *tu_at_out;
  cabac_tu_desc *tus_out;
  uint32_t *values_out, *tu_info_out;
  uint16_t *records;

  // entries and blocks of candidate c, clipped as cabac_hip_search_unit.h clips side runs and blocks (the blocks to the n_tu the
  // caller's arrays hold besides)
  __device__ __forceinline__ PlanWalkUnit unit(uint32_t c) const {
    const uint64_t n_all = ent_first[n_units];
    const uint64_t first = min(ent_first[c], n_all), end = max(min(ent_first[c + 1u], n_all), first);
    const uint32_t t_all = min(cand_first[n_units], n_tu);
    PlanWalkUnit u;
    u.plan = reinterpret_cast<const uint2 *>(plan) + first;
    u.vin = values + first;
    u.vout = values_out ? values_out + first : nullptr;
    u.n = (uint32_t)min(end - first, (uint64_t)0xffffffffu);
    u.t0 = min(cand_first[c], t_all);
    u.t1 = max(min(cand_first[c + 1u], t_all), u.t0);
    return u;
  }
  __device__ __forceinline__ void count_end(uint32_t c, bool bad_rec, bool bad_val, uint64_t off) const {
    // (positions in a run are 32 bits: a candidate that outgrows them fits no capacity)
    const uint32_t flag = bad_rec ? CABAC_RES_BAD_RECORD : bad_val ? CABAC_RES_BAD_VALUE : off > 0xffffffffull ? CABAC_RES_OVERFLOW : 0u;
    flags[c] = flag;
    cnt[c] = flag ? 0u : (uint32_t)off;
  }
  __device__ __forceinline__ bool emit_begin(uint32_t c, const PlanWalkUnit &u, uint32_t lane, uint64_t &base) const {
    base = rec_first[c];
    if (flags[c] == 0u) return true;
    // stopped, or the call does not fit: an empty run, every block rejected in front of it
    for (uint32_t t = u.t0 + lane; t < u.t1; t += 64u) {
      cabac_tu_desc d = tus[t];
      d.log2_width = d.log2_height = 7;
      tus_out[t] = d;
      tu_at_out[t] = 0u;
    }
    return false;
  }
  __device__ __forceinline__ void emit_block(uint32_t t, bool coded, uint64_t, uint64_t off, uint32_t, uint32_t info) const {
    cabac_tu_desc d = tus[t];
    if (!coded) d.log2_width = d.log2_height = 7;  // one the binariser rejects; its coeff_offset stays
    tus_out[t] = d;
    tu_at_out[t] = (uint32_t)off;
    if (tu_info_out) tu_info_out[t] = info;
  }
};

__device__ __forceinline__ PsIo ps_io(const PlanResolveIn &in, uint32_t *cnt, uint32_t *flags, const PlanResolveOut &out) {
  return PsIo{in.n_cand, in.cand_first, in.ent_first, in.plan, in.values, in.n_tu, in.tus, in.tu_at, in.tu_guard, nullptr, in.tu_info,
              cnt, flags, out.rec_first, out.tu_at_out, out.tus_out, out.values_out, out.tu_info_out, out.records};
}

}  // namespace

__global__ __launch_bounds__(64 * kPwWaves) void plan_resolve_count_kernel(PlanResolveIn in, uint32_t *__restrict__ cnt,
                                                                            uint32_t *__restrict__ flags) {
  plan_walk<false>(ps_io(in, cnt, flags, PlanResolveOut{}));
}

__global__ __launch_bounds__(64 * kPwWaves) void plan_resolve_emit_kernel(PlanResolveIn in, uint32_t *cnt, uint32_t *flags,
                                                                           PlanResolveOut out) {
  plan_walk<true>(ps_io(in, cnt, flags, out));
}

// rec_first[c] = the records of the candidates in front of c, rec_first[n_cand] = all of them, *total (may be null) = the need.
// A need above the capacity: every rec_first entry 0 and CABAC_RES_OVERFLOW on every candidate that has no flag yet, which is
// what makes the second walk write the empty form.  One workgroup; thread k owns the candidates k, k + 1024, ... in both loops.
__global__ __launch_bounds__(1024) void plan_resolve_scan_kernel(uint32_t n_cand, const uint32_t *__restrict__ cnt,
                                                                 uint32_t *__restrict__ flags, uint64_t capacity,
                                                                 uint64_t *__restrict__ rec_first, uint64_t *__restrict__ total) {
  __shared__ uint64_t wave_sum[16];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t tile = 0; tile < n_cand; tile += 1024u) {
    const uint32_t c = tile + tid;
    const uint64_t a = c < n_cand ? cnt[c] : 0;
    uint64_t incl = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t base = carry;
    for (uint32_t k = 0; k < wave; k++) base += wave_sum[k];
    if (c < n_cand) rec_first[c] = base + incl - a;
    __syncthreads();
    if (tid == 1023) carry = base + incl;
    __syncthreads();
  }
  const uint64_t need = carry;
  const bool fits = need <= capacity;
  if (!fits)
    for (uint32_t c = tid; c < n_cand; c += 1024u) {
      rec_first[c] = 0;
      if (flags[c] == 0u) flags[c] = CABAC_RES_OVERFLOW;
    }
  if (tid == 0) {
    rec_first[n_cand] = fits ? need : 0;
    if (total) *total = need;
  }
}

__global__ __launch_bounds__(256) void plan_flag_cost_kernel(uint32_t n_cand, const uint32_t *__restrict__ flags,
                                                             uint64_t *__restrict__ frac_bits) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < n_cand && flags[c] != 0u) frac_bits[c] = ~0ull;
}

hipError_t launch_plan_resolve_count(hipStream_t st, const PlanResolveIn &in, uint32_t *cnt, uint32_t *flags) {
  if (in.n_cand)
    hipLaunchKernelGGL(plan_resolve_count_kernel, dim3((in.n_cand + kPwWaves - 1u) / kPwWaves), dim3(64 * kPwWaves), 0, st, in, cnt, flags);
  return hipGetLastError();
}

hipError_t launch_plan_resolve_scan(hipStream_t st, uint32_t n_cand, const uint32_t *cnt, uint32_t *flags, uint64_t capacity,
                                    uint64_t *rec_first, uint64_t *total) {
  hipLaunchKernelGGL(plan_resolve_scan_kernel, dim3(1), dim3(1024), 0, st, n_cand, cnt, flags, capacity, rec_first, total);
  return hipGetLastError();
}

hipError_t launch_plan_resolve_emit(hipStream_t st, const PlanResolveIn &in, uint32_t *cnt, uint32_t *flags, const PlanResolveOut &out) {
  if (in.n_cand)
    hipLaunchKernelGGL(plan_resolve_emit_kernel, dim3((in.n_cand + kPwWaves - 1u) / kPwWaves), dim3(64 * kPwWaves), 0, st, in, cnt, flags,
                       out);
  return hipGetLastError();
}

hipError_t launch_plan_flag_cost(hipStream_t st, uint32_t n_cand, const uint32_t *flags, uint64_t *frac_bits) {
  if (n_cand) hipLaunchKernelGGL(plan_flag_cost_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, st, n_cand, flags, frac_bits);
  return hipGetLastError();
}

}  // namespace cabac
