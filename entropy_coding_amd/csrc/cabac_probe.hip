// Probe points (cabac_hip_probe.h): written bits inside a substream.
//
// getNumWrittenBits() (arith_codec.cpp:482-485) after a prefix of a bin string is the number of bits the coder has shifted out
// of `low` so far: every renormalisation shift of a context or terminate bin and the one shift of a bypass bin.  Where those bits
// are at that moment — stored, buffered behind a possible carry, among outstanding 0xFF bytes or still inside low — does not
// matter to the count (quad_enc_finish says the same of its probe: 8 * pos + 16 * nbuf + pend is "every shift so far"), and a
// carry moves no bit.  So the count needs the RANGE half of the encoder's chain only: no low, no carry, no flush check, no
// store.  The shifts of a bin depend on the range in front of it and on the context state it sees, so the walk is the encoder's:
// phase (a) of a 16-bin step resolves the states lane-parallel (quad_phase_fields, cabac_quad.h), then sixteen chain steps, the
// four rows of the wave together, each bin's fields delivered by a DPP row broadcast.
//
// Lane I of a row keeps the running count behind bin I (one select per bin), so after a step every lane holds the count behind
// its own record, and a probe "after the first k records" reads lane (k - 1) & 15 of the step that holds record k - 1.  The row
// carries the position of its next probe in a register: a step with no probe in it costs one compare (quad_probe_drain has the
// rest).  Layout and launch geometry are the estimator's: four substreams per wave, sixteen lanes each, the context store in LDS;
// four-wave workgroups from 1 024 waves up.  No atomics on global memory, no workgroup waits for another, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_kernels.h"
#include "cabac_quad.h"

namespace cabac {

namespace {

// One chain step for the four rows: quad_enc_step without low.  align() arrives as an LPS of width 256 that shifts nothing
// (quad_phase_fields), so there is no case for it.  A lane past the end of its row has all-zero fields: t = 0, no shift.
template <int I>
__device__ __forceinline__ void count_step(const QuadFields &f, uint32_t j, uint32_t &range, uint32_t &count, uint32_t &mine) {
  const uint32_t k = row_bcast<I>(f.k), c2 = row_bcast<I>(f.c2), lpsm = row_bcast<I>(f.lpsm), ep = row_bcast<I>(f.ep);
  const uint32_t t = (__umul24((range >> 5) & 15u, k) + c2) >> 1;  // LPS width: ((r>>5)*k>>1) + c
  const uint32_t rm = range - t;
  const uint32_t nl = (uint32_t)(__builtin_clz(t) - 23);           // getRenormBitsLPS; masked out when t == 0
  const uint32_t nm = (rm >> 8) ^ 1u;                              // rm < 512: 1 iff rm < 256
  const uint32_t nb = sel(lpsm, nl, nm);
  range = sel(lpsm, t, rm) << nb;
  count += nb + ep;
  mine = j == (uint32_t)I ? count : mine;
}

}  // namespace

template <int W>
__global__ __launch_bounds__(64 * W) void written_bits_kernel(uint32_t n_sub, const cabac_substream_desc *__restrict__ desc,
                                                              const uint16_t *__restrict__ records, ProbeList pl,
                                                              const uint32_t *__restrict__ start_state,
                                                              const uint8_t *__restrict__ start_rate,
                                                              const uint32_t *__restrict__ start_set, uint32_t *__restrict__ bits,
                                                              uint32_t *__restrict__ flags) {
  __shared__ uint32_t ctx_all[W * kQuadSubs * kQuadCtxStride];
  __shared__ uint32_t match_all[W][kMatchWords];
  __shared__ uint2 rates[512];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = lane >> 4, j = lane & 15u;
  for (uint32_t k = threadIdx.x; k < W * kMatchWords; k += 64u * W) (&match_all[0][0])[k] = 0u;
  quad_rate_tab_init(rates, threadIdx.x, 64u * W);
  const uint32_t sub = (blockIdx.x * W + wave) * kQuadSubs + row;
  CtxSets cs{};
  cs.n_sets = pl.n_sets;
  cs.state = start_state;
  cs.rate = start_rate;
  cs.start_set = start_set;
  const QuadSetUse su = quad_set_use(sub, sub < n_sub, cs);
  const bool live = sub < n_sub && !su.bad;  // rows beyond the batch and rows with a bad set walk nothing: their probes answer 0
  const cabac_substream_desc d = desc[live ? sub : 0];
  const uint32_t n = live ? d.n_records : 0u;
  const uint16_t *rec = records + d.rec_offset;
  uint32_t *rctx = ctx_all + (wave * kQuadSubs + row) * kQuadCtxStride;
  quad_ctx_load<true>(rctx, d.qp, d.init_id & 3u, j, 16u, su, cs);
  __syncthreads();

  uint32_t n_wave = n;
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 16));
  n_wave = max(n_wave, (uint32_t)__shfl_xor((int)n_wave, 32));
  const uint32_t max_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_wave);
  const uint16_t *rec_safe = n != 0 ? rec : reinterpret_cast<const uint16_t *>(desc);
  const uint32_t last_rec = n != 0 ? n - 1u : 0u;
  uint32_t next_rec = rec_safe[min(j, last_rec)];
  uint32_t bad = 0;
  uint32_t range = 510;  // start(), arith_codec.cpp:329-337
  uint32_t count = 0;    // row-uniform: the shifts so far
  uint32_t mine = 0;     // the count behind this lane's record of the step
  QuadProbeCursor pc = quad_probe_begin(pl, sub, sub < n_sub, n, lane);
  if (__ballot(pc.at == 0u) != 0) quad_probe_drain(pl, pc, n, 0u, 0u, lane, bits);  // in front of every record: 0
  for (uint32_t base = 0; base < max_n; base += 16) {
    const uint32_t r = next_rec;
    next_rec = rec_safe[min(base + 16u + j, last_rec)];
    const QuadFields f = quad_phase_fields<true>(r, base + j < n, lane, row, rctx, bad, match_all[wave], rates);
#define QSTEP(I) count_step<I>(f, j, range, count, mine)
    QSTEP(0); QSTEP(1); QSTEP(2); QSTEP(3); QSTEP(4); QSTEP(5); QSTEP(6); QSTEP(7);
    QSTEP(8); QSTEP(9); QSTEP(10); QSTEP(11); QSTEP(12); QSTEP(13); QSTEP(14); QSTEP(15);
#undef QSTEP
    if (__builtin_expect(__ballot(pc.at <= base + 16u) != 0, 0)) quad_probe_drain(pl, pc, n, base + 16u, mine, lane, bits);
  }
  const uint64_t bad_mask = __ballot(bad != 0);
  if (sub < n_sub && j == 0 && flags != nullptr)
    flags[sub] = su.bad ? 0x40u /* CABAC_RES_BAD_SET */ : (((bad_mask >> (row * 16u)) & 0xffffull) ? CABAC_RES_BAD_RECORD : 0u);
}

hipError_t launch_written_bits(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               const ProbeList &probes, const uint32_t *start_state, const uint8_t *start_rate,
                               const uint32_t *start_set, uint32_t *bits, uint32_t *flags) {
  if (n_sub == 0) return hipSuccess;
  const uint32_t waves = (n_sub + kQuadSubs - 1) / kQuadSubs;
  // four-wave workgroups pin one wave per SIMD (as launch_estimate); small batches spread single waves
  if (waves >= 1024u)
    hipLaunchKernelGGL(written_bits_kernel<4>, dim3((waves + 3) / 4), dim3(256), 0, st, n_sub, desc, records, probes, start_state,
                       start_rate, start_set, bits, flags);
  else
    hipLaunchKernelGGL(written_bits_kernel<1>, dim3(waves), dim3(64), 0, st, n_sub, desc, records, probes, start_state, start_rate,
                       start_set, bits, flags);
  return hipGetLastError();
}

}  // namespace cabac
