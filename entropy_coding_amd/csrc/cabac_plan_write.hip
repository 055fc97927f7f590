// The plan write (cabac_hip_write_plan.h): a plan of syntax elements, guards, computed entries and guarded blocks
// (cabac_hip_parse_plan.h) plus the values of the real elements and the blocks' coefficients -> the expanded substream of bin
// records the encode kernel codes.  What tests/parse_plan_model.py::fill / expand do on the CPU.
//
//   residual sizes pass (cabac_residual.hip)  ->  n_records and info word per block, whatever its guard will say
//   plan_resolve_kernel   per substream: the walk for its sizes — filled values (in LDS only), coded / skipped per block, bin
//                         count per element, running sums, expanded length, byte-slot size, the stop
//   splice_scan_kernel    across substreams (cabac_splice.hip); the host waits here once: sizes decide the buffers
//   plan_emit_kernel      the same walk again, now writing: descriptors, the elements' bins at their places by OUTPUT position,
//                         each coded block's destination, the filled values, the info words
//   residual records pass over a descriptor list in which skipped blocks are ones the binariser rejects (they write nothing)
//   encode kernel, plan_stops_kernel (a stopped substream codes nothing), assembly
// The rows form (cabac_hip_plan_rows.h) runs plan_emit_rows_kernel in place of plan_emit_kernel: the same walk, which also notes
// where in its expanded run each substream's hand-over entry lies; the WPP encode schedule takes that as its sync_at.
//
// The form in pieces (cabac_hip_plan_continue.h) runs plan_resolve_pieces_kernel and plan_emit_pieces_kernel: the same walk over one
// piece of every substream's plan.  Its first walk also loads and checks the substream's coder state (cabac_quad.h), its second one
// writes the encode descriptor with the CALLER'S slot; the encoder in pieces codes the expanded records into that slot, and
// plan_stops_pieces_kernel gives a stopped piece its result and its flag.  No scan of byte sizes, no assembly.
//
// The walk itself is cabac_plan_walk.h's, one wave per substream; this file says where a substream's plan lies and where its
// results go (one atomicOr reports a substream that outgrows 32 bits).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_hip_parse_elements.h"
#include "cabac_hip_parse_plan.h"
#include "cabac_kernels.h"
#include "cabac_plan_walk.h"
#include "cabac_quad.h"

namespace cabac {

namespace {

__device__ __forceinline__ uint64_t pw_slot_bytes(uint64_t n_records) { return ((7u * n_records + 7u) / 8u + 8u + 15u) / 16u * 16u; }

struct PwOut {  // what the second walk writes
  const uint32_t *sub_n, *sub_cap, *sub_flag;
  const uint64_t *rec_base, *byte_base;
  cabac_substream_desc *desc_out;
  cabac_tu_desc *tus_out;
  uint64_t *tu_offset;
  uint16_t *records;
  uint32_t *values_out, *tu_info_out;
};

// the plan write as cabac_plan_walk.h sees it: a unit is a substream, its run is the expanded substream (blocks included)
struct PwIo {
  static constexpr bool kBlocksInRun = true;
  uint32_t n_units;
  const cabac_substream_desc *desc;
  const uint32_t *plan, *values, *tile_first;
  const cabac_tu_desc *tus;
  const uint32_t *tu_at, *tu_guard, *tu_n_records, *tu_info;
  uint32_t *sub_n, *sub_cap, *sub_flag, *err;  // first walk
  PwOut out;                                   // second walk
  uint16_t *records;

  __device__ __forceinline__ PlanWalkUnit unit(uint32_t sub) const {
    const cabac_substream_desc dsc = desc[sub];
    PlanWalkUnit u;
    u.plan = reinterpret_cast<const uint2 *>(plan) + dsc.rec_offset;
    u.vin = values + dsc.rec_offset;
    u.vout = out.values_out ? out.values_out + dsc.rec_offset : nullptr;
    u.n = dsc.n_records;
    u.t0 = tile_first[sub];
    u.t1 = tile_first[sub + 1];
    return u;
  }
  __device__ __forceinline__ bool emit_begin(uint32_t sub, const PlanWalkUnit &u, uint32_t lane, uint64_t &base) const {
    base = out.rec_base[sub];
    if (lane == 0u) {
      cabac_substream_desc o = desc[sub];
      o.rec_offset = base;
      o.byte_offset = out.byte_base[sub];
      o.n_records = out.sub_n[sub];
      o.byte_capacity = out.sub_cap[sub];
      out.desc_out[sub] = o;
    }
    if (out.sub_flag[sub] == 0u) return true;
    cabac_tu_desc rejected{};  // a stopped substream: none of its blocks is coded, nothing else of it is written
    rejected.log2_width = rejected.log2_height = 7;
    for (uint32_t t = u.t0 + lane; t < u.t1; t += 64u) {
      out.tus_out[t] = rejected;
      out.tu_offset[t] = base;
    }
    return false;
  }
  __device__ __forceinline__ void emit_block(uint32_t t, bool coded, uint64_t base, uint64_t off, uint32_t excl, uint32_t info) const {
    cabac_tu_desc rejected{};  // what the records pass gets for a block that writes nothing
    rejected.log2_width = rejected.log2_height = 7;
    out.tus_out[t] = coded ? tus[t] : rejected;
    out.tu_offset[t] = base + off + excl;
    if (out.tu_info_out) out.tu_info_out[t] = info;
  }
  __device__ __forceinline__ void count_end(uint32_t sub, bool bad_rec, bool bad_val, uint64_t off) const {
    const uint32_t flag = bad_rec ? CABAC_RES_BAD_RECORD : bad_val ? CABAC_RES_BAD_VALUE : 0u;
    const uint64_t expanded = flag ? 0u : off;
    if (expanded > 0xfffffff0ull || pw_slot_bytes(expanded) > 0xfffffff0ull) atomicOr(err, 1u);
    sub_flag[sub] = flag;
    sub_n[sub] = (uint32_t)expanded;
    sub_cap[sub] = (uint32_t)pw_slot_bytes(expanded);
  }
};

// the rows form (cabac_hip_plan_rows.h): the same unit, and the record index of its hand-over entry
struct PwRowsIo : PwIo {
  const uint32_t *sync_entry;  // per substream: the hand-over entry of its plan
  uint32_t *sync_rec;          // per substream: the records of its expanded run in front of that entry
  __device__ __forceinline__ uint32_t sync_at(uint32_t sub) const { return sync_entry[sub]; }
  __device__ __forceinline__ void emit_sync(uint32_t sub, uint64_t off) const { sync_rec[sub] = (uint32_t)off; }
};

// the form in pieces (cabac_hip_plan_continue.h): the same unit, coded into the caller's slot from a coder state.  sub_flag says
// what becomes of the piece: 0 it is walked and coded; CABAC_RES_BAD_RECORD / CABAC_RES_BAD_VALUE its walk stops; kPcPass its
// state is refused or comes with flags, so that the encoder in pieces answers for it and nothing else of it is written.
constexpr uint32_t kPcPass = 0x80000000u;

struct PcIo : PwIo {
  CtxPieces cp;
  __device__ __forceinline__ void count_end(uint32_t sub, bool bad_rec, bool bad_val, uint64_t off) const {
    // the state is data from memory: checked here, where it is loaded, before the second walk writes anything.  (A bad set index
    // is the encoder's to report: the walk writes what the one-call form writes for such a substream.)
    const QuadPieceUse pu = quad_piece_use<true>(sub, true, false, desc[sub].byte_capacity, cp);
    const uint32_t flag = !pu.code ? kPcPass : bad_rec ? CABAC_RES_BAD_RECORD : bad_val ? CABAC_RES_BAD_VALUE : 0u;
    const uint64_t expanded = flag ? 0u : off;
    if (expanded > 0xfffffff0ull) atomicOr(err, 1u);
    sub_flag[sub] = flag;
    sub_n[sub] = (uint32_t)expanded;
    sub_cap[sub] = 0u;  // (the slot is the caller's)
  }
  __device__ __forceinline__ bool emit_begin(uint32_t sub, const PlanWalkUnit &u, uint32_t lane, uint64_t &base) const {
    base = out.rec_base[sub];
    const uint32_t flag = out.sub_flag[sub];
    if (lane == 0u) {
      cabac_substream_desc o = desc[sub];  // byte_offset, byte_capacity, qp and init_id are the caller's
      o.rec_offset = base;
      o.n_records = out.sub_n[sub];
      if (flag != 0u) o.init_id &= ~(uint32_t)CABAC_SUB_FINISH;  // a stopped piece is not finished: it passes its state through
      out.desc_out[sub] = o;
    }
    if (flag == 0u) return true;
    cabac_tu_desc rejected{};  // none of its blocks is coded, nothing else of it is written
    rejected.log2_width = rejected.log2_height = 7;
    for (uint32_t t = u.t0 + lane; t < u.t1; t += 64u) {
      out.tus_out[t] = rejected;
      out.tu_offset[t] = base;
    }
    return false;
  }
};

__device__ __forceinline__ PwIo pw_io(uint32_t n_sub, const PlanWriteIn &in, uint32_t *sub_n, uint32_t *sub_cap, uint32_t *sub_flag,
                                      uint32_t *err, const PwOut &out) {
  return PwIo{n_sub, in.desc, in.plan, in.values, in.tile_first, in.tus, in.tu_at, in.tu_guard, in.tu_n_records, in.tu_info,
              sub_n, sub_cap, sub_flag, err, out, out.records};
}

}  // namespace

__global__ __launch_bounds__(64 * kPwWaves) void plan_resolve_kernel(uint32_t n_sub, PlanWriteIn in, uint32_t *__restrict__ sub_n,
                                                                      uint32_t *__restrict__ sub_cap, uint32_t *__restrict__ sub_flag,
                                                                      uint32_t *__restrict__ err) {
  plan_walk<false>(pw_io(n_sub, in, sub_n, sub_cap, sub_flag, err, PwOut{}));
}

__global__ __launch_bounds__(64 * kPwWaves) void plan_emit_kernel(uint32_t n_sub, PlanWriteIn in, PwOut out) {
  plan_walk<true>(pw_io(n_sub, in, nullptr, nullptr, nullptr, nullptr, out));
}

__global__ __launch_bounds__(64 * kPwWaves) void plan_emit_rows_kernel(uint32_t n_sub, PlanWriteIn in, PwOut out,
                                                                        const uint32_t *__restrict__ sync_entry,
                                                                        uint32_t *__restrict__ sync_rec) {
  plan_walk<true, true>(PwRowsIo{pw_io(n_sub, in, nullptr, nullptr, nullptr, nullptr, out), sync_entry, sync_rec});
}

__global__ __launch_bounds__(64 * kPwWaves) void plan_resolve_pieces_kernel(uint32_t n_sub, PlanWriteIn in, CtxPieces cp,
                                                                             uint32_t *__restrict__ sub_n, uint32_t *__restrict__ sub_cap,
                                                                             uint32_t *__restrict__ sub_flag, uint32_t *__restrict__ err) {
  plan_walk<false>(PcIo{pw_io(n_sub, in, sub_n, sub_cap, sub_flag, err, PwOut{}), cp});
}

__global__ __launch_bounds__(64 * kPwWaves) void plan_emit_pieces_kernel(uint32_t n_sub, PlanWriteIn in, PwOut out) {
  plan_walk<true>(PcIo{pw_io(n_sub, in, nullptr, nullptr, nullptr, nullptr, out), CtxPieces{}});
}

// the stops of the form in pieces, behind the encoder: a stopped piece has passed its state through (a fresh one as the state of
// start()); it returns {0, flag} and the flag is added to the state.  A piece that was passed to the encoder has its answer.
__global__ __launch_bounds__(256) void plan_stops_pieces_kernel(uint32_t n_sub, const uint32_t *__restrict__ sub_flag,
                                                                cabac_substream_result *__restrict__ results,
                                                                cabac_coder_state *__restrict__ coder_out) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_sub) return;
  const uint32_t flag = sub_flag[s];
  if (flag == 0u || flag == kPcPass) return;
  cabac_substream_result r;
  r.n_bits = 0u;
  r.flags = flag;
  results[s] = r;
  if (coder_out != nullptr) coder_out[s].flags |= flag;
}

// the out sets of a plan write from sets: a stopped substream writes none
__global__ __launch_bounds__(256) void plan_out_sets_kernel(uint32_t n_sub, const uint32_t *__restrict__ sub_flag,
                                                            const uint32_t *__restrict__ out_set, uint32_t *__restrict__ out_set_live) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < n_sub) out_set_live[s] = sub_flag[s] != 0u ? 0xffffffffu : out_set[s];
}

__global__ __launch_bounds__(256) void plan_stops_kernel(uint32_t n_sub, const uint32_t *__restrict__ sub_flag,
                                                         cabac_substream_result *__restrict__ results) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_sub) return;
  const uint32_t flag = sub_flag[s];
  if (flag != 0u) {
    cabac_substream_result r;
    r.n_bits = 0u;
    r.flags = flag;
    results[s] = r;
  }
}

hipError_t launch_plan_resolve(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, uint32_t *sub_n, uint32_t *sub_cap,
                               uint32_t *sub_flag, uint32_t *err) {
  hipError_t e = hipMemsetAsync(err, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if (n_sub)
    hipLaunchKernelGGL(plan_resolve_kernel, dim3((n_sub + kPwWaves - 1u) / kPwWaves), dim3(64 * kPwWaves), 0, st, n_sub, in, sub_n, sub_cap,
                       sub_flag, err);
  return hipGetLastError();
}

hipError_t launch_plan_emit(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const uint32_t *sub_n, const uint32_t *sub_cap,
                            const uint32_t *sub_flag, const uint64_t *rec_base, const uint64_t *byte_base,
                            cabac_substream_desc *desc_out, cabac_tu_desc *tus_out, uint64_t *tu_offset, uint16_t *records,
                            uint32_t *values_out, uint32_t *tu_info_out, const uint32_t *sync_entry, uint32_t *sync_rec) {
  const PwOut out{sub_n, sub_cap, sub_flag, rec_base, byte_base, desc_out, tus_out, tu_offset, records, values_out, tu_info_out};
  const dim3 grid((n_sub + kPwWaves - 1u) / kPwWaves), block(64 * kPwWaves);
  if (n_sub && sync_entry) hipLaunchKernelGGL(plan_emit_rows_kernel, grid, block, 0, st, n_sub, in, out, sync_entry, sync_rec);
  else if (n_sub) hipLaunchKernelGGL(plan_emit_kernel, grid, block, 0, st, n_sub, in, out);
  return hipGetLastError();
}

hipError_t launch_plan_resolve_pieces(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const CtxPieces &cp, uint32_t *sub_n,
                                      uint32_t *sub_cap, uint32_t *sub_flag, uint32_t *err) {
  hipError_t e = hipMemsetAsync(err, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(plan_resolve_pieces_kernel, dim3((n_sub + kPwWaves - 1u) / kPwWaves), dim3(64 * kPwWaves), 0, st, n_sub, in, cp, sub_n,
                     sub_cap, sub_flag, err);
  return hipGetLastError();
}

hipError_t launch_plan_emit_pieces(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const uint32_t *sub_n, const uint32_t *sub_flag,
                                   const uint64_t *rec_base, cabac_substream_desc *desc_out, cabac_tu_desc *tus_out, uint64_t *tu_offset,
                                   uint16_t *records, uint32_t *values_out, uint32_t *tu_info_out) {
  const PwOut out{sub_n, nullptr, sub_flag, rec_base, nullptr, desc_out, tus_out, tu_offset, records, values_out, tu_info_out};
  hipLaunchKernelGGL(plan_emit_pieces_kernel, dim3((n_sub + kPwWaves - 1u) / kPwWaves), dim3(64 * kPwWaves), 0, st, n_sub, in, out);
  return hipGetLastError();
}

hipError_t launch_plan_stops_pieces(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, cabac_substream_result *results,
                                    cabac_coder_state *coder_out) {
  hipLaunchKernelGGL(plan_stops_pieces_kernel, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, n_sub, sub_flag, results, coder_out);
  return hipGetLastError();
}

hipError_t launch_plan_out_sets(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, const uint32_t *out_set, uint32_t *out_set_live) {
  if (n_sub) hipLaunchKernelGGL(plan_out_sets_kernel, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, n_sub, sub_flag, out_set, out_set_live);
  return hipGetLastError();
}

hipError_t launch_plan_stops(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, cabac_substream_result *results) {
  if (n_sub) hipLaunchKernelGGL(plan_stops_kernel, dim3((n_sub + 255u) / 256u), dim3(256), 0, st, n_sub, sub_flag, results);
  return hipGetLastError();
}

}  // namespace cabac
