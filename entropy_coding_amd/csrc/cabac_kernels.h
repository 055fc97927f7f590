// Internal launch interface between the kernels (cabac_kernels.hip) and the C ABI (cabac_capi.cpp).
#ifndef CABAC_KERNELS_H
#define CABAC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_hip_pieces.h"
#include "cabac_hip_workspace.h"

struct cabac_search_log_counters;  // cabac_hip_search_emit.h
struct cabac_search_log_entry;

namespace cabac {

struct WsState;  // the fixed workspace, below
struct WsGate;

// Context sets of the codec calls (cabac_hip_ctx_sets.h): substream s starts from set start_set[s] of state / rate and writes the
// contexts it leaves as set out_set[s] of out_state / out_rate (0xffffffff: Ctx::init / nothing; start_set / out_set null: all
// of them so).  An index >= n_sets codes nothing.  The out arrays may be the start arrays.
struct CtxSets {
  uint32_t n_sets;
  const uint32_t *state;
  const uint8_t *rate;
  const uint32_t *start_set;
  const uint32_t *out_set;
  uint32_t *out_state;
  uint8_t *out_rate;
};

// The sets and the coder states of the pieces calls (cabac_hip_pieces.h): everything a kernel does with sets it does with the base,
// everything about the coder state is in the overloads that take this type (cabac_quad.h).  coder_in null: all fresh; coder_out
// null: no state written; they may be the same array.
struct CtxPieces : CtxSets {
  const cabac_coder_state *coder_in;
  cabac_coder_state *coder_out;
};

hipError_t launch_ctx_init(hipStream_t st, uint32_t n_sub, const int32_t *qp, const uint32_t *init_id, uint32_t *state,
                           uint8_t *rate);
// in_flight: the number of substreams on the device at the same time when this launch is one chunk of a batch whose
// chunks run concurrently on several streams (0 = this launch is alone); the workgroup geometry follows the whole batch
hipError_t launch_encode(hipStream_t st, int variant, uint32_t n_sub, const cabac_substream_desc *desc,
                         const uint16_t *records, uint8_t *bytes, cabac_substream_result *results, uint32_t in_flight = 0,
                         const CtxSets *sets = nullptr);
hipError_t launch_decode(hipStream_t st, int variant, uint32_t n_sub, const cabac_substream_desc *desc,
                         const uint16_t *records, const uint8_t *bytes, uint8_t *bins,
                         cabac_substream_result *results, uint32_t in_flight = 0, uint32_t *select = nullptr,
                         const CtxSets *sets = nullptr);

// v4 "quad" kernels (cabac_kernels_v4.hip): four substreams per wave
hipError_t launch_encode_v4(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, const CtxSets *sets = nullptr);
hipError_t launch_encode_v6(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, uint32_t in_flight = 0, const CtxSets *sets = nullptr);
hipError_t launch_encode_v7(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint8_t *bytes, cabac_substream_result *results, uint32_t in_flight = 0, const CtxSets *sets = nullptr);
// lanes_per_sub: 16 = the quad decoder (four substreams per wave), 4 = sixteen substreams per wave, 0 = by the batch: from
// 9 216 substreams in flight the choice is made on the device (select: one device word of the caller's, not shared with
// another launch in flight; null = the quad decoder)
hipError_t launch_decode_v4(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            const uint8_t *bytes, uint8_t *bins, cabac_substream_result *results, uint32_t in_flight = 0,
                            int lanes_per_sub = 16, uint32_t *select = nullptr, const CtxSets *sets = nullptr);

// the bin codec in pieces (cabac_hip_pieces.h): not dispatched.  The decoder has one geometry; the encoder the caller's choice
// (cabac_hip_piece_encoder.h), variant 4: one wave per four substreams, 7: the lane-serial encoder, sixteen substreams per
// workgroup from 1 024 substreams and four below — everything they write is the same
hipError_t launch_encode_pieces(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                uint8_t *bytes, cabac_substream_result *results, const CtxPieces &pieces, int variant);
hipError_t launch_decode_pieces(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                const uint8_t *bytes, uint8_t *bins, cabac_substream_result *results, const CtxPieces &pieces);

// bit estimator (cabac_kernels_v4.hip)
hipError_t launch_estimate(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                           uint64_t *frac_bits, uint32_t *flags, const uint32_t *start_state = nullptr,
                           const uint8_t *start_rate = nullptr, const uint32_t *start_set = nullptr);

// probe points (cabac_hip_probe.h): running totals at caller-chosen positions inside the substreams.  The probe list: substream
// s owns at[first[s] .. first[s + 1]), each "after the first k records", non-decreasing, clipped to the substream's length; n_sets:
// the sets state / rate hold (substream s starts from set start_set[s]; 0xffffffff or start_set null: Ctx::init; an index >=
// n_sets: CABAC_RES_BAD_SET, its values 0).  flags (may be null): 0, CABAC_RES_BAD_RECORD or CABAC_RES_BAD_SET per substream
struct ProbeList {
  const uint32_t *first, *at;
  uint32_t n_sets;
};
// written bits (cabac_probe.hip): bits[p] = getNumWrittenBits() after the probe's records — the range half of the encoder's chain
hipError_t launch_written_bits(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               const ProbeList &probes, const uint32_t *start_state, const uint8_t *start_rate,
                               const uint32_t *start_set, uint32_t *bits, uint32_t *flags);
// estimated bits (cabac_kernels_v4.hip): the probe instantiation of the estimator's walk, frac_bits[p] per probe
hipError_t launch_estimate_probes(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                  const ProbeList &probes, const uint32_t *start_state, const uint8_t *start_rate,
                                  const uint32_t *start_set, uint64_t *frac_bits, uint32_t *flags);
// the probes of a spliced call (cabac_splice.hip) as positions in the expanded strings: probe_rec[p] = k + pre[m], as
// launch_splice_sync_index, for the pair (probe_at[p], probe_splice[p]) of the substream that owns probe p (probe_splice null: the
// upper end).  One thread per probe.  After launch_splice_plan accepted the list.
hipError_t launch_splice_probe_index(hipStream_t st, uint32_t n_sub, uint32_t n_probe, const cabac_substream_desc *desc,
                                     const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                     const uint32_t *probe_first, const uint32_t *probe_at, const uint32_t *probe_splice,
                                     uint32_t *probe_rec);

// context advance (cabac_kernels_v4.hip; cabac_hip_ctx_sets.h): update() for every context-coded record of the runs, sets in, sets
// out; nothing is coded.  flags (may be null): CABAC_RES_BAD_RECORD, CABAC_RES_BAD_SET or 0 per substream
hipError_t launch_ctx_advance(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                              const CtxSets &sets, uint32_t *flags);
// one level of a WPP call, substreams [first, first + n): desc_out[s] = desc[s] with n_records = min(sync_at[s], n_records) and
// the flag bits of init_id cleared; slot_out[s] = s; start_out[s] = sync_from[s] if it is 0xffffffff or below `first`, else an
// index that every sets call answers with CABAC_RES_BAD_SET
hipError_t launch_wpp_level(hipStream_t st, uint32_t first, uint32_t n, const cabac_substream_desc *desc, const uint32_t *sync_from,
                            const uint32_t *sync_at, cabac_substream_desc *desc_out, uint32_t *start_out, uint32_t *slot_out);

// device binariser (cabac_binarize.hip)
hipError_t launch_binarize(hipStream_t st, uint32_t n_sub, const uint64_t *se_offset, const uint32_t *se,
                           const uint64_t *rec_offset, uint32_t *n_records, uint16_t *records);

// residual binariser (cabac_residual.hip)
// scratch: residual_scratch_bytes(n_tu) bytes of device memory the launch may overwrite (block ordering)
size_t residual_scratch_bytes(uint32_t n_tu);
// order_ready: `scratch` still holds the block order of an earlier launch over the SAME tus[] (the sizes pass of this call)
// coeff_bytes: 4 (int32_t, the reference's TCoeff) or 2 (int16_t: blocks of 15-bit dynamic range)
hipError_t launch_residual(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                           const uint64_t *rec_offset, uint32_t *n_records, uint32_t *info, uint16_t *records,
                           void *scratch, bool order_ready = false);

// fused residual estimator (cabac_residual_estimate.hip): candidate c = blocks [cand_first[c], cand_first[c+1]) costed in order from
// context set start_set[c]; scratch: residual_estimate_scratch_bytes(n_cand) bytes the launch may overwrite (candidate ordering)
size_t residual_estimate_scratch_bytes(uint32_t n_cand);
hipError_t launch_residual_estimate(hipStream_t st, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                    const void *coeff, int coeff_bytes /* 4 or 2 */, const uint32_t *start_state,
                                    const uint8_t *start_rate, const uint32_t *start_set, uint64_t *frac_bits,
                                    uint64_t *tu_frac_bits, uint32_t *tu_info, void *scratch);

// the exporting variant (cabac_hip_search.h): walks the n_item candidates index[0 .. n_item) (index null: n_item == n_cand, every
// candidate; an entry >= n_cand is skipped) and writes the contexts item i leaves as set out_set[i] (0xffffffff: none) of
// out_state / out_rate, which may be the start arrays; frac_bits may be null here.  scratch: residual_estimate_scratch_bytes(n_item)
hipError_t launch_residual_estimate_export(hipStream_t st, uint32_t n_item, const uint32_t *index, uint32_t n_cand,
                                           const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                           const uint32_t *start_state, const uint8_t *start_rate, const uint32_t *start_set,
                                           const uint32_t *out_set, uint32_t *out_state, uint8_t *out_rate, uint64_t *frac_bits,
                                           uint64_t *tu_frac_bits, uint32_t *tu_info, void *scratch);

// the variant with side records (cabac_hip_search_unit.h): the exporting walk over candidates that are record strings with blocks
// spliced in — candidate c owns records[rec_first[c] .. rec_first[c+1]) and block t goes in front of index tu_at[t] of its
// candidate's run (tu_at null: behind the run).  out_set null: no set is written; flags (may be null): CABAC_RES_BAD_RECORD or 0
// per candidate.  scratch: residual_estimate_scratch_bytes(n_item)
hipError_t launch_unit_estimate(hipStream_t st, uint32_t n_item, const uint32_t *index, uint32_t n_cand, const uint32_t *cand_first,
                                const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, const uint32_t *start_state,
                                const uint8_t *start_rate, const uint32_t *start_set, const uint64_t *rec_first,
                                const uint16_t *records, const uint32_t *tu_at, const uint32_t *out_set, uint32_t *out_state,
                                uint8_t *out_rate, uint64_t *frac_bits, uint64_t *tu_frac_bits, uint32_t *tu_info, uint32_t *flags,
                                void *scratch);

// search rounds (cabac_search.hip): per group g = candidates [group_first[g], group_first[g+1]) (clipped to
// min(group_first[n_group], n_cand_max)) the index and the value of the smallest dist + ((lambda_q16 * frac_bits) >> 31)
hipError_t launch_search_select(hipStream_t st, uint32_t n_group, uint32_t n_cand_max, const uint32_t *group_first,
                                const uint64_t *frac_bits, const uint64_t *dist /* may be null */, uint64_t lambda_q16, uint32_t *pick,
                                uint64_t *cost);

// the winner log (cabac_search_emit.hip; cabac_hip_search_emit.h): the device arrays of one log and what they hold at most
struct SearchLogArrays {
  cabac_search_log_counters *counters;
  cabac_search_log_entry *entries;
  uint16_t *records;
  cabac_tu_desc *tu;
  uint32_t *tu_at;
  void *coeff;
  uint32_t *chain_rec, *chain_tu;  // per chain: the records / blocks of its entries so far
  uint32_t *mark_rec, *mark_tu;    // per chain: its hand-over point (cabac_hip_splice_rows.h), 0xffffffff = the end of the chain
  uint64_t record_cap, coeff_cap;
  uint32_t n_chain, entry_cap, tu_cap;
};
// the scratch of one append, carved out of one allocation that depends on n_group only: per group what the sizes pass found
// (chain 0xffffffff: the group appends nothing) and where the scan put it; hdr = {the call fits, the log's coefficient cursor in
// front of the call, the call's coefficients}
struct SearchLogScratch {
  uint64_t *hdr, *rec_src, *n_coeff, *rec_dst, *co_dst /* n_group + 1, relative to the call */;
  uint32_t *chain, *n_rec, *n_tu, *tu_src, *tu_dst, *entry;
  size_t bytes;
};
inline SearchLogScratch search_log_scratch(void *p, uint32_t n_group) {
  SearchLogScratch s;
  const size_t n = n_group;
  s.hdr = static_cast<uint64_t *>(p);
  s.rec_src = s.hdr + 4;
  s.n_coeff = s.rec_src + n;
  s.rec_dst = s.n_coeff + n;
  s.co_dst = s.rec_dst + n;
  s.chain = reinterpret_cast<uint32_t *>(s.co_dst + n + 1);
  s.n_rec = s.chain + n;
  s.n_tu = s.n_rec + n;
  s.tu_src = s.n_tu + n;
  s.tu_dst = s.tu_src + n;
  s.entry = s.tu_dst + n;
  s.bytes = (4 + 4 * n + 1) * sizeof(uint64_t) + 6 * n * sizeof(uint32_t);
  return s;
}
size_t search_log_scratch_bytes(uint32_t n_group);
hipError_t launch_search_log_reset(hipStream_t st, const SearchLogArrays &log);
// the hand-over points of the n listed chains (cabac_hip_splice_rows.h): mark_rec / mark_tu = the chains' cursors as they stand
hipError_t launch_search_log_mark(hipStream_t st, const SearchLogArrays &log, uint32_t n, const uint32_t *chain);
// the three launches of an append: sizes, scan (capacity, entries, cursors), copy; scratch: search_log_scratch_bytes(n_group)
hipError_t launch_search_log_append(hipStream_t st, const SearchLogArrays &log, uint32_t n_group, const uint32_t *pick,
                                    const uint32_t *group_chain, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                    const void *coeff, int coeff_bytes, const uint64_t *rec_first, const uint16_t *records,
                                    const uint32_t *tu_at, void *scratch);
// the chains' entries laid out for launch_splice_plan: desc_out / splice_first (n_chain, n_chain + 1), records (n_record), splices
// (n_tu); n_entry, n_record, n_tu: the log's counters as the host read them
hipError_t launch_search_log_place(hipStream_t st, const SearchLogArrays &log, const cabac_substream_desc *desc, uint32_t n_entry,
                                   uint64_t n_record, uint32_t n_tu, cabac_substream_desc *desc_out, uint32_t *splice_first,
                                   uint16_t *records, cabac_splice *splices);

// residual parser family (cabac_residual_parse.hip): bytes -> coefficient blocks, one substream = blocks [tile_first[s],
// tile_first[s+1]).  What the walks read and write; members a walk does not read are null.  The first eight are every walk's.
struct ParseIn {
  const cabac_substream_desc *desc;
  const uint8_t *bytes;
  const uint32_t *tile_first;
  const cabac_tu_desc *tus;
  void *coeff;
  int coeff_bytes;    // 4 or 2
  uint32_t *tu_info;  // may be null: per block scanPosLast | CABAC_TU_INFO_*
  cabac_substream_result *results;
  const uint32_t *tu_at;     // block t goes in front of index tu_at[t] of its substream's run (null: behind the run)
  const uint32_t *tu_guard;  // may be null: one guard word per block
  const uint32_t *plan;      // 2 words per entry: the binariser's word0, a guard word
  uint32_t *values;          // values[rec_offset + i] receives the value of entry i
  const uint16_t *records;   // the side records of the unit walk ...
  uint8_t *side_bins;        // ... and side_bins[rec_offset + i] the bin of side record i
};
// kResidual: blocks alone.  kUnit (cabac_hip_parse_unit.h): substream s = the side records records[desc[s].rec_offset .. +
// n_records) with the blocks spliced in, all on one context store.  kElement (cabac_hip_parse_elements.h): the run is a plan of
// syntax elements.  kPlan (cabac_hip_parse_plan.h): the element walk with the two computed entry kinds, on the same operands.
enum class ParseWalk { kResidual, kUnit, kElement, kPlan };
hipError_t launch_parse(hipStream_t st, ParseWalk walk, uint32_t n_sub, const ParseIn &in);
// the plan walk from and into context sets (cabac_hip_plan_rows.h): substream s hands its contexts over when the walk arrives at
// entry out_at[s] (out_at null: behind the substream).  A start index at or above start_bound is a bad one.  slot_base
// 0xffffffff: the out sets are sets.out_set's; otherwise substream s writes set slot_base + s and sets.out_set is not read
hipError_t launch_plan_parse_sets(hipStream_t st, uint32_t n_sub, const ParseIn &in, const CtxSets &sets, const uint32_t *out_at,
                                  uint32_t start_bound, uint32_t slot_base);
// the plan walk in pieces (cabac_hip_plan_resume.h): the sets form (out set behind the piece) from and into a coder state per substream
hipError_t launch_plan_parse_pieces(hipStream_t st, uint32_t n_sub, const ParseIn &in, const CtxPieces &pieces);

// residual records spliced into host-recorded substreams (cabac_splice.hip); array sizes: pre n_splice + n_sub + 1,
// sub_n / sub_cap / rec_base / byte_base n_sub, seen n_tu, err 1, totals 3 ({records, bytes, error})
hipError_t launch_splice_plan(hipStream_t st, uint32_t n_sub, uint32_t n_tu, const cabac_substream_desc *desc,
                              const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_splice,
                              const uint32_t *tu_n_records, uint32_t *pre, uint32_t *sub_n, uint32_t *sub_cap, uint32_t *seen, uint32_t *err,
                              uint64_t *rec_base, uint64_t *byte_base, uint64_t *totals, const uint64_t *n_dev = nullptr,
                              const WsGate *gate = nullptr);
// n_dev (null: n_tu and n_splice as given): a device word that holds the number of blocks and splices that count — the log's emit
// on a fixed workspace, whose arrays are sized by the log's capacities; n_tu and n_splice then only bound the arrays
hipError_t launch_splice_expand(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *host_records,
                                const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                const uint32_t *sub_n, const uint32_t *sub_cap, const uint64_t *rec_base, const uint64_t *byte_base,
                                cabac_substream_desc *desc_out, uint64_t *tu_offset, uint16_t *records);
// the hand-over points of spliced substreams (cabac_hip_splice_rows.h) as indices into their expanded strings: sync_rec[s] =
// k + pre[m] with k = min(sync_at[s], n_records) host records and m = sync_splice[s] splices in front, clipped to
// [#{at < k}, #{at <= k}] (sync_splice null: the upper end).  After launch_splice_plan accepted the list.
hipError_t launch_splice_sync_index(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *splice_first,
                                    const cabac_splice *splices, const uint32_t *pre, const uint32_t *sync_at,
                                    const uint32_t *sync_splice, uint32_t *sync_rec);
hipError_t launch_tu_range_check(hipStream_t st, uint32_t n_tu, const cabac_tu_desc *tus, uint64_t n_coeff_total, uint32_t *err);
hipError_t launch_tu_info_any(hipStream_t st, uint32_t n_tu, const uint32_t *info, uint32_t *flag);
hipError_t launch_bin_count(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                            uint32_t *counts);

// the scan of launch_splice_plan alone: rec_base / byte_base (n_sub each) from sub_n / sub_cap, totals = {records, bytes, *err != 0}
hipError_t launch_splice_scan(hipStream_t st, uint32_t n_sub, uint32_t *sub_n, uint32_t *sub_cap, uint64_t *rec_base,
                              uint64_t *byte_base, const uint32_t *err, uint64_t *totals, const WsGate *gate = nullptr);

// the plan writer (cabac_plan_write.hip; cabac_hip_write_plan.h): the plan walk on the writer's side, once for the sizes and once
// for the records.  What both walks read: the plan and the real values, the blocks with the sizes and info words of the residual
// binariser's sizes pass.
struct PlanWriteIn {
  const cabac_substream_desc *desc;
  const uint32_t *plan, *values, *tile_first;
  const cabac_tu_desc *tus;
  const uint32_t *tu_at, *tu_guard;         // may be null
  const uint32_t *tu_n_records, *tu_info;   // of launch_residual's sizes pass over tus[]
};
// per substream the expanded length, the byte-slot size and the stop (0, CABAC_RES_BAD_RECORD or CABAC_RES_BAD_VALUE; a stopped
// substream has length 0); *err is set when a substream outgrows 32 bits
hipError_t launch_plan_resolve(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, uint32_t *sub_n, uint32_t *sub_cap,
                               uint32_t *sub_flag, uint32_t *err);
// the second walk: the expanded descriptors, the elements' bin records at their places, per block its destination and its
// descriptor where it is coded (tus_out[t] is one the binariser rejects where it is skipped or its substream stopped), the filled
// values (values_out may be null and may be in.values) and the info words (tu_info_out may be null)
hipError_t launch_plan_emit(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const uint32_t *sub_n, const uint32_t *sub_cap,
                            const uint32_t *sub_flag, const uint64_t *rec_base, const uint64_t *byte_base,
                            cabac_substream_desc *desc_out, cabac_tu_desc *tus_out, uint64_t *tu_offset, uint16_t *records,
                            uint32_t *values_out, uint32_t *tu_info_out, const uint32_t *sync_entry = nullptr,
                            uint32_t *sync_rec = nullptr);
// sync_entry (the rows form; null: the plain walk): per substream the hand-over entry of its plan; sync_rec[s] then receives the
// records of its expanded run in front of that entry
// out_set_live[s] = out_set[s], or 0xffffffff for a stopped substream
hipError_t launch_plan_out_sets(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, const uint32_t *out_set, uint32_t *out_set_live);
// a stopped substream codes nothing: results[s] = {0, sub_flag[s]} where sub_flag[s] != 0
hipError_t launch_plan_stops(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, cabac_substream_result *results);
// the plan write in pieces (cabac_hip_plan_continue.h), n_sub > 0: the two walks over one piece of every substream's plan — the first
// also checks the coder states of `cp` (sub_flag: 0, the stop, or 0x80000000 for a state that is refused or comes with flags), the
// second writes the encode descriptors with the caller's slots — and the stops behind launch_encode_pieces
hipError_t launch_plan_resolve_pieces(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const CtxPieces &cp, uint32_t *sub_n,
                                      uint32_t *sub_cap, uint32_t *sub_flag, uint32_t *err);
hipError_t launch_plan_emit_pieces(hipStream_t st, uint32_t n_sub, const PlanWriteIn &in, const uint32_t *sub_n, const uint32_t *sub_flag,
                                   const uint64_t *rec_base, cabac_substream_desc *desc_out, cabac_tu_desc *tus_out, uint64_t *tu_offset,
                                   uint16_t *records, uint32_t *values_out, uint32_t *tu_info_out);
hipError_t launch_plan_stops_pieces(hipStream_t st, uint32_t n_sub, const uint32_t *sub_flag, cabac_substream_result *results,
                                    cabac_coder_state *coder_out);

// the plan resolve of the search rounds (cabac_plan_search.hip; cabac_hip_search_plan.h): the same walk, one candidate per unit,
// into the unit-candidate form.  What both walks read: candidate c owns the entries [ent_first[c], ent_first[c+1]) of plan /
// values and the blocks [cand_first[c], cand_first[c+1]) of the n_tu blocks; tu_info: of launch_residual's sizes pass over tus[].
struct PlanResolveIn {
  uint32_t n_cand;
  const uint32_t *cand_first;
  const uint64_t *ent_first;
  const uint32_t *plan, *values;
  uint32_t n_tu;
  const cabac_tu_desc *tus;
  const uint32_t *tu_at, *tu_guard;  // may be null
  const uint32_t *tu_info;
};
struct PlanResolveOut {  // what the second walk writes (values_out, tu_info_out may be null; values_out may be the values read)
  const uint64_t *rec_first;
  uint16_t *records;
  uint32_t *tu_at_out;
  cabac_tu_desc *tus_out;
  uint32_t *values_out, *tu_info_out;
};
// per candidate the side records it needs (cnt, 0 for a stopped one) and its stop (flags: 0, CABAC_RES_BAD_RECORD,
// CABAC_RES_BAD_VALUE)
hipError_t launch_plan_resolve_count(hipStream_t st, const PlanResolveIn &in, uint32_t *cnt, uint32_t *flags);
// rec_first (n_cand + 1) from cnt, *total (may be null) = the need; a need above `capacity`: rec_first all 0 and
// CABAC_RES_OVERFLOW in the flags of every candidate that has none
hipError_t launch_plan_resolve_scan(hipStream_t st, uint32_t n_cand, const uint32_t *cnt, uint32_t *flags, uint64_t capacity,
                                    uint64_t *rec_first, uint64_t *total);
// the second walk; a candidate with a flag gets the empty form (no record, every block rejected at position 0)
hipError_t launch_plan_resolve_emit(hipStream_t st, const PlanResolveIn &in, uint32_t *cnt, uint32_t *flags, const PlanResolveOut &out);
// frac_bits[c] = UINT64_MAX where flags[c] != 0
hipError_t launch_plan_flag_cost(hipStream_t st, uint32_t n_cand, const uint32_t *flags, uint64_t *frac_bits);

// the fixed workspace (cabac_workspace.hip; cabac_hip_workspace.h): the device words of a ctx whose workspace is fixed.  One
// block serves every call: the calls of a ctx run in stream order.
struct WsState {
  cabac_workspace_status status;
  uint64_t rec_cap, slot_cap;               // the room for expanded records and byte slots the gate compares the totals with
  uint64_t log_entry, log_record, log_tu;   // the log's counters as the fixed place pass took them (all 0 for a log it refuses)
  uint32_t voided;                          // the gate's decision for the call in flight
  uint32_t log_flags;                       // CABAC_WS_LOG_* of the call in flight; the gate takes them and clears them
};
// The residual binariser's scratch (cabac_residual.hip): kResidualScratchHeader words of class counts, cursors and the
// transform-skip flag, then the block order, 0xffffffff where a slot holds no block.  The gate EMPTIES it for a voided call —
// header 0, order 0xffffffff — so that the records pass behind it (order_ready: it takes the order as it finds it) walks no block
// and writes nothing; the binariser's kernels are what they were.
constexpr uint32_t kResidualScratchHeader = 24;
// THE GATE is the tail of the scan of a call on a fixed workspace (launch_splice_plan / launch_splice_scan with a WsGate): the
// call is VOIDED when the scan's error word is set (reported as err_flag), the log's place pass left flags, or a total exceeds its
// room; the status takes the needs, the flags and the counts.  A voided call's tables are emptied — sub_n, sub_cap, rec_base,
// byte_base 0, sub_flag (may be null) CABAC_RES_OVERFLOW, residual_scratch (may be null; of residual_scratch_bytes(n_tu) bytes)
// emptied as said above — so that what follows finds empty substreams with zero-capacity slots and no block; launch_assemble with ws writes its results, {0, CABAC_RES_OVERFLOW}.
struct WsGate {
  WsState *ws;
  uint32_t err_flag;
  uint32_t *sub_flag, *residual_scratch;
  size_t residual_scratch_bytes;
};
// out_set_live[s] = out_set[s], or 0xffffffff for every substream of a voided call
hipError_t launch_ws_out_sets(hipStream_t st, const WsState *ws, uint32_t n_sub, const uint32_t *out_set, uint32_t *out_set_live);
// dst[t] = src[t] for the blocks the log holds (t < ws->log_tu, at most cap)
hipError_t launch_ws_log_info(hipStream_t st, const WsState *ws, uint32_t cap, const uint32_t *src, uint32_t *dst);
// the gated forms of launch_splice_expand and launch_splice_sync_index: a voided call writes its (empty) descriptors and zero
// hand-over indices and reads nothing of the splice list
hipError_t launch_splice_expand_gated(hipStream_t st, const WsState *ws, uint32_t n_sub, const cabac_substream_desc *desc,
                                      const uint16_t *host_records, const uint32_t *splice_first, const cabac_splice *splices,
                                      const uint32_t *pre, const uint32_t *sub_n, const uint32_t *sub_cap, const uint64_t *rec_base,
                                      const uint64_t *byte_base, cabac_substream_desc *desc_out, uint64_t *tu_offset, uint16_t *records);
hipError_t launch_splice_sync_index_gated(hipStream_t st, const WsState *ws, uint32_t n_sub, const cabac_substream_desc *desc,
                                          const uint32_t *splice_first, const cabac_splice *splices, const uint32_t *pre,
                                          const uint32_t *sync_at, const uint32_t *sync_splice, uint32_t *sync_rec);
// launch_search_log_place sized from the log's capacities: the counters are read on the device (ws->log_* and ws->log_flags
// receive them); tus_out receives tu_cap descriptors, the logged ones copied and the unused tail ones the binariser rejects;
// the splice list is the logged blocks' (launch_splice_plan takes their number from &ws->log_tu)
hipError_t launch_search_log_place_fixed(hipStream_t st, const SearchLogArrays &log, WsState *ws, const cabac_substream_desc *desc,
                                         cabac_substream_desc *desc_out, uint32_t *splice_first, uint16_t *records,
                                         cabac_splice *splices, cabac_tu_desc *tus_out);

// substream assembly (cabac_assemble.hip)
hipError_t launch_assemble(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc,
                           const cabac_substream_result *results, const uint8_t *bytes, uint8_t *payload,
                           uint64_t payload_capacity, uint64_t *offsets, const WsState *ws = nullptr,
                           cabac_substream_result *results_w = nullptr);
// ws (a call on a fixed workspace; then results_w = results, writable): a voided call's results are written by the sizes scan
hipError_t launch_pack_bins(hipStream_t st, uint64_t n, const uint8_t *bins, uint8_t *packed);
hipError_t launch_gather_records(hipStream_t st, uint32_t n_seg, const uint64_t *src_off, const uint64_t *dst_off, const uint32_t *len,
                                 const uint16_t *src, uint16_t *dst);
hipError_t launch_split(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc, const uint64_t *offsets,
                        const uint8_t *payload, uint8_t *bytes);
hipError_t launch_count_emulations(hipStream_t st, uint32_t n_sub, const cabac_substream_desc *desc,
                                   const cabac_substream_result *results, const uint8_t *bytes, uint32_t *counts);

}  // namespace cabac
#endif
