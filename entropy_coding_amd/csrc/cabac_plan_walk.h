// The plan walk on the writer's side, shared by the plan write (cabac_plan_write.hip) and the plan resolve of the search rounds
// (cabac_plan_search.hip): a plan of syntax elements, guards, computed entries and guarded blocks (cabac_hip_parse_plan.h) plus the
// values of the real elements and the info words of the blocks -> which elements and blocks are coded, the filled values, the
// elements' bin records.  What tests/parse_plan_model.py::fill / expand do on the CPU.
//
// The walk.  One wave per UNIT (a substream of the plan write, a candidate of the plan resolve).  The only serial thing in a plan
// is liveness along reference chains (a guard on a COND on a guarded element ...), so the wave does not step through the entries:
// it takes a STAGE of up to 64 consecutive entries with no block position inside, one entry per lane, and lets every lane resolve
// its entry as soon as the entries it refers to are resolved — those in front of the stage are (their values lie in the ring),
// those inside it are named by a ballot.  The number of rounds is the depth of the reference chain inside the stage (2 - 4 in the
// worked transform unit), at most the stage's width: the lowest unresolved lane refers to lower lanes only and is always ready.
// Between two stages the blocks at that position are taken 64 at a time; their guards refer to entries in front of them, so one
// round does.  LDS per wave: the ring of the last 256 values, the last 16 info words (the count of blocks walked is wave-uniform
// and lives in a register), and the tile of the output-position loop.  Every loop is bounded by the unit's entries, its blocks and
// 64; no workgroup waits for another; no atomics on the data path.
//
// Where a unit's plan range lies and where its results go is the caller's: plan_walk<kEmit, Io> takes an Io that says
//   n_units                                     units of the launch, one wave each
//   tus, tu_at, tu_guard, tu_info               the blocks (tu_at, tu_guard may be null), tu_info: the sizes pass's info words
//   tu_n_records                                the sizes pass's record counts, read only where kBlocksInRun
//   kBlocksInRun                                true: a coded block's records count into the unit's run (the plan write's expanded
//                                               substream); false: the run holds the elements' bins alone (the plan resolve)
//   unit(k)                                     -> PlanWalkUnit: the unit's entries, values in / out and blocks [t0, t1)
//   count_end(k, bad_rec, bad_val, off)         first walk (kEmit false), lane 0: the stop and the length of the run
//   emit_begin(k, unit, lane, base)             second walk, every lane: sets base, the unit's first record in `records`; false:
//                                               the unit is not walked (it has written what a stopped unit gets)
//   emit_block(t, coded, base, off, excl, info) second walk, the lane of block t: `off` records of the unit in front of the run of
//                                               blocks at this position, `excl` those of the coded blocks of the run in front of it
//   records                                     second walk: the elements' bins go to records[base + their place in the run]
// plan_walk<true, true> (the rows form of the plan write, cabac_hip_plan_rows.h) asks two things more of the Io:
//   sync_at(k)                                  the unit's hand-over entry
//   emit_sync(k, off)                           second walk, one lane: `off` records of the unit lie in front of that entry — the
//                                               elements' bins and the records of the coded blocks at positions up to it (behind
//                                               the run for an entry at or behind the end of the plan; 0 for a unit not walked)
// With kSync false, the default, nothing of this is instantiated.
#ifndef CABAC_PLAN_WALK_H
#define CABAC_PLAN_WALK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_hip_parse_elements.h"
#include "cabac_hip_parse_plan.h"
#include "cabac_se_code.h"

namespace cabac {

namespace {

constexpr uint32_t kPwWaves = 4;  // units per workgroup

struct PwLds {
  uint32_t ring[256];  // value(i) at ring[i & 255]
  uint32_t inf[16];    // info word of block k of the unit at inf[k & 15]
  uint32_t scan[65];   // output-position loop: exclusive bin offsets of the stage's elements
  uint32_t w0s[64], vals[64];
};

// orders the LDS accesses of the lanes of one wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane, uint32_t *total) {
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  *total = __shfl(incl, 63);
  return incl - v;
}

__device__ __forceinline__ bool test_holds(uint32_t gw, uint32_t v) {
  const uint32_t imm = gw >> 16, cmp = (gw >> 8) & 3u;
  return cmp == 0u ? v != imm : cmp == 1u ? v == imm : cmp == 2u ? v >= imm : v < imm;
}

// the list of cabac_hip_parse_plan.h; i: the entry's index in its plan, nb: nb(i)
__device__ __forceinline__ bool bad_entry(uint32_t w0, uint32_t gw, uint32_t i, uint32_t nb) {
  const uint32_t kind = w0 & 15u, p = w0 >> 4, id0 = p & 0x1ffu, idn = (p >> 9) & 0x1ffu;
  bool bad = kind > CABAC_PE_BLOCK_INFO || (gw & 0xfc00u) != 0u || (gw & 0xffu) > i;
  if (kind == CABAC_SE_CTX_BIN) bad |= id0 >= (uint32_t)CABAC_NUM_CONTEXTS;
  else if (kind == CABAC_SE_UNARY_MAX) bad |= id0 >= (uint32_t)CABAC_NUM_CONTEXTS || idn >= (uint32_t)CABAC_NUM_CONTEXTS;
  else if (kind == CABAC_SE_EP_BINS || kind == CABAC_SE_UNARY_EP) bad |= (p & 63u) > 32u;
  else if (kind == CABAC_SE_TRUNC_BIN) bad |= p == 0u;
  else if (kind == CABAC_SE_REM_ABS) {
    const uint32_t ml = (p >> 10) & 63u;
    bad |= (p & 31u) > 14u || ml < 15u || ml > 20u || ((p >> 5) & 31u) > 32u - ml;
  } else if (kind == CABAC_PE_COND) {
    const uint32_t back2 = p & 0xffu, join = (p >> 8) & 3u;
    bad |= join == 3u || (join != 0u && (back2 == 0u || back2 > i));
  } else if (kind == CABAC_PE_BLOCK_INFO) {
    const uint32_t width = (p >> 9) & 63u;
    bad |= (p & 15u) >= nb || width == 0u || ((p >> 4) & 31u) + width > 32u;
  }
  return bad;
}

// the values an element's code carries (cabac_hip_write_plan.h, "BAD VALUE"); the entry is a real one and not bad
__device__ __forceinline__ bool in_domain(uint32_t w0, uint32_t v) {
  const uint32_t kind = w0 & 15u, p = w0 >> 4;
  switch (kind) {
  case CABAC_SE_CTX_BIN:
  case CABAC_SE_TRM: return v <= 1u;
  case CABAC_SE_EP_BINS: return (p & 63u) >= 32u || v < (1u << (p & 63u));
  case CABAC_SE_UNARY_MAX: return v <= ((p >> 18) & 0xffu);
  case CABAC_SE_UNARY_EP: return v <= (p & 63u);
  case CABAC_SE_TRUNC_BIN: return v < p;
  case CABAC_SE_EXP_GOLOMB: return v < 0u - (1u << (p & 31u));  // count + prefix ones < 32
  case CABAC_SE_REM_ABS: {  // up to the longest prefix and a suffix of ones
    const uint32_t rice = p & 31u, cutoff = (p >> 5) & 31u, ml = (p >> 10) & 63u;
    const uint64_t top = ((((uint64_t)1 << (32u - ml - cutoff)) + cutoff - 1u) << rice) + ((uint64_t)1 << ml) - 1u;
    return (uint64_t)v <= top;
  }
  default: return true;  // ALIGN carries no value
  }
}

struct PlanWalkUnit {
  const uint2 *plan;    // its entries
  const uint32_t *vin;  // the values of its real elements
  uint32_t *vout;       // second walk: receives the filled values (may be null, may be vin)
  uint32_t n, t0, t1;   // entries; its blocks [t0, t1)
};

template <bool kEmit, bool kSync = false, class Io>
__device__ __forceinline__ void plan_walk(const Io &io) {
  static_assert(kEmit || !kSync, "the hand-over index belongs to the second walk");
  __shared__ PwLds lds_all[kPwWaves];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x * kPwWaves + wave;
  if (unit >= io.n_units) return;
  PwLds &lds = lds_all[wave];
  const PlanWalkUnit u = io.unit(unit);
  const uint32_t n = u.n, t0 = u.t0, t1 = u.t1;
  uint64_t base = 0;
  if (kEmit && !io.emit_begin(unit, u, lane, base)) {
    if constexpr (kSync) {
      if (lane == 0u) io.emit_sync(unit, 0u);
    }
    return;
  }
  [[maybe_unused]] uint32_t sync_at = 0;
  if constexpr (kSync) sync_at = min(io.sync_at(unit), n);

  uint32_t i = 0, t = t0, nb = 0;  // the next element, the next block, the blocks walked (all wave-uniform)
  uint64_t off = 0;                // records of the unit so far
  bool bad_rec = false, bad_val = false;
  while (i < n || t < t1) {
    // Everything either kind of trip reads from memory is asked for here, at once and unconditionally: the walk is bound by
    // latency (one wave per unit, up to a few hundred trips in a row), so a trip must cost one round to memory, not one per
    // decision.  The half that the trip does not use stays in flight behind it.
    const uint32_t idx = i + lane, tt = t + lane;
    uint32_t w0 = 0xfu, gw = 0, value_in = 0;
    if (idx < n) {
      const uint2 w = u.plan[idx];
      w0 = w.x;
      gw = w.y;
      value_in = u.vin[idx];
    }
    uint32_t raw_at = n, gw_b = 0, raw_info = 0, cnt_b = 0, fl_b = 0;
    if (tt < t1) {
      if (io.tu_at) raw_at = io.tu_at[tt];
      if (io.tu_guard) gw_b = io.tu_guard[tt];
      raw_info = io.tu_info[tt];
      if (Io::kBlocksInRun) cnt_b = io.tu_n_records[tt];
      fl_b = io.tus[tt].flags;
    }
    const uint32_t at_next = t < t1 ? min(max((uint32_t)__shfl((int)raw_at, 0), i), n) : n;
    if (t < t1 && at_next == i) {
      // ---- the blocks at position i, up to 64 of them: their guards refer to elements in front of i ----
      const bool here = tt < t1 && (i == n || raw_at <= i);
      const uint64_t not_here = ~__ballot(here);
      const uint32_t m = not_here ? (uint32_t)__builtin_ctzll(not_here) : 64u;  // the run of blocks whose at(t) is i
      const bool mine = lane < m;
      uint32_t info = CABAC_TU_INFO_NOT_CODED, sz = 0;
      bool coded = false, b_rec = false, b_val = false;
      if (mine) {
        const uint32_t back = gw_b & 0xffu;
        b_rec = !kEmit && ((gw_b & 0xfc00u) != 0u || back > i);  // (the second walk sees no stopped unit)
        coded = back == 0u || test_holds(gw_b, lds.ring[(i - back) & 255u]);
        if (coded) {
          b_val = !kEmit && (raw_info & (CABAC_TU_INFO_EMPTY | CABAC_TU_INFO_BAD_DESC)) != 0u;
          // the binariser reports a position for a transform-skip block too; the reader reports CABAC_TU_INFO_TS alone
          info = b_val ? raw_info : (fl_b & CABAC_TU_TRANSFORM_SKIP) ? CABAC_TU_INFO_TS : raw_info;
          sz = b_val ? 0u : cnt_b;
        }
      }
      bad_rec |= __ballot(b_rec) != 0ull;
      bad_val |= __ballot(b_val) != 0ull;
      uint32_t total;
      const uint32_t excl = wave_excl_scan(sz, lane, &total);
      wave_sync();  // the ring and the info words read so far, before the info words change
      if (mine && lane + 16u >= m) lds.inf[(nb + lane) & 15u] = info;  // the last 16 of the run
      wave_sync();
      if (kEmit && mine) io.emit_block(tt, coded, base, off, excl, info);
      nb += m;
      t += m;
      off += total;
      continue;
    }
    // ---- a stage of elements [i, e): no block position inside ----
    const uint32_t e = min(i + 64u, at_next);
    const bool valid = idx < e;
    if (!valid) {
      w0 = 0xfu;
      gw = 0;
    }
    uint32_t v = 0;
    const uint32_t kind = w0 & 15u;
    const bool bad = !kEmit && valid && bad_entry(w0, gw, idx, nb);  // (the second walk sees no stopped unit)
    bad_rec |= __ballot(bad) != 0ull;
    const bool real = valid && kind <= CABAC_SE_ALIGN;
    // what the entry refers to: r1 the guard's (the test's) element, r2 a COND's second one; 0: none
    const uint32_t r1 = valid ? (gw & 0xffu) : 0u;
    const uint32_t r2 = (valid && kind == CABAC_PE_COND && ((w0 >> 12) & 3u) != 0u) ? ((w0 >> 4) & 0xffu) : 0u;
    // values in front of the stage are read now: their ring slots may be overwritten by this stage (a reference 255 back lies
    // in the slot of the next element)
    uint32_t v1 = 0, v2 = 0;
    if (r1 > lane) v1 = lds.ring[(idx - r1) & 255u];
    if (r2 > lane) v2 = lds.ring[(idx - r2) & 255u];
    wave_sync();
    uint64_t done = ~__ballot(valid);
    bool resolved = !valid, active = false;
    for (uint32_t round = 0; round < 64u && done != ~0ull; round++) {
      const bool dep1 = r1 == 0u || r1 > lane || ((done >> (lane - r1)) & 1ull) != 0ull;
      const bool dep2 = r2 == 0u || r2 > lane || ((done >> (lane - r2)) & 1ull) != 0ull;
      const bool ready = !resolved && dep1 && dep2;
      if (ready) {
        if (r1 != 0u && r1 <= lane) v1 = lds.ring[(idx - r1) & 255u];
        if (r2 != 0u && r2 <= lane) v2 = lds.ring[(idx - r2) & 255u];
        const bool holds = r1 == 0u || test_holds(gw, v1);
        if (kind == CABAC_PE_COND) {
          const uint32_t join = (w0 >> 12) & 3u, other = v2 != 0u ? 1u : 0u;
          v = holds ? 1u : 0u;
          if (join == 1u) v &= other;
          else if (join == 2u) v |= other;
        } else if (kind == CABAC_PE_BLOCK_INFO) {
          if (holds && !bad) {
            const uint32_t p = w0 >> 4, width = (p >> 9) & 63u, word = lds.inf[(nb - 1u - (p & 15u)) & 15u];
            v = (word >> ((p >> 4) & 31u)) & (width >= 32u ? 0xffffffffu : (1u << width) - 1u);
          }
        } else if (real && holds) {
          active = true;
          v = value_in;
        }
        lds.ring[idx & 255u] = v;
        resolved = true;
      }
      done |= __ballot(ready);
      wave_sync();
    }
    // the active elements' bins; a value its code does not carry stops the unit
    const bool outside = !kEmit && active && !bad && !in_domain(w0, v);
    bad_val |= __ballot(outside) != 0ull;
    active = active && !bad && !outside;
    const uint32_t cnt = active ? se_decode(w0, v).n : 0u;
    uint32_t total;
    const uint32_t excl = wave_excl_scan(cnt, lane, &total);
    if constexpr (kSync) {  // the hand-over entry lies in this stage: the blocks at its position have been taken in front of it
      if (idx == sync_at && valid) io.emit_sync(unit, off + excl);
    }
    if (kEmit) {
      if (u.vout && valid) u.vout[idx] = v;
      // by output position: bin o of the stage belongs to the last element whose offset is <= o
      lds.scan[lane] = excl;
      lds.w0s[lane] = active ? w0 : 0xfu;
      lds.vals[lane] = v;
      if (lane == 0u) lds.scan[64] = total;
      wave_sync();
      uint16_t *dst = io.records + base + off;
      for (uint32_t o = lane; o < total; o += 64u) {
        uint32_t lo = 0, hi = 64;  // invariant: scan[lo] <= o < scan[hi]
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (lds.scan[mid] <= o) lo = mid;
          else hi = mid;
        }
        const SeCode s = se_decode(lds.w0s[lo], lds.vals[lo]);
        dst[o] = se_bin(s, o - lds.scan[lo]);
      }
      wave_sync();
    }
    off += total;
    i = e;
  }
  if (!kEmit && lane == 0u) io.count_end(unit, bad_rec, bad_val, off);
  if constexpr (kSync) {
    if (sync_at >= n && lane == 0u) io.emit_sync(unit, off);
  }
}

}  // namespace

}  // namespace cabac
#endif
