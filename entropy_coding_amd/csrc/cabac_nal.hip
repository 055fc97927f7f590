// Emulation prevention on the device (the step after addSubstream): escape a segmented byte string
// into NAL payload bytes (insert 03 in front of a byte <= 3 that follows two zeros) and the inverse.  The contract is the pair
// of sequential walks written out in include/cabac_hip_nal.h; this file restates them so that they run in parallel over
// pieces of the string instead of over segments (a slice may be ten long substreams or one).
//
// Escape.  With k the length of the zero run that ends just before a byte, the byte gets a 03 in front iff it is <= 3, k >= 2
// and k is even (the walk's z is 2 exactly then: an insertion restarts it, so inside a run z goes 1 2 1 2 ...).  k is local
// except for a run that reaches the start of the piece, so a piece needs ONE number from its left, the run entering it, and
// only its leading zero run and the byte behind that run depend on that number.
//   1. summary   one wave per 1 KiB chunk: leading run, trailing run, all-zero?, the byte behind the leading run, and the
//                insertion count for an entering run of 0
//   2. scan      one workgroup: the entering run of every chunk (operator: an all-zero chunk adds its length, any other
//                chunk replaces the value by its trailing run), from it the true count, and the exclusive sum of the counts
//   3. write     one workgroup per 4 KiB tile (4 chunks): 16 bytes per lane, the tile's output built in LDS, stored as
//                aligned dwords
//   4. offsets   one wave per entry point: chunk base + a recount of the chunk up to the offset
// Separate launches are the synchronisation between the passes.  Unescape has the same four passes; its rule is local (a 03 is
// dropped iff exactly two zeros precede it), so its summary is a count and two flags and the scan is a sum.
// Run lengths are carried capped (cap_run): only "0, 1, 2, 3, or more" and the parity matter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip_nal.h"
#include "cabac_nal_kernels.h"

namespace cabac {
namespace {

constexpr uint32_t kChunk = 1024u;            // bytes per wave: 64 lanes x 16
constexpr uint32_t kTileChunks = 4u;          // chunks per workgroup of the write passes
constexpr uint32_t kTile = kChunk * kTileChunks;
constexpr uint32_t kLdsWords = (kTile + kTile / 2u) / 4u + 4u;   // worst case one insertion per two bytes, + the funnel's look-ahead

__device__ inline uint32_t cap_run(uint32_t x) { return x < 4u ? x : (4u | (x & 1u)); }
// number of odd k in [3, m]
__device__ inline uint32_t odd_from_3(uint32_t m) { return m ? (m - 1u) >> 1 : 0u; }

__device__ inline uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ inline uint32_t wave_or(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x |= __shfl_xor(x, d);
  return x;
}
__device__ inline uint32_t wave_excl_sum(uint32_t x, uint32_t lane) {
  uint32_t incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  return incl - x;
}

// the (all-zero, run) pair of a piece and the operator that joins a piece to the one on its left
struct Run {
  uint32_t az, val;   // az: the piece is all zero (val = its length); else val = its trailing zero run
};
__device__ inline Run join(Run left, Run right) { return right.az ? Run{left.az, left.val + right.val} : right; }
__device__ inline Run wave_incl_join(Run r, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Run up{(uint32_t)__shfl_up(r.az, d), (uint32_t)__shfl_up(r.val, d)};
    if ((int)lane >= d) r = join(up, r);
  }
  return r;
}

// bytes [i0, i0 + v) of `p` as four little-endian dwords, the rest 0xff (v <= 16; i0 a multiple of 16)
__device__ inline void load16(const uint8_t *__restrict__ p, uint64_t i0, uint32_t v, bool aligned, uint32_t (&w)[4]) {
  if (v == 16u && aligned) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p + i0);
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    return;
  }
  w[0] = w[1] = w[2] = w[3] = 0xffffffffu;
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++)
    if (j < v) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8u * (j & 3u)))) | ((uint32_t)p[i0 + j] << (8u * (j & 3u)));
}
__device__ inline uint32_t byte_at(const uint32_t (&w)[4], uint32_t j) { return (w[j >> 2] >> (8u * (j & 3u))) & 0xffu; }
// the same for an index known only at run time (selects, so that the dwords stay in registers)
__device__ inline uint32_t byte_at_dyn(const uint32_t (&w)[4], uint32_t j) {
  const uint32_t k = j >> 2, d = k == 0u ? w[0] : k == 1u ? w[1] : k == 2u ? w[2] : w[3];
  return (d >> (8u * (j & 3u))) & 0xffu;
}
__device__ inline uint32_t zero_mask(const uint32_t (&w)[4]) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++) m |= (uint32_t)(byte_at(w, j) == 0u) << j;
  return m;
}

// ---- escape: what a lane knows about its 16 bytes ----
struct EscLane {
  uint32_t w[4], v;
  Run own;        // of the lane's v bytes
  uint32_t lead;  // its leading zero run
};
__device__ inline void esc_lane_load(EscLane &L, const uint8_t *__restrict__ p, uint64_t chunk_base, uint32_t len, uint32_t lane,
                                     bool aligned) {
  const uint32_t at = 16u * lane;
  L.v = len > at ? min(len - at, 16u) : 0u;
  load16(p, chunk_base + at, L.v, aligned, L.w);
  const uint32_t zm = zero_mask(L.w);   // the padding is 0xff: bits only below v
  L.lead = min((uint32_t)__builtin_ctz(~zm | 0x10000u), L.v);
  if (L.lead == L.v) {
    L.own = Run{1u, L.v};
  } else {
    const uint32_t t = zm << (32u - L.v);   // the byte v - 1 at bit 31
    L.own = Run{0u, (uint32_t)__builtin_clz(~t)};
  }
}
// bit j: byte j of the lane gets a 03 in front; `run` = the (capped) zero run ending just before the lane
__device__ inline uint32_t esc_lane_mask(const EscLane &L, uint32_t run) {
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++) {
    const uint32_t b = byte_at(L.w, j);   // padding 0xff: no insertion
    mask |= (uint32_t)(b <= 3u && run >= 2u && !(run & 1u)) << j;
    run = b == 0u ? run + 1u : 0u;
  }
  return mask;
}
// the run entering each lane of a chunk whose own entering run is `enter`; *chunk = the pair of the whole chunk
__device__ inline uint32_t esc_lane_enter(const EscLane &L, uint32_t enter, uint32_t lane, Run *chunk) {
  const Run incl = wave_incl_join(L.own, lane);
  Run ex{(uint32_t)__shfl_up(incl.az, 1), (uint32_t)__shfl_up(incl.val, 1)};
  if (lane == 0u) ex = Run{1u, 0u};
  if (chunk) *chunk = Run{(uint32_t)__shfl(incl.az, 63), (uint32_t)__shfl(incl.val, 63)};
  return cap_run(ex.az ? enter + ex.val : ex.val);
}

__device__ inline uint64_t clipped_len(const uint64_t *__restrict__ offsets, uint32_t n_seg, uint64_t bytes_max) {
  const uint64_t n = offsets[n_seg];
  return n < bytes_max ? n : bytes_max;
}

// pass 1: summ[c] = { lead | trail << 16, count(enter = 0) | byte behind the leading run << 16 | all-zero << 24 }
__global__ __launch_bounds__(256) void nal_escape_summary_kernel(uint32_t n_seg, const uint64_t *__restrict__ offsets,
                                                                 const uint8_t *__restrict__ payload, uint64_t bytes_max,
                                                                 uint2 *__restrict__ summ) {
  const uint64_t n = clipped_len(offsets, n_seg, bytes_max);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t c = (uint64_t)blockIdx.x * kTileChunks + (threadIdx.x >> 6), base = c * kChunk;
  if (base >= n) return;   // a chunk behind the real length: nothing to do
  const uint32_t len = (uint32_t)min((uint64_t)kChunk, n - base);
  EscLane L;
  esc_lane_load(L, payload, base, len, lane, ((uintptr_t)payload & 15u) == 0u);
  Run chunk;
  const uint32_t enter = esc_lane_enter(L, 0u, lane, &chunk);
  const uint32_t cnt = wave_sum((uint32_t)__builtin_popcount(esc_lane_mask(L, enter)));
  // the first lane that is not all zero holds the end of the chunk's leading run and the byte behind it
  const uint64_t open = __ballot(!L.own.az);
  uint32_t lead = len, behind = 0xffu;
  if (open) {
    const int first = __builtin_ctzll(open);
    const uint32_t l = (uint32_t)__shfl((int)L.lead, first);
    const uint32_t b = (uint32_t)__shfl((int)byte_at_dyn(L.w, L.lead & 15u), first);
    lead = 16u * (uint32_t)first + l;
    behind = b;
  }
  if (lane == 0u) summ[c] = make_uint2(lead | (chunk.val << 16), cnt | (behind << 16) | (chunk.az << 24));
}

// insertions of a chunk as a function of the run entering it: only its leading run and the byte behind it depend on that
__device__ inline uint32_t esc_count(uint2 s, uint32_t len, uint32_t enter) {
  const uint32_t lead = s.x & 0xffffu, cnt0 = s.y & 0xffffu, behind = (s.y >> 16) & 0xffu;
  const bool has_behind = lead < len && behind <= 3u;   // (behind is not zero by construction)
  const uint32_t in_run0 = odd_from_3(lead), in_run = odd_from_3(enter + lead) - odd_from_3(enter);
  const uint32_t b0 = has_behind && lead >= 2u && !(lead & 1u), b = has_behind && enter + lead >= 2u && !((enter + lead) & 1u);
  return cnt0 - in_run0 - b0 + in_run + b;
}

// pass 2: one workgroup; groups of 1024 chunks with a running carry
__global__ __launch_bounds__(1024) void nal_escape_scan_kernel(uint32_t n_seg, const uint64_t *__restrict__ offsets, uint64_t bytes_max,
                                                               uint64_t nal_capacity, const uint2 *__restrict__ summ,
                                                               uint32_t *__restrict__ run_in, uint64_t *__restrict__ ins_before,
                                                               cabac_nal_status *__restrict__ status) {
  __shared__ Run wave_run[16];
  __shared__ uint32_t wave_cnt[16];
  __shared__ uint32_t carry_run;
  __shared__ uint64_t carry_ins;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t n_real = offsets[n_seg], n = n_real < bytes_max ? n_real : bytes_max;
  const uint64_t nc = (n + kChunk - 1u) / kChunk;
  if (tid == 0) carry_run = 0, carry_ins = 0;
  __syncthreads();
  for (uint64_t g = 0; g < nc; g += 1024u) {
    const uint64_t c = g + tid;
    const bool in = c < nc;
    const uint32_t len = in ? (uint32_t)min((uint64_t)kChunk, n - c * kChunk) : 0u;
    const uint2 s = in ? summ[c] : make_uint2(0u, 0xffu << 16 | 1u << 24);
    const Run own = in ? Run{s.y >> 24, (s.y >> 24) ? len : (s.x >> 16)} : Run{1u, 0u};
    const Run incl = wave_incl_join(own, lane);
    if (lane == 63u) wave_run[wave] = incl;
    __syncthreads();
    Run left{1u, 0u};   // everything of this group to the left of the thread's wave
    for (uint32_t k = 0; k < wave; k++) left = join(left, wave_run[k]);
    Run ex{(uint32_t)__shfl_up(incl.az, 1), (uint32_t)__shfl_up(incl.val, 1)};
    if (lane == 0u) ex = Run{1u, 0u};
    ex = join(left, ex);
    const uint32_t before = carry_run;
    const uint32_t enter = cap_run(ex.az ? before + ex.val : ex.val);
    const uint32_t cnt = in ? esc_count(s, len, enter) : 0u;
    const uint32_t cnt_ex = wave_excl_sum(cnt, lane);
    if (lane == 63u) wave_cnt[wave] = cnt_ex + cnt;
    __syncthreads();
    uint32_t cnt_left = 0;
    for (uint32_t k = 0; k < wave; k++) cnt_left += wave_cnt[k];
    const uint64_t ins = carry_ins + cnt_left + cnt_ex;
    if (in) run_in[c] = enter, ins_before[c] = ins;
    __syncthreads();
    if (tid == 1023u) {
      const Run all = join(left, incl);
      carry_run = cap_run(all.az ? before + all.val : all.val);
      carry_ins = ins + cnt;
    }
    __syncthreads();
  }
  if (tid == 0) {
    run_in[nc] = carry_run;
    ins_before[nc] = carry_ins;
    cabac_nal_status st;
    st.out_bytes = n + carry_ins;
    st.n_changed = carry_ins > 0xffffffffull ? 0xffffffffu : (uint32_t)carry_ins;
    st.flags = (st.out_bytes > nal_capacity ? CABAC_NAL_OVERFLOW : 0u) | (n && carry_run ? CABAC_NAL_TRAILING_ZERO : 0u) |
               (n_real > bytes_max ? CABAC_NAL_INPUT_CLIPPED : 0u);
    *status = st;
  }
}

// the tile's output, `m` bytes in LDS from byte 0, to out[o0 ..) below `capacity`: single bytes up to the first aligned
// dword and behind the last one, aligned dwords between (the LDS side is read through a funnel shift)
__device__ inline void flush_tile(const uint32_t *lds, uint8_t *__restrict__ out, uint64_t o0, uint64_t m, uint64_t capacity) {
  if (o0 >= capacity) return;
  if (m > capacity - o0) m = capacity - o0;
  const uint8_t *lds8 = reinterpret_cast<const uint8_t *>(lds);
  uint8_t *g = out + o0;
  const uint32_t head = (uint32_t)min((uint64_t)((4u - ((uintptr_t)g & 3u)) & 3u), m);
  const uint32_t n_dw = (uint32_t)((m - head) >> 2), tail_at = head + 4u * n_dw;
  if (threadIdx.x < head) g[threadIdx.x] = lds8[threadIdx.x];
  uint32_t *g32 = reinterpret_cast<uint32_t *>(g + head);
  for (uint32_t i = threadIdx.x; i < n_dw; i += blockDim.x) {
    const uint32_t q = head + 4u * i;
    const uint64_t two = (uint64_t)lds[q >> 2] | ((uint64_t)lds[(q >> 2) + 1u] << 32);
    g32[i] = (uint32_t)(two >> (8u * (q & 3u)));
  }
  if (threadIdx.x < (uint32_t)m - tail_at) g[tail_at + threadIdx.x] = lds8[tail_at + threadIdx.x];
}

// pass 3
__global__ __launch_bounds__(256) void nal_escape_write_kernel(uint32_t n_seg, const uint64_t *__restrict__ offsets,
                                                               const uint8_t *__restrict__ payload, uint64_t bytes_max,
                                                               const uint32_t *__restrict__ run_in, const uint64_t *__restrict__ ins_before,
                                                               uint8_t *__restrict__ nal, uint64_t nal_capacity) {
  __shared__ uint32_t lds[kLdsWords];
  const uint64_t n = clipped_len(offsets, n_seg, bytes_max);
  const uint64_t c0 = (uint64_t)blockIdx.x * kTileChunks, tile_base = c0 * kChunk;
  if (tile_base >= n) return;
  const uint64_t nc = (n + kChunk - 1u) / kChunk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t c = c0 + (threadIdx.x >> 6), base = c * kChunk;
  const uint64_t tile_ins = ins_before[c0];
  uint8_t *lds8 = reinterpret_cast<uint8_t *>(lds);
  if (base < n) {
    const uint32_t len = (uint32_t)min((uint64_t)kChunk, n - base);
    EscLane L;
    esc_lane_load(L, payload, base, len, lane, ((uintptr_t)payload & 15u) == 0u);
    const uint32_t mask = esc_lane_mask(L, esc_lane_enter(L, run_in[c], lane, nullptr));
    const uint32_t cnt = (uint32_t)__builtin_popcount(mask);
    uint32_t pos = (uint32_t)(base - tile_base) + (uint32_t)(ins_before[c] - tile_ins) + 16u * lane + wave_excl_sum(cnt, lane);
    if (mask == 0u && L.v == 16u && (pos & 3u) == 0u) {   // nearly every lane: a shifted copy
      lds[(pos >> 2) + 0u] = L.w[0], lds[(pos >> 2) + 1u] = L.w[1], lds[(pos >> 2) + 2u] = L.w[2], lds[(pos >> 2) + 3u] = L.w[3];
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16u; j++)
        if (j < L.v) {
          if ((mask >> j) & 1u) lds8[pos++] = 3u;
          lds8[pos++] = (uint8_t)byte_at(L.w, j);
        }
    }
  }
  __syncthreads();
  const uint64_t c1 = min(c0 + kTileChunks, nc);
  const uint64_t m = (min(n, tile_base + kTile) - tile_base) + (ins_before[c1] - tile_ins);
  flush_tile(lds, nal, tile_base + tile_ins, m, nal_capacity);
}

// pass 4: nal_offsets[s] = o + insertions in front of raw positions < o, o = offsets[s] clipped to the length
__global__ __launch_bounds__(256) void nal_escape_offsets_kernel(uint32_t n_seg, const uint64_t *__restrict__ offsets,
                                                                 const uint8_t *__restrict__ payload, uint64_t bytes_max,
                                                                 const uint32_t *__restrict__ run_in, const uint64_t *__restrict__ ins_before,
                                                                 uint64_t *__restrict__ nal_offsets) {
  const uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (s > n_seg) return;
  const uint64_t n = clipped_len(offsets, n_seg, bytes_max);
  const uint64_t o = min(offsets[s], n), c = o / kChunk;
  const uint32_t within = (uint32_t)(o % kChunk);
  uint32_t cnt = 0;
  if (within) {   // (a wave-uniform branch) the chunk's bytes in front of o: the walk up to there does not look ahead
    EscLane L;
    esc_lane_load(L, payload, c * kChunk, within, lane, ((uintptr_t)payload & 15u) == 0u);
    cnt = wave_sum((uint32_t)__builtin_popcount(esc_lane_mask(L, esc_lane_enter(L, run_in[c], lane, nullptr))));
  }
  if (lane == 0u) nal_offsets[s] = o + ins_before[c] + cnt;
}

// ---- unescape ----
// bit j of the result: byte j of the lane is a 03 to drop (exactly two zeros in front of it).  `before` holds the three
// bytes in front of the lane (the earliest in bits 0..7; 0xff where the string has not begun), `after` the byte behind
// it (0 where the string ends).  *flags gains FORBIDDEN / BAD_ESCAPE as this lane's bytes show them.
__device__ inline uint32_t unesc_lane_mask(const uint32_t (&w)[4], uint32_t v, uint32_t before, uint32_t after, uint32_t *flags) {
  // window bit t: t = 0..2 the bytes in front, t = 3..18 the lane's, t = 19 the one behind
  uint32_t zm = 0, m3 = 0, le2 = 0, gt3 = 0;
#pragma unroll
  for (uint32_t t = 0; t < 3u; t++) zm |= (uint32_t)(((before >> (8u * t)) & 0xffu) == 0u) << t;
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++) {
    const uint32_t b = byte_at(w, j);   // padding 0xff
    zm |= (uint32_t)(b == 0u) << (j + 3u);
    m3 |= (uint32_t)(b == 3u) << (j + 3u);
    le2 |= (uint32_t)(b <= 2u) << (j + 3u);
    gt3 |= (uint32_t)(b > 3u && j < v) << (j + 3u);
  }
  gt3 |= (uint32_t)(v == 16u && after > 3u) << 19;
  const uint32_t two = (zm << 1) & (zm << 2);
  const uint32_t rem = m3 & two & ~(zm << 3);
  if (flags) *flags |= ((le2 & two) ? CABAC_NAL_FORBIDDEN : 0u) | ((rem & (gt3 >> 1)) ? CABAC_NAL_BAD_ESCAPE : 0u);
  return (rem >> 3) & 0xffffu;
}

struct UnLane {
  uint32_t w[4], v, before, after;
};
__device__ inline void un_lane_load(UnLane &L, const uint8_t *__restrict__ p, uint64_t chunk_base, uint32_t len, uint64_t n,
                                    uint32_t lane, bool aligned, bool want_after) {
  const uint32_t at = 16u * lane;
  const uint64_t i0 = chunk_base + at;
  L.v = len > at ? min(len - at, 16u) : 0u;
  load16(p, i0, L.v, aligned, L.w);
  L.before = 0xffffffu;
  L.after = 0u;
  if (L.v == 0u) return;
  if (i0) {   // i0 >= 16
    if (aligned) L.before = *reinterpret_cast<const uint32_t *>(p + i0 - 4u) >> 8;
    else L.before = (uint32_t)p[i0 - 3u] | ((uint32_t)p[i0 - 2u] << 8) | ((uint32_t)p[i0 - 1u] << 16);
  }
  if (want_after && L.v == 16u && i0 + 16u < n) L.after = p[i0 + 16u];
}

// pass 1: summ[c] = { removals, flags }
__global__ __launch_bounds__(256) void nal_unescape_summary_kernel(uint32_t n_seg, const uint64_t *__restrict__ nal_offsets,
                                                                   const uint8_t *__restrict__ nal, uint64_t bytes_max,
                                                                   uint2 *__restrict__ summ) {
  const uint64_t n = clipped_len(nal_offsets, n_seg, bytes_max);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t c = (uint64_t)blockIdx.x * kTileChunks + (threadIdx.x >> 6), base = c * kChunk;
  if (base >= n) return;
  const uint32_t len = (uint32_t)min((uint64_t)kChunk, n - base);
  UnLane L;
  un_lane_load(L, nal, base, len, n, lane, ((uintptr_t)nal & 15u) == 0u, true);
  uint32_t flags = 0;
  const uint32_t mask = unesc_lane_mask(L.w, L.v, L.before, L.after, &flags);
  const uint32_t cnt = wave_sum((uint32_t)__builtin_popcount(mask));
  flags = wave_or(flags);
  if (lane == 0u) summ[c] = make_uint2(cnt, flags);
}

// pass 2
__global__ __launch_bounds__(1024) void nal_unescape_scan_kernel(uint32_t n_seg, const uint64_t *__restrict__ nal_offsets,
                                                                 uint64_t bytes_max, uint64_t payload_capacity, int want_loc,
                                                                 uint64_t loc_capacity, const uint2 *__restrict__ summ,
                                                                 uint64_t *__restrict__ rem_before, cabac_nal_status *__restrict__ status) {
  __shared__ uint32_t wave_cnt[16], wave_flags[16];
  __shared__ uint64_t carry;
  __shared__ uint32_t carry_flags;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t n_real = nal_offsets[n_seg], n = n_real < bytes_max ? n_real : bytes_max;
  const uint64_t nc = (n + kChunk - 1u) / kChunk;
  if (tid == 0) carry = 0, carry_flags = 0;
  __syncthreads();
  for (uint64_t g = 0; g < nc; g += 1024u) {
    const uint64_t c = g + tid;
    const uint2 s = c < nc ? summ[c] : make_uint2(0u, 0u);
    const uint32_t ex = wave_excl_sum(s.x, lane), fl = wave_or(s.y);
    if (lane == 63u) wave_cnt[wave] = ex + s.x, wave_flags[wave] = fl;
    __syncthreads();
    uint32_t left = 0;
    for (uint32_t k = 0; k < wave; k++) left += wave_cnt[k];
    const uint64_t before = carry + left + ex;
    if (c < nc) rem_before[c] = before;
    __syncthreads();
    if (tid == 1023u) {
      uint32_t f = carry_flags;
      for (uint32_t k = 0; k < 16u; k++) f |= wave_flags[k];
      carry_flags = f;
      carry = before + s.x;
    }
    __syncthreads();
  }
  if (tid == 0) {
    rem_before[nc] = carry;
    cabac_nal_status st;
    st.out_bytes = n - carry;
    st.n_changed = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
    st.flags = carry_flags | (st.out_bytes > payload_capacity ? CABAC_NAL_OVERFLOW : 0u) |
               (want_loc && carry > loc_capacity ? CABAC_NAL_LOC_OVERFLOW : 0u) | (n_real > bytes_max ? CABAC_NAL_INPUT_CLIPPED : 0u);
    *status = st;
  }
}

// pass 3: the compacting write and the location list
__global__ __launch_bounds__(256) void nal_unescape_write_kernel(uint32_t n_seg, const uint64_t *__restrict__ nal_offsets,
                                                                 const uint8_t *__restrict__ nal, uint64_t bytes_max,
                                                                 const uint64_t *__restrict__ rem_before, uint8_t *__restrict__ payload,
                                                                 uint64_t payload_capacity, uint32_t *__restrict__ locations,
                                                                 uint64_t loc_capacity, uint32_t loc_base) {
  __shared__ uint32_t lds[kTile / 4u + 4u];
  const uint64_t n = clipped_len(nal_offsets, n_seg, bytes_max);
  const uint64_t c0 = (uint64_t)blockIdx.x * kTileChunks, tile_base = c0 * kChunk;
  if (tile_base >= n) return;
  const uint64_t nc = (n + kChunk - 1u) / kChunk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t c = c0 + (threadIdx.x >> 6), base = c * kChunk;
  const uint64_t tile_rem = rem_before[c0];
  uint8_t *lds8 = reinterpret_cast<uint8_t *>(lds);
  if (base < n) {
    const uint32_t len = (uint32_t)min((uint64_t)kChunk, n - base);
    UnLane L;
    un_lane_load(L, nal, base, len, n, lane, ((uintptr_t)nal & 15u) == 0u, false);
    uint32_t mask = unesc_lane_mask(L.w, L.v, L.before, 0u, nullptr);
    const uint32_t cnt = (uint32_t)__builtin_popcount(mask), ex = wave_excl_sum(cnt, lane);
    const uint64_t chunk_rem = rem_before[c];
    uint32_t pos = (uint32_t)(base - tile_base) - (uint32_t)(chunk_rem - tile_rem) + 16u * lane - ex;
    if (mask == 0u && L.v == 16u && (pos & 3u) == 0u) {
      lds[(pos >> 2) + 0u] = L.w[0], lds[(pos >> 2) + 1u] = L.w[1], lds[(pos >> 2) + 2u] = L.w[2], lds[(pos >> 2) + 3u] = L.w[3];
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16u; j++)
        if (j < L.v && !((mask >> j) & 1u)) lds8[pos++] = (uint8_t)byte_at(L.w, j);
    }
    if (locations) {
      uint64_t idx = chunk_rem + ex;
      while (mask) {   // rare
        const uint32_t j = (uint32_t)__builtin_ctz(mask);
        mask &= mask - 1u;
        if (idx < loc_capacity) locations[idx] = (uint32_t)(base + 16u * lane + j) + loc_base;
        idx++;
      }
    }
  }
  __syncthreads();
  const uint64_t c1 = min(c0 + kTileChunks, nc);
  const uint64_t m = (min(n, tile_base + kTile) - tile_base) - (rem_before[c1] - tile_rem);
  flush_tile(lds, payload, tile_base - tile_rem, m, payload_capacity);
}

// pass 4: offsets[s] = o - removals at NAL positions < o
__global__ __launch_bounds__(256) void nal_unescape_offsets_kernel(uint32_t n_seg, const uint64_t *__restrict__ nal_offsets,
                                                                   const uint8_t *__restrict__ nal, uint64_t bytes_max,
                                                                   const uint64_t *__restrict__ rem_before, uint64_t *__restrict__ offsets) {
  const uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (s > n_seg) return;
  const uint64_t n = clipped_len(nal_offsets, n_seg, bytes_max);
  const uint64_t o = min(nal_offsets[s], n), c = o / kChunk;
  const uint32_t within = (uint32_t)(o % kChunk);
  uint32_t cnt = 0;
  if (within) {
    UnLane L;
    un_lane_load(L, nal, c * kChunk, within, n, lane, ((uintptr_t)nal & 15u) == 0u, false);
    cnt = wave_sum((uint32_t)__builtin_popcount(unesc_lane_mask(L.w, L.v, L.before, 0u, nullptr)));
  }
  if (lane == 0u) offsets[s] = o - rem_before[c] - cnt;
}

struct Scratch {
  uint2 *summ;
  uint64_t *changed_before;
  uint32_t *run_in;
};
uint64_t max_chunks(uint64_t bytes_max) { return (bytes_max + kChunk - 1u) / kChunk; }
Scratch carve(void *scratch, uint64_t bytes_max) {
  const uint64_t nc = max_chunks(bytes_max);
  Scratch s;
  s.summ = static_cast<uint2 *>(scratch);
  s.changed_before = reinterpret_cast<uint64_t *>(s.summ + nc);
  s.run_in = reinterpret_cast<uint32_t *>(s.changed_before + nc + 1u);
  return s;
}

}  // namespace

size_t nal_scratch_bytes(uint64_t bytes_max) {
  const uint64_t nc = max_chunks(bytes_max);
  return (size_t)(nc * sizeof(uint2) + (nc + 1u) * sizeof(uint64_t) + (nc + 1u) * sizeof(uint32_t));
}

hipError_t launch_nal_escape(hipStream_t st, uint32_t n_seg, const uint64_t *offsets, const uint8_t *payload, uint64_t payload_bytes_max,
                             uint8_t *nal, uint64_t nal_capacity, uint64_t *nal_offsets, cabac_nal_status *status, void *scratch) {
  const Scratch s = carve(scratch, payload_bytes_max);
  const uint64_t tiles = (max_chunks(payload_bytes_max) + kTileChunks - 1u) / kTileChunks;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  if (tiles)
    hipLaunchKernelGGL(nal_escape_summary_kernel, dim3((uint32_t)tiles), dim3(256), 0, st, n_seg, offsets, payload, payload_bytes_max,
                       s.summ);
  hipLaunchKernelGGL(nal_escape_scan_kernel, dim3(1), dim3(1024), 0, st, n_seg, offsets, payload_bytes_max, nal_capacity, s.summ,
                     s.run_in, s.changed_before, status);
  if (tiles)
    hipLaunchKernelGGL(nal_escape_write_kernel, dim3((uint32_t)tiles), dim3(256), 0, st, n_seg, offsets, payload, payload_bytes_max,
                       s.run_in, s.changed_before, nal, nal_capacity);
  hipLaunchKernelGGL(nal_escape_offsets_kernel, dim3(n_seg / 4u + 1u), dim3(256), 0, st, n_seg, offsets, payload, payload_bytes_max,
                     s.run_in, s.changed_before, nal_offsets);
  return hipGetLastError();
}

hipError_t launch_nal_unescape(hipStream_t st, uint32_t n_seg, const uint64_t *nal_offsets, const uint8_t *nal, uint64_t nal_bytes_max,
                               uint8_t *payload, uint64_t payload_capacity, uint64_t *offsets, uint32_t *locations, uint64_t loc_capacity,
                               uint32_t loc_base, cabac_nal_status *status, void *scratch) {
  const Scratch s = carve(scratch, nal_bytes_max);
  const uint64_t tiles = (max_chunks(nal_bytes_max) + kTileChunks - 1u) / kTileChunks;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  if (tiles)
    hipLaunchKernelGGL(nal_unescape_summary_kernel, dim3((uint32_t)tiles), dim3(256), 0, st, n_seg, nal_offsets, nal, nal_bytes_max,
                       s.summ);
  hipLaunchKernelGGL(nal_unescape_scan_kernel, dim3(1), dim3(1024), 0, st, n_seg, nal_offsets, nal_bytes_max, payload_capacity,
                     locations ? 1 : 0, loc_capacity, s.summ, s.changed_before, status);
  if (tiles)
    hipLaunchKernelGGL(nal_unescape_write_kernel, dim3((uint32_t)tiles), dim3(256), 0, st, n_seg, nal_offsets, nal, nal_bytes_max,
                       s.changed_before, payload, payload_capacity, locations, loc_capacity, loc_base);
  hipLaunchKernelGGL(nal_unescape_offsets_kernel, dim3(n_seg / 4u + 1u), dim3(256), 0, st, n_seg, nal_offsets, nal, nal_bytes_max,
                     s.changed_before, offsets);
  return hipGetLastError();
}

}  // namespace cabac
