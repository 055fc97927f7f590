// The device binariser's code of one syntax element (cabac_hip.h, "Syntax-element record"): {n_bins, two bypass code words or a
// context-coded unary run}, and bin `idx` of it as a bin record.  Shared by the binariser (cabac_binarize.hip) and the plan
// walk (cabac_plan_walk.h: the plan write and the plan resolve), which binarises the active elements of a plan the same way.
#ifndef CABAC_SE_CODE_H
#define CABAC_SE_CODE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cabac_hip.h"
#include "cabac_rem_abs.hpp"

namespace cabac {

struct SeCode {
  uint32_t n;           // number of bins
  uint32_t kind;        // CABAC_SE_*
  uint32_t code1, len1; // first bypass code word (MSB first)
  uint32_t code2, len2; // second bypass code word
  uint32_t a, b, c;     // kind-specific (ctx ids, symbol)
};

__device__ __forceinline__ uint32_t floor_log2_u32(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x | 1u); }

__device__ __forceinline__ SeCode se_decode(uint32_t w0, uint32_t value) {
  SeCode s;
  s.kind = w0 & 15u;
  s.n = 0;
  s.code1 = s.len1 = s.code2 = s.len2 = 0;
  s.a = s.b = s.c = 0;
  switch (s.kind) {
  case CABAC_SE_CTX_BIN:
    s.n = 1;
    s.a = (w0 >> 4) & 0x1ffu;
    s.b = value & 1u;
    break;
  case CABAC_SE_EP_BINS:
    s.len1 = (w0 >> 4) & 63u;
    s.code1 = value;
    s.n = s.len1;
    break;
  case CABAC_SE_REM_ABS: {  // arith_codec.cpp:426-458 (the code word: host/cabac_rem_abs.hpp)
    const cabac_code::RemAbsCode c = cabac_code::rem_abs_code(value, (w0 >> 4) & 31u, (w0 >> 9) & 31u, (w0 >> 14) & 63u);
    s.len1 = c.ones + c.stop;                    // the run and its separator as one field: ones, then a 0
    s.code1 = ((1u << c.ones) - 1u) << c.stop;   // (ones + stop <= 32: 1u << 32 does not occur, the longest run is 32 - maxLog2)
    s.len2 = c.tail_bits;
    s.code2 = c.tail;
    s.n = s.len1 + s.len2;
    break;
  }
  case CABAC_SE_TRM:
    s.n = 1;
    s.b = value & 1u;
    break;
  case CABAC_SE_UNARY_MAX: {  // cabac_writer.cpp:3072-3081
    s.a = (w0 >> 4) & 0x1ffu;
    s.b = (w0 >> 13) & 0x1ffu;
    const uint32_t mx = (w0 >> 22) & 0xffu;
    s.c = value;
    s.n = value + 1 < mx ? value + 1 : mx;
    break;
  }
  case CABAC_SE_UNARY_EP: {  // cabac_writer.cpp:3083-3101
    const uint32_t mx = (w0 >> 4) & 63u;
    if (mx != 0) {
      const uint32_t ones = value;  // `symbol` ones, then a zero if symbol < maxSymbol
      const uint32_t last = mx > value ? 1u : 0u;
      s.len1 = ones + last;
      s.code1 = (ones >= 32u ? 0xffffffffu : ((1u << ones) - 1u)) << last;
      s.n = s.len1;
    }
    break;
  }
  case CABAC_SE_EXP_GOLOMB: {  // cabac_writer.cpp:3103-3118
    uint32_t count = (w0 >> 4) & 31u, symbol = value, bins = 0, nb = 0;
    while (symbol >= (1u << count)) {
      bins = (bins << 1) + 1;
      nb++;
      symbol -= 1u << count;
      count++;
    }
    s.code1 = bins << 1;
    s.len1 = nb + 1;
    s.code2 = symbol;
    s.len2 = count;
    s.n = s.len1 + s.len2;
    break;
  }
  case CABAC_SE_TRUNC_BIN: {  // cabac_writer.cpp:854-882 (g_tbMax[k] == floor(log2 k))
    const uint32_t mx = w0 >> 4;
    const uint32_t thresh = floor_log2_u32(mx), val = 1u << thresh, b = mx - val;
    if (value < val - b) {
      s.code1 = value;
      s.len1 = thresh;
    } else {
      s.code1 = value + val - b;
      s.len1 = thresh + 1;
    }
    s.n = s.len1;
    break;
  }
  case CABAC_SE_ALIGN: s.n = 1; break;
  default: break;
  }
  return s;
}

__device__ __forceinline__ uint16_t se_bin(const SeCode &s, uint32_t idx) {
  switch (s.kind) {
  case CABAC_SE_CTX_BIN: return (uint16_t)(s.a | (s.b ? CABAC_REC_BIN : 0u));
  case CABAC_SE_TRM: return (uint16_t)(CABAC_REC_TRM | (s.b ? CABAC_REC_BIN : 0u));
  case CABAC_SE_ALIGN: return (uint16_t)CABAC_REC_ALIGN;
  case CABAC_SE_UNARY_MAX:
    return (uint16_t)((idx == 0 ? s.a : s.b) | ((s.c > idx) ? CABAC_REC_BIN : 0u));
  default: {  // one or two bypass code words, MSB first
    uint32_t bit;
    if (idx < s.len1) bit = (s.code1 >> (s.len1 - 1 - idx)) & 1u;
    else bit = (s.code2 >> (s.len2 - 1 - (idx - s.len1))) & 1u;
    return (uint16_t)(CABAC_REC_EP | (bit ? CABAC_REC_BIN : 0u));
  }
  }
}

}  // namespace cabac
#endif
