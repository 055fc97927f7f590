// The sparse coefficient transport on the CPU (declared in include/cabac_hip_sparse.h): cabac_hip_sparse_pack_host and
// cabac_hip_sparse_unpack_host, the two walks of the header's DEFINITION OF THE RESULT written out.  No HIP include and no ctx:
// a plain C++ compiler builds this file alone (the sanitizer test does), and callers without a GPU can use it.
#include <cstdint>
#include <cstring>

#include "cabac_hip_sparse.h"

namespace {

struct Status {
  uint64_t n_entries = 0;
  uint32_t flags = 0, first_bad = CABAC_SPARSE_NO_BAD;
  void raise(uint32_t flag, uint32_t t) {
    flags |= flag;
    if (flag != CABAC_SPARSE_OVERFLOW && t < first_bad) first_bad = t;
  }
  void store(cabac_sparse_status *out) const { *out = cabac_sparse_status{n_entries, flags, first_bad}; }
};

// a good block: log2 sizes up to 6, inside the dense array
bool good_block(const cabac_tu_desc &d, uint64_t n_coeff_total) {
  if (d.log2_width > 6 || d.log2_height > 6) return false;
  const uint64_t n = uint64_t(1) << (d.log2_width + d.log2_height);
  return d.coeff_offset <= n_coeff_total && n <= n_coeff_total - d.coeff_offset;
}

template <class T>
void pack(uint32_t n_tu, const cabac_tu_desc *tus, const T *coeff, uint64_t n_coeff_total, uint32_t *ent_first, uint32_t *entries,
          uint64_t entry_capacity, Status &st) {
  uint64_t n = 0;
  for (uint32_t t = 0; t < n_tu; t++) {
    ent_first[t] = (uint32_t)n;
    if (!good_block(tus[t], n_coeff_total)) {
      st.raise(CABAC_SPARSE_BAD_BLOCK, t);
      continue;
    }
    const uint32_t w = 1u << tus[t].log2_width, h = 1u << tus[t].log2_height;
    const uint32_t cw = w < 32u ? w : 32u, ch = h < 32u ? h : 32u;
    const T *blk = coeff + tus[t].coeff_offset;
    for (uint32_t y = 0; y < ch; y++)
      for (uint32_t x = 0; x < cw; x++) {
        const T v = blk[y * w + x];
        if (v == 0) continue;
        if (sizeof(T) == 4 && (v < -32768 || v > 32767)) st.raise(CABAC_SPARSE_RANGE, t);
        if (n < entry_capacity) entries[n] = (y * w + x) | (uint32_t)(uint16_t)v << 16;
        n++;
      }
  }
  ent_first[n_tu] = (uint32_t)n;
  st.n_entries = n;
  if (n > entry_capacity) st.raise(CABAC_SPARSE_OVERFLOW, 0);
}

template <class T>
void unpack(uint32_t n_tu, const cabac_tu_desc *tus, const uint32_t *ent_first, const uint32_t *entries, uint64_t n_entries, T *coeff,
            uint64_t n_coeff_total, Status &st) {
  for (uint32_t t = 0; t < n_tu; t++) {
    if (!good_block(tus[t], n_coeff_total)) {
      st.raise(CABAC_SPARSE_BAD_BLOCK, t);
      continue;
    }
    const uint32_t n = 1u << (tus[t].log2_width + tus[t].log2_height);
    T *blk = coeff + tus[t].coeff_offset;
    std::memset(blk, 0, size_t(n) * sizeof(T));
    uint64_t lo = ent_first[t], hi = ent_first[t + 1];
    if (lo > hi) {  // descends: no entries
      st.raise(CABAC_SPARSE_BAD_FIRST, t);
      hi = lo;
    }
    if (hi > n_entries) {  // passes the list: clipped
      st.raise(CABAC_SPARSE_BAD_FIRST, t);
      hi = n_entries;
      if (lo > hi) lo = hi;
    }
    for (uint64_t k = lo; k < hi; k++) {
      const uint32_t pos = entries[k] & 0xFFFFu;
      if (pos >= n) st.raise(CABAC_SPARSE_BAD_POS, t);
      else blk[pos] = (T)(int16_t)(uint16_t)(entries[k] >> 16);
    }
  }
  st.n_entries = ent_first[n_tu] < n_entries ? ent_first[n_tu] : n_entries;
}

bool args_ok(int coeff_bytes, uint64_t n_coeff_total) { return (coeff_bytes == 2 || coeff_bytes == 4) && (n_coeff_total >> 32) == 0; }

}  // namespace

extern "C" {

int cabac_hip_sparse_pack_host(uint32_t n_tu, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                               uint32_t *ent_first, uint32_t *entries, uint64_t entry_capacity, cabac_sparse_status *status) {
  if (!status || !ent_first || (n_tu && !tus) || (n_coeff_total && !coeff) || (entry_capacity && !entries) ||
      !args_ok(coeff_bytes, n_coeff_total))
    return CABAC_HIP_ERR_INVALID;
  Status st;
  if (coeff_bytes == 2) pack(n_tu, tus, static_cast<const int16_t *>(coeff), n_coeff_total, ent_first, entries, entry_capacity, st);
  else pack(n_tu, tus, static_cast<const int32_t *>(coeff), n_coeff_total, ent_first, entries, entry_capacity, st);
  st.store(status);
  return CABAC_HIP_OK;
}

int cabac_hip_sparse_unpack_host(uint32_t n_tu, const cabac_tu_desc *tus, const uint32_t *ent_first, const uint32_t *entries,
                                 uint64_t n_entries, void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                                 cabac_sparse_status *status) {
  if (!status || !ent_first || (n_tu && !tus) || (n_coeff_total && !coeff) || (n_entries && !entries) ||
      !args_ok(coeff_bytes, n_coeff_total))
    return CABAC_HIP_ERR_INVALID;
  Status st;
  if (coeff_bytes == 2) unpack(n_tu, tus, ent_first, entries, n_entries, static_cast<int16_t *>(coeff), n_coeff_total, st);
  else unpack(n_tu, tus, ent_first, entries, n_entries, static_cast<int32_t *>(coeff), n_coeff_total, st);
  st.store(status);
  return CABAC_HIP_OK;
}

}  // extern "C"
