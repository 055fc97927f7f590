// Stand-alone driver for entropy_coding_amd/csrc/cabac_sparse_host.cpp under AddressSanitizer / UBSan (tests/test_sparse_host_san.py
// builds both with -fsanitize=address,undefined and runs this program as a child; nothing is preloaded).  Every buffer is a heap
// allocation of exactly the size the contract of include/cabac_hip_sparse.h asks for, so a read or write one element outside it
// aborts the run.  The cases are the edges of tests/test_sparse_model.py; results are checked by the round trip (S2) and by the
// status word.  Prints "sparse host ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cabac_hip_sparse.h"

namespace {

int g_case = 0;
#define REQUIRE(cond)                                                            \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "case %d: %s (line %d)\n", g_case, #cond, __LINE__); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

template <class T>
struct Tight {  // exactly n elements on the heap (at least one byte, so that the pointer is never null)
  T *p;
  size_t n;
  explicit Tight(size_t count) : p(static_cast<T *>(std::malloc(count ? count * sizeof(T) : 1))), n(count) {}
  ~Tight() { std::free(p); }
  Tight(const Tight &) = delete;
  Tight &operator=(const Tight &) = delete;
};

struct Shape {
  uint8_t lw, lh;
};

// the blocks laid out with `gap` spare elements in front of each, the first at `start`
size_t lay(const std::vector<Shape> &shapes, size_t start, size_t gap, cabac_tu_desc *tus) {
  size_t at = start;
  for (size_t t = 0; t < shapes.size(); t++) {
    at += gap;
    std::memset(&tus[t], 0, sizeof tus[t]);
    tus[t].coeff_offset = at;
    tus[t].log2_width = shapes[t].lw;
    tus[t].log2_height = shapes[t].lh;
    at += size_t(1) << (shapes[t].lw + shapes[t].lh);
  }
  return at;
}

template <class T>
void round_trip(const std::vector<Shape> &shapes, size_t start, size_t gap, uint32_t density_percent) {
  g_case++;
  Tight<cabac_tu_desc> tus(shapes.size());
  const size_t n_total = lay(shapes, start, gap, tus.p);
  Tight<T> coeff(n_total), back(n_total);
  const T sentinel = (T)0x5A5A;
  uint64_t want = 0;
  for (size_t i = 0; i < n_total; i++) coeff.p[i] = back.p[i] = sentinel;
  for (size_t t = 0; t < shapes.size(); t++) {
    const uint32_t w = 1u << shapes[t].lw, h = 1u << shapes[t].lh;
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) {
        T v = 0;
        if (x >= 32 || y >= 32) v = 7;  // junk outside the coded region
        else if (rnd() % 100 < density_percent) v = (T)((int)(rnd() % 65536) - 32768);
        coeff.p[tus.p[t].coeff_offset + y * w + x] = v;
        want += (x < 32 && y < 32 && v != 0);
      }
  }
  Tight<uint32_t> first(shapes.size() + 1);
  cabac_sparse_status st;
  // capacity 0 and need - 1: the full count is reported, nothing is written past the capacity
  {
    Tight<uint32_t> none(0);
    REQUIRE(cabac_hip_sparse_pack_host((uint32_t)shapes.size(), tus.p, coeff.p, sizeof(T), n_total, first.p, none.p, 0, &st) == CABAC_HIP_OK);
    REQUIRE(st.n_entries == want && (st.flags == (want ? CABAC_SPARSE_OVERFLOW : 0u)) && first.p[shapes.size()] == want);
  }
  if (want > 1) {
    Tight<uint32_t> less(want - 1);
    REQUIRE(cabac_hip_sparse_pack_host((uint32_t)shapes.size(), tus.p, coeff.p, sizeof(T), n_total, first.p, less.p, want - 1, &st) == CABAC_HIP_OK);
    REQUIRE(st.n_entries == want && st.flags == CABAC_SPARSE_OVERFLOW);
  }
  Tight<uint32_t> ent(want);
  REQUIRE(cabac_hip_sparse_pack_host((uint32_t)shapes.size(), tus.p, coeff.p, sizeof(T), n_total, first.p, ent.p, want, &st) == CABAC_HIP_OK);
  REQUIRE(st.n_entries == want && st.flags == 0 && st.first_bad == CABAC_SPARSE_NO_BAD && first.p[0] == 0);
  REQUIRE(cabac_hip_sparse_unpack_host((uint32_t)shapes.size(), tus.p, first.p, ent.p, want, back.p, sizeof(T), n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.n_entries == want && st.flags == 0 && st.first_bad == CABAC_SPARSE_NO_BAD);
  // S2: the coded region reproduced, the rest of the block zero, the gaps untouched
  std::vector<uint8_t> inside(n_total, 0);
  for (size_t t = 0; t < shapes.size(); t++) {
    const uint32_t w = 1u << shapes[t].lw, h = 1u << shapes[t].lh;
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) {
        const size_t i = tus.p[t].coeff_offset + y * w + x;
        inside[i] = 1;
        REQUIRE(back.p[i] == ((x < 32 && y < 32) ? coeff.p[i] : (T)0));
      }
  }
  for (size_t i = 0; i < n_total; i++) REQUIRE(inside[i] || back.p[i] == sentinel);
}

void bad_inputs() {
  g_case++;
  const std::vector<Shape> shapes = {{2, 2}, {2, 2}, {2, 2}, {2, 2}};
  Tight<cabac_tu_desc> tus(shapes.size());
  const size_t n_total = lay(shapes, 0, 0, tus.p);
  Tight<int16_t> coeff(n_total);
  for (size_t i = 0; i < n_total; i++) coeff.p[i] = (int16_t)(i % 3 ? 0 : 1 + (int)i);
  Tight<uint32_t> first(shapes.size() + 1), ent(n_total);
  cabac_sparse_status st;
  REQUIRE(cabac_hip_sparse_pack_host(4, tus.p, coeff.p, 2, n_total, first.p, ent.p, n_total, &st) == CABAC_HIP_OK && st.flags == 0);
  const uint64_t n = st.n_entries;
  // BAD_POS: the entry is dropped, nothing is written outside the block
  const uint32_t keep = ent.p[first.p[2]];
  ent.p[first.p[2]] = (keep & 0xFFFF0000u) | 0xFFFFu;
  REQUIRE(cabac_hip_sparse_unpack_host(4, tus.p, first.p, ent.p, n, coeff.p, 2, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_BAD_POS && st.first_bad == 2);
  ent.p[first.p[2]] = keep;
  // BAD_FIRST: a first beyond the list must not be followed; a descending pair has no entries
  const uint32_t f3 = first.p[3];
  first.p[3] = 0xFFFFFFF0u;
  REQUIRE(cabac_hip_sparse_unpack_host(4, tus.p, first.p, ent.p, n, coeff.p, 2, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_BAD_FIRST && st.first_bad == 2);
  first.p[3] = f3;
  {
    Tight<uint32_t> shorter(n - 1);  // the list one entry shorter than the firsts say
    std::memcpy(shorter.p, ent.p, (n - 1) * sizeof(uint32_t));
    REQUIRE(cabac_hip_sparse_unpack_host(4, tus.p, first.p, shorter.p, n - 1, coeff.p, 2, n_total, &st) == CABAC_HIP_OK);
    REQUIRE(st.flags == CABAC_SPARSE_BAD_FIRST && st.first_bad == 3 && st.n_entries == n - 1);
  }
  // BAD_BLOCK: a size the format does not have, and a block that passes the end of the array: neither is read nor written
  tus.p[1].log2_height = 7;
  tus.p[3].coeff_offset = n_total - 15;
  REQUIRE(cabac_hip_sparse_pack_host(4, tus.p, coeff.p, 2, n_total, first.p, ent.p, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_BAD_BLOCK && st.first_bad == 1 && first.p[1] == first.p[2] && first.p[3] == first.p[4]);
  REQUIRE(cabac_hip_sparse_unpack_host(4, tus.p, first.p, ent.p, st.n_entries, coeff.p, 2, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_BAD_BLOCK && st.first_bad == 1);
  tus.p[3].coeff_offset = ~0ull - 3;  // offset + size wraps
  REQUIRE(cabac_hip_sparse_pack_host(4, tus.p, coeff.p, 2, n_total, first.p, ent.p, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_BAD_BLOCK);
  // RANGE from 32-bit blocks
  Tight<int32_t> wide(16);
  std::memset(wide.p, 0, 16 * sizeof(int32_t));
  wide.p[15] = 40000;
  wide.p[0] = -32768;
  REQUIRE(cabac_hip_sparse_pack_host(1, tus.p, wide.p, 4, 16, first.p, ent.p, n_total, &st) == CABAC_HIP_OK);
  REQUIRE(st.flags == CABAC_SPARSE_RANGE && st.first_bad == 0 && st.n_entries == 2 && ent.p[1] == (15u | (40000u & 0xFFFFu) << 16));
  // refusals
  REQUIRE(cabac_hip_sparse_pack_host(1, tus.p, wide.p, 3, 16, first.p, ent.p, n_total, &st) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_sparse_pack_host(1, tus.p, wide.p, 4, 1ull << 32, first.p, ent.p, n_total, &st) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_sparse_unpack_host(1, tus.p, first.p, ent.p, 0, wide.p, 4, 16, nullptr) == CABAC_HIP_ERR_INVALID);
  // no block at all
  REQUIRE(cabac_hip_sparse_pack_host(0, nullptr, nullptr, 2, 0, first.p, nullptr, 0, &st) == CABAC_HIP_OK);
  REQUIRE(st.n_entries == 0 && st.flags == 0 && first.p[0] == 0);
}

}  // namespace

int main() {
  std::vector<Shape> all;
  for (uint8_t lw = 0; lw <= 6; lw++)
    for (uint8_t lh = 0; lh <= 6; lh++) all.push_back({lw, lh});
  for (uint32_t density : {0u, 5u, 100u}) {
    round_trip<int16_t>(all, 0, 0, density);
    round_trip<int32_t>(all, 0, 0, density);
    round_trip<int16_t>(all, 1, 3, density);  // odd offsets, gaps
    round_trip<int32_t>(all, 1, 1, density);
  }
  round_trip<int16_t>({{0, 1}}, 1, 0, 100);  // 1 x 2 at an odd offset, alone in its array
  round_trip<int16_t>({{1, 1}, {0, 0}}, 1, 0, 100);
  round_trip<int16_t>({}, 0, 0, 0);
  bad_inputs();
  std::printf("sparse host ok\n");
  return 0;
}
