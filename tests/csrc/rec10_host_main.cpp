// Stand-alone driver for entropy_coding_amd/csrc/cabac_rec10_host.cpp under AddressSanitizer / UBSan (tests/test_rec10_host_san.py
// builds both with -fsanitize=address,undefined and runs this program as a child; nothing is preloaded).  Every buffer is a heap
// allocation of exactly the size the contract of include/cabac_hip_rec10.h asks for, so a read or write one element outside it
// aborts the run.  The cases are those of tests/test_rec10_model.py: the round trip R1 at the block edges, with cabac_rec10_put /
// cabac_rec10_get beside it, ranges of an unpack, a capacity that is short, and records with reserved bits.  Prints
// "rec10 host ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "cabac_hip_rec10.h"

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

uint16_t valid_record() { return (uint16_t)((rnd() & 0x1FFu) | (rnd() & 1u) << 15); }

void round_trip(uint64_t n) {
  g_case++;
  uint64_t bytes = 1;
  REQUIRE(cabac_hip_rec10_bytes(n, &bytes) == CABAC_HIP_OK && bytes == CABAC_REC10_BYTES(n) && bytes == (n + 63) / 64 * 80);
  Tight<uint16_t> rec(n), back(n);
  Tight<uint8_t> packed(bytes), built(bytes);
  for (uint64_t r = 0; r < n; r++) rec.p[r] = valid_record();
  std::memset(packed.p, 0xEE, bytes);
  uint64_t bad = 0;
  REQUIRE(cabac_hip_rec10_pack_host(rec.p, n, packed.p, bytes, &bad) == CABAC_HIP_OK && bad == UINT64_MAX);
  REQUIRE(cabac_hip_rec10_pack_host(rec.p, n, packed.p, bytes, nullptr) == CABAC_HIP_OK);
  for (uint64_t r = n; r < (n + 63) / 64 * 64; r++) REQUIRE(cabac_rec10_get(packed.p, r) == 0);  // the zero tail
  std::memset(back.p, 0x5A, n * sizeof(uint16_t));
  REQUIRE(cabac_hip_rec10_unpack_host(packed.p, 0, n, back.p) == CABAC_HIP_OK);
  REQUIRE(n == 0 || std::memcmp(rec.p, back.p, n * sizeof(uint16_t)) == 0);
  std::memset(built.p, 0, bytes);
  for (uint64_t r = n; r-- > 0;) cabac_rec10_put(built.p, r, rec.p[r]);
  REQUIRE(bytes == 0 || std::memcmp(built.p, packed.p, bytes) == 0);
  for (uint64_t r = 0; r < n; r++) REQUIRE(cabac_rec10_get(packed.p, r) == rec.p[r]);
  // ranges: records[first .. first + cnt) and nothing else
  const uint64_t firsts[] = {0, 1, 63, 65, n / 2 + 3};
  for (uint64_t first : firsts)
    for (uint64_t stop_short = 0; stop_short < 2; stop_short++) {
      if (first + stop_short > n) continue;
      const uint64_t cnt = n - first - stop_short;
      Tight<uint16_t> dst(first + cnt);  // ends with the last record written
      for (uint64_t r = 0; r < first; r++) dst.p[r] = 0xA5A5;
      REQUIRE(cabac_hip_rec10_unpack_host(packed.p, first, cnt, dst.p) == CABAC_HIP_OK);
      for (uint64_t r = 0; r < first; r++) REQUIRE(dst.p[r] == 0xA5A5);
      for (uint64_t r = first; r < first + cnt; r++) REQUIRE(dst.p[r] == rec.p[r]);
    }
}

void short_capacity(uint64_t n) {
  g_case++;
  const uint64_t bytes = CABAC_REC10_BYTES(n);
  Tight<uint16_t> rec(n);
  for (uint64_t r = 0; r < n; r++) rec.p[r] = valid_record();
  const uint64_t caps[] = {bytes - 1, bytes - 80, 0};
  for (uint64_t cap : caps) {
    Tight<uint8_t> packed(cap);  // exactly the capacity: a write behind it is a heap overflow
    std::memset(packed.p, 0x5E, cap);
    uint64_t bad = 0;
    REQUIRE(cabac_hip_rec10_pack_host(rec.p, n, packed.p, cap, &bad) == CABAC_HIP_ERR_INVALID && bad == UINT64_MAX);
    for (uint64_t i = 0; i < cap; i++) REQUIRE(packed.p[i] == 0x5E);
  }
}

void reserved_bits(uint64_t n, unsigned bit) {
  g_case++;
  const uint64_t bytes = CABAC_REC10_BYTES(n);
  Tight<uint16_t> rec(n), back(n);
  Tight<uint8_t> packed(bytes);
  for (uint64_t r = 0; r < n; r++) rec.p[r] = valid_record();
  const uint64_t spots[] = {0, 63, 64, n - 1};
  for (uint64_t a : spots)
    for (uint64_t b : spots) {
      if (a > b) continue;  // a == b: one bad record; a < b: two, the smaller index is reported
      const uint16_t keep_a = rec.p[a], keep_b = rec.p[b];
      rec.p[b] = (uint16_t)(rec.p[b] | 1u << (23 - bit));
      rec.p[a] = (uint16_t)(rec.p[a] | 1u << bit);
      uint64_t bad = 0;
      REQUIRE(cabac_hip_rec10_pack_host(rec.p, n, packed.p, bytes, &bad) == CABAC_HIP_ERR_INVALID && bad == a);
      rec.p[b] = keep_b;
      rec.p[a] = keep_a;
      // the output holds the records with the bits dropped
      REQUIRE(cabac_hip_rec10_unpack_host(packed.p, 0, n, back.p) == CABAC_HIP_OK && std::memcmp(rec.p, back.p, n * sizeof(uint16_t)) == 0);
    }
}

void arbitrary_bytes() {  // every 80-byte pattern is a block of 64 records with clear reserved bits, and packs back to itself
  g_case++;
  const uint64_t n = 64 * 5, bytes = CABAC_REC10_BYTES(n);
  Tight<uint8_t> raw(bytes), again(bytes);
  Tight<uint16_t> rec(n);
  for (uint64_t i = 0; i < bytes; i++) raw.p[i] = (uint8_t)rnd();
  REQUIRE(cabac_hip_rec10_unpack_host(raw.p, 0, n, rec.p) == CABAC_HIP_OK);
  for (uint64_t r = 0; r < n; r++) REQUIRE((rec.p[r] & CABAC_REC10_RESERVED_BITS) == 0);
  uint64_t bad = 0;
  REQUIRE(cabac_hip_rec10_pack_host(rec.p, n, again.p, bytes, &bad) == CABAC_HIP_OK && std::memcmp(raw.p, again.p, bytes) == 0);
}

void nulls() {
  g_case++;
  uint64_t bad = 0;
  uint8_t byte = 0;
  uint16_t rec = 0;
  REQUIRE(cabac_hip_rec10_bytes(1, nullptr) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_pack_host(nullptr, 1, &byte, 80, &bad) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_pack_host(&rec, 1, nullptr, 80, &bad) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_unpack_host(nullptr, 0, 1, &rec) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_unpack_host(&byte, 0, 1, nullptr) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_unpack_host(&byte, UINT64_MAX, 2, &rec) == CABAC_HIP_ERR_INVALID);
  REQUIRE(cabac_hip_rec10_pack_host(nullptr, 0, nullptr, 0, &bad) == CABAC_HIP_OK && bad == UINT64_MAX);
  REQUIRE(cabac_hip_rec10_unpack_host(nullptr, 7, 0, nullptr) == CABAC_HIP_OK);
}

}  // namespace

int main() {
  const uint64_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 4097};
  for (uint64_t n : sizes) round_trip(n);
  for (uint64_t n : {uint64_t(1), uint64_t(64), uint64_t(65), uint64_t(4097)}) short_capacity(n);
  for (unsigned bit : {9u, 14u})
    for (uint64_t n : {uint64_t(65), uint64_t(4097)}) reserved_bits(n, bit);
  arbitrary_bytes();
  nulls();
  std::printf("rec10 host ok\n");
  return 0;
}
