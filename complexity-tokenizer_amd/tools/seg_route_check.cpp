// Host-side check of the small pure functions behind k_segment's mask phase and its doc-start
// bits (csrc/seg_lane.h pack8*, csrc/seg_route_hd.h), each against the expression it replaced or
// the definition it implements.  A stand-alone program: prints one line per part, exits non-zero on
// the first difference.  Built and run by tests/test_seg_route_cpu.py (also under
// -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/seg_lane.h"
#include "../csrc/seg_route_hd.h"

namespace {

std::mt19937_64 rng(20240611);
uint32_t r32() { return (uint32_t)rng(); }

// ---- the forms that were replaced
uint32_t pack8_mul(uint32_t r0, uint32_t r1) {  // one 32x32->64 high multiply
  const uint32_t c = ((r0 & seg::kHi) >> 4) | (r1 & seg::kHi);
  return (uint32_t)(((uint64_t)c * 0x20408100u) >> 32) & 0xFFu;
}
int fail(const char* what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
  printf("FAIL %s: (%llx, %llx) got %llx want %llx\n", what, (unsigned long long)a, (unsigned long long)b,
         (unsigned long long)got, (unsigned long long)want);
  return 1;
}

// all 256 flag patterns (bits 0..3: the bit 7 of r0's bytes, bits 4..7: of r1's); the other 7 bits
// of every byte zero, all ones, and 1,000 random fills
int check_pack8() {
  uint64_t cases = 0;
  for (int fill = 0; fill < 1002; fill++) {
    for (uint32_t f = 0; f < 256; f++) {
      uint32_t r0 = 0, r1 = 0;
      for (int k = 0; k < 4; k++) {
        r0 |= ((f >> k) & 1u) << (8 * k + 7);
        r1 |= ((f >> (4 + k)) & 1u) << (8 * k + 7);
      }
      r0 |= fill == 0 ? 0u : fill == 1 ? 0x7F7F7F7Fu : r32() & 0x7F7F7F7Fu;
      r1 |= fill == 0 ? 0u : fill == 1 ? 0x7F7F7F7Fu : r32() & 0x7F7F7F7Fu;
      const uint32_t want = pack8_mul(r0, r1);
      if (want != f) return fail("pack8_mul itself", r0, r1, want, f);
      const uint32_t got = seg::pack8(r0, r1);
      if (got != want) return fail("pack8", r0, r1, got, want);
      if (seg::pack8_hi(r0, r1) & 0x7Fu) return fail("pack8_hi low bits", r0, r1, seg::pack8_hi(r0, r1), 0);
      for (int sh = 0; sh < 32; sh += 8)
        if (seg::pack8_at(r0, r1, sh) != want << sh) return fail("pack8_at", r0, r1, seg::pack8_at(r0, r1, sh), want << sh);
      cases++;
    }
  }
  // the dot product's host twin on arbitrary operands, against 64-bit arithmetic
  for (int i = 0; i < 100000; i++) {
    const uint32_t a = r32(), b = r32(), c = r32();
    uint64_t want = c;
    for (int k = 0; k < 4; k++) want += (uint64_t)((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
    if (seg::dot4(a, b, c) != (uint32_t)want) return fail("dot4", a, b, seg::dot4(a, b, c), (uint32_t)want);
  }
  printf("pack8 ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}

// doc-start bits by piece number against the per-piece definition: bit j = piece j's start is a
// doc start
int check_doc_word(uint64_t st, uint64_t D, uint32_t prew) {
  std::vector<uint32_t> got(4096 / 32 + 4, 0), want(4096 / 32 + 4, 0);
  seg::doc_pieces(st, D, prew, [&](uint32_t j) { got.at(j >> 5) |= 1u << (j & 31); });
  uint32_t j = prew;
  for (int b = 0; b < 64; b++) {
    if (!((st >> b) & 1)) continue;
    if ((D >> b) & 1) want.at(j >> 5) |= 1u << (j & 31);
    j++;
  }
  if (got != want) return fail("doc_pieces", st, D, prew, 0);
  return 0;
}
int check_doc() {
  uint64_t cases = 0;
  const uint32_t prews[] = {0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 1000, 3968 - 64};
  for (uint32_t prew : prews) {
    const uint64_t fixed[][2] = {
        {0ull, 0ull},                                    // a word with no start
        {0ull, ~0ull},                                   // (doc bits where no piece starts do not count)
        {~0ull, ~0ull}, {~0ull, 0ull}, {~0ull, 1ull},    // 64 starts
        {~0ull, 1ull << 63}, {~0ull, 1ull | 1ull << 63},
        {1ull, 1ull}, {1ull << 63, 1ull << 63}, {1ull | 1ull << 63, 1ull | 1ull << 63},  // doc starts at bits 0 and 63
        {0x8000000080000001ull, 0x8000000000000001ull},
    };
    for (const auto& f : fixed) {
      if (check_doc_word(f[0], f[1], prew)) return 1;
      cases++;
    }
    // ordinals landing on 31 / 32 and 63 / 64 / 65: k starts below the doc start
    for (uint32_t target : {31u, 32u, 63u, 64u, 65u}) {
      if (target < prew || target - prew > 63) continue;
      const uint32_t k = target - prew;
      const uint64_t st = k == 63 ? ~0ull : (1ull << (k + 1)) - 1;
      if (check_doc_word(st, 1ull << k, prew)) return 1;
      if (check_doc_word(st, st, prew)) return 1;
      cases += 2;
    }
    for (int i = 0; i < 20000; i++) {
      uint64_t st = rng();
      if (i & 1) st &= rng() & rng();  // sparser words
      uint64_t D = st & rng();
      if (i & 2) D &= rng() & rng();
      if (i % 7 == 0) D = rng();  // (not a subset: only D & st may count)
      if (check_doc_word(st, D, prew)) return 1;
      cases++;
    }
  }
  printf("doc bits ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}

}  // namespace

int main() {
  if (check_pack8() || check_doc()) return 1;
  printf("all ok\n");
  return 0;
}
