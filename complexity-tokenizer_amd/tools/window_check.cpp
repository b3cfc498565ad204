// Host check of the stride-window arithmetic (csrc/window_hd.h): the window count of a row from
// (P, max_length, stride) and the bounds of window k.  The expected values are written out by hand
// from the reference's loop (src/encoding.rs:175-223), not computed through the header.  Prints
// "ok" and exits 0, else says what differed.
//   build: g++ -O2 -std=c++17 -Wall window_check.cpp
#include <cstdint>
#include <cstdio>

#include "../csrc/window_hd.h"

namespace {

int g_bad = 0;

void eq(const char* what, const char* field, uint64_t got, uint64_t want) {
  if (got == want) return;
  printf("%s: %s = %llu, expected %llu\n", what, field, (unsigned long long)got, (unsigned long long)want);
  g_bad++;
}

void count(const char* what, uint64_t P, uint64_t m, uint64_t s, uint64_t want) {
  eq(what, "count", win::count(P, m, s), want);
}

void window(const char* what, uint64_t k, uint64_t P, uint64_t m, uint64_t s, uint64_t start, uint64_t end) {
  eq(what, "start", win::start(k, m, s), start);
  eq(what, "end", win::end(k, P, m, s), end);
}

void check_valid() {
  eq("m 1 s 0", "valid", win::valid(1, 0), 1);
  eq("m 8 s 7", "valid", win::valid(8, 7), 1);
  eq("m 8 s 8", "valid", win::valid(8, 8), 0);
  eq("m 8 s 9", "valid", win::valid(8, 9), 0);
  eq("m 0 s 0", "valid", win::valid(0, 0), 0);
}

void check_small() {
  // m = 8, s = 3: windows advance by 5
  count("m8 s3 P0", 0, 8, 3, 1);
  window("m8 s3 P0 w0", 0, 0, 8, 3, 0, 0);
  count("m8 s3 P7", 7, 8, 3, 1);
  window("m8 s3 P7 w0", 0, 7, 8, 3, 0, 7);
  count("m8 s3 P8", 8, 8, 3, 1);
  window("m8 s3 P8 w0", 0, 8, 8, 3, 0, 8);
  count("m8 s3 P9", 9, 8, 3, 2);
  window("m8 s3 P9 w0", 0, 9, 8, 3, 0, 8);
  window("m8 s3 P9 w1", 1, 9, 8, 3, 5, 9);
  // P - m an exact multiple of m - s, and one more
  count("m8 s3 P13", 13, 8, 3, 2);
  window("m8 s3 P13 w1", 1, 13, 8, 3, 5, 13);
  count("m8 s3 P14", 14, 8, 3, 3);
  window("m8 s3 P14 w1", 1, 14, 8, 3, 5, 13);
  window("m8 s3 P14 w2", 2, 14, 8, 3, 10, 14);
  count("m8 s3 P18", 18, 8, 3, 3);
  count("m8 s3 P19", 19, 8, 3, 4);
  window("m8 s3 P19 w3", 3, 19, 8, 3, 15, 19);
  // s = 0: plain chunks
  count("m4 s0 P3", 3, 4, 0, 1);
  count("m4 s0 P4", 4, 4, 0, 1);
  count("m4 s0 P5", 5, 4, 0, 2);
  window("m4 s0 P5 w1", 1, 5, 4, 0, 4, 5);
  count("m4 s0 P8", 8, 4, 0, 2);
  window("m4 s0 P8 w1", 1, 8, 4, 0, 4, 8);
  count("m4 s0 P9", 9, 4, 0, 3);
  window("m4 s0 P9 w2", 2, 9, 4, 0, 8, 9);
  count("m4 s0 P12", 12, 4, 0, 3);
  // s = m - 1: windows advance by one
  count("m4 s3 P4", 4, 4, 3, 1);
  count("m4 s3 P5", 5, 4, 3, 2);
  window("m4 s3 P5 w1", 1, 5, 4, 3, 1, 5);
  count("m4 s3 P10", 10, 4, 3, 7);
  window("m4 s3 P10 w6", 6, 10, 4, 3, 6, 10);
  // m = 1 (s = 0 = m - 1)
  count("m1 s0 P0", 0, 1, 0, 1);
  count("m1 s0 P1", 1, 1, 0, 1);
  count("m1 s0 P2", 2, 1, 0, 2);
  count("m1 s0 P5", 5, 1, 0, 5);
  window("m1 s0 P5 w4", 4, 5, 1, 0, 4, 5);
}

void check_large() {
  // P = 2^32, m = 512, s = 128: P - m = 384 * 11184809 + 128
  count("P 2^32 m512 s128", 4294967296ull, 512, 128, 11184811ull);
  window("P 2^32 m512 s128 last", 11184810ull, 4294967296ull, 512, 128, 4294967040ull, 4294967296ull);
  window("P 2^32 m512 s128 last but one", 11184809ull, 4294967296ull, 512, 128, 4294966656ull, 4294967168ull);
  // more windows than 2^32: the count needs 64 bits
  count("P 2^32+15 m2 s1", 4294967311ull, 2, 1, 4294967310ull);
  window("P 2^32+15 m2 s1 last", 4294967309ull, 4294967311ull, 2, 1, 4294967309ull, 4294967311ull);
  // k * (m - s) past 2^32 with both factors below it: P = 16 * 2^32 + 16 (a 16-item template over
  // 2^32 ids), m = 2^32 - 1, s = 0: P - m = 15 * m + 32
  count("P 16*2^32+16 m 2^32-1", 68719476752ull, 4294967295ull, 0, 17);
  window("P 16*2^32+16 m 2^32-1 w16", 16, 68719476752ull, 4294967295ull, 0, 68719476720ull, 68719476752ull);
  window("P 16*2^32+16 m 2^32-1 w15", 15, 68719476752ull, 4294967295ull, 0, 64424509425ull, 68719476720ull);
  // P just around m near 2^32
  count("P m-1 near 2^32", 4294967294ull, 4294967295ull, 7, 1);
  count("P m near 2^32", 4294967295ull, 4294967295ull, 7, 1);
  count("P m+1 near 2^32", 4294967296ull, 4294967295ull, 7, 2);
  window("P m+1 near 2^32 w1", 1, 4294967296ull, 4294967295ull, 7, 4294967288ull, 4294967296ull);
}

}  // namespace

int main() {
  check_valid();
  check_small();
  check_large();
  if (g_bad) {
    printf("%d mismatches\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
