// Host check of the merge passes' chunk order (csrc/chunk_sort_hd.h): the bucket of every length
// 1..64 for every pass against tables written out by hand, and a scalar model of the kernel's
// counting sort (class_pass / chunk_sort in kernels.hip: strided ownership, one returning add per
// entry on the bucket's counter, the counters' exclusive scan, the scatter) whose walk must visit
// every entry once, the first min(E, SORTCAP) of them bucket-monotone in the chosen direction.
// Prints "ok" and exits 0, else says what differed.
//   build: g++ -O2 -std=c++17 -Wall chunk_sort_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/chunk_sort_hd.h"

namespace {

int g_bad = 0;

void fail(const std::string& what) {
  if (g_bad < 20) printf("%s\n", what.c_str());
  g_bad++;
}

std::string rep(char c, int n) { return std::string((size_t)n, c); }

// buckets of n = 1..64 as hex digits, by hand (lengths outside the class take the nearest bucket)
void check_tables() {
  struct Row {
    int N;
    bool exact;
    uint32_t buckets;
    std::string want;
  };
  const Row rows[] = {
      {8, false, 4, "00112233" + rep('3', 56)},
      {8, true, 4, "00000123" + rep('3', 56)},
      {16, false, 4, rep('0', 8) + "00112233" + rep('3', 48)},
      {16, true, 8, rep('0', 8) + "01234567" + rep('7', 48)},
      {32, false, 4, rep('0', 16) + "0000111122223333" + rep('3', 32)},
      {32, true, 16, rep('0', 16) + "0123456789abcdef" + rep('f', 32)},
      {64, false, 4, rep('0', 32) + "00000000111111112222222233333333"},
  };
  for (const Row& r : rows) {
    if (r.want.size() != 64) fail("table row of the wrong size");
    if (csort::n_buckets(r.N, r.exact) != r.buckets) fail("n_buckets N=" + std::to_string(r.N));
    for (uint32_t n = 1; n <= 64; n++) {
      const char c = r.want[n - 1];
      const uint32_t want = c <= '9' ? (uint32_t)(c - '0') : (uint32_t)(c - 'a' + 10);
      const uint32_t got = csort::bucket(r.N, r.exact, n);
      if (got != want)
        fail("bucket N=" + std::to_string(r.N) + " exact=" + std::to_string(r.exact) + " n=" + std::to_string(n) + ": " +
             std::to_string(got) + ", expected " + std::to_string(want));
    }
  }
  // the mode word: which rule a pass takes, and the walk direction in the code
  for (uint32_t mode = 0; mode <= csort::kModeMask; mode++) {
    const int Ns[] = {8, 16, 32, 64};
    for (int N : Ns) {
      const bool ex = N == 8 ? (mode & 1u) : N == 16 ? (mode & 2u) : N == 32 ? (mode & 4u) : false;
      if (csort::exact(N, mode) != ex) fail("exact N=" + std::to_string(N) + " mode=" + std::to_string(mode));
      if (csort::sorts(N, mode) != (N != 8 || ex)) fail("sorts N=" + std::to_string(N) + " mode=" + std::to_string(mode));
      const uint32_t nb = csort::n_buckets(N, ex);
      for (uint32_t n = 1; n <= 64; n++) {
        const uint32_t b = csort::bucket(N, ex, n);
        const uint32_t want = (mode & 8u) ? b : nb - 1 - b;
        const uint32_t c = csort::code(N, mode, n);
        if (c != want || c >= csort::kMaxBuckets) fail("code N=" + std::to_string(N) + " mode=" + std::to_string(mode));
      }
    }
  }
  if (csort::kModeDefault > csort::kModeMask) fail("default mode outside the mask");
}

uint32_t g_rng = 12345;
uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

// The kernel's sort on NT threads; the threads' adds land in an arbitrary order (here: the rounds in
// order, the threads of a round from a random start with a stride coprime to NT).  Returns Es.
uint32_t sort_model(const std::vector<uint32_t>& len, int N, uint32_t mode, uint32_t sortcap, uint32_t NT,
                    std::vector<uint16_t>& perm) {
  const uint32_t E = (uint32_t)len.size();
  perm.assign(sortcap, 0xFFFFu);
  if (!csort::sorts(N, mode)) return 0;
  const uint32_t Es = E < sortcap ? E : sortcap;
  const uint32_t G = 4, EPT = (sortcap + G * NT - 1) / (G * NT) * G;
  uint32_t bcnt[csort::kMaxBuckets] = {}, bfill[csort::kMaxBuckets];
  std::vector<uint32_t> cr((size_t)EPT * NT, 0);
  for (uint32_t j = 0; j < EPT; j++) {
    const uint32_t t0 = rnd() % NT;
    for (uint32_t k = 0; k < NT; k++) {
      const uint32_t tid = (t0 + k * 5u) % NT;  // (NT = 512, 768, 1024: coprime to 5)
      const uint32_t q = tid + j * NT;
      if (q >= Es) continue;
      const uint32_t c = csort::code(N, mode, len[q]);
      if (c >= csort::kMaxBuckets) {
        fail("code outside the counters");
        return Es;
      }
      cr[(size_t)j * NT + tid] = (c << 16) | bcnt[c]++;
    }
  }
  uint32_t acc = 0;
  for (uint32_t b = 0; b < csort::kMaxBuckets; b++) {
    bfill[b] = acc;
    acc += bcnt[b];
  }
  for (uint32_t j = 0; j < EPT; j++)
    for (uint32_t tid = 0; tid < NT; tid++) {
      const uint32_t q = tid + j * NT;
      if (q >= Es) continue;
      const uint32_t v = cr[(size_t)j * NT + tid], slot = bfill[v >> 16] + (v & 0xFFFFu);
      if (slot >= sortcap) {
        fail("slot outside perm");
        return Es;
      }
      perm[slot] = (uint16_t)q;
    }
  return Es;
}

void check_case(const char* what, const std::vector<uint32_t>& len, int N, uint32_t mode, uint32_t sortcap, uint32_t NT) {
  std::vector<uint16_t> perm;
  const uint32_t E = (uint32_t)len.size();
  const uint32_t Es = sort_model(len, N, mode, sortcap, NT, perm);
  const std::string id = std::string(what) + " N=" + std::to_string(N) + " mode=" + std::to_string(mode) +
                         " E=" + std::to_string(E) + " cap=" + std::to_string(sortcap) + " NT=" + std::to_string(NT);
  if (Es != (csort::sorts(N, mode) ? (E < sortcap ? E : sortcap) : 0u)) fail(id + ": Es");
  // the walk of class_pass: entry i is perm[i] below Es, i itself from there on
  std::vector<uint8_t> seen(E, 0);
  uint32_t prev = 0;
  for (uint32_t i = 0; i < E; i++) {
    const uint32_t q = i < Es ? perm[i] : i;
    if (q >= E || (i < Es && q >= Es) || seen[q]) {
      fail(id + ": walk position " + std::to_string(i) + " gives entry " + std::to_string(q));
      return;
    }
    seen[q] = 1;
    if (i < Es) {
      const uint32_t b = csort::bucket(N, csort::exact(N, mode), len[q]);
      if (i > 0 && ((mode & csort::kAscending) ? b < prev : b > prev)) {
        fail(id + ": bucket order broken at walk position " + std::to_string(i));
        return;
      }
      prev = b;
    }
  }
}

void check_sort() {
  struct Cfg {
    uint32_t sortcap, NT;
  };
  // the instances of kernels.hip: k_bpe_short folded and plain (narrow), wide; k_bpe_mid at 512 and 768
  const Cfg cfgs[] = {{6016, 1024}, {7168, 1024}, {8192, 1024}, {8192, 512}, {8192, 768}};
  const int Ns[] = {8, 16, 32};
  for (const Cfg& c : cfgs) {
    const uint32_t Es[] = {0, 1, 63, 64, 65, c.sortcap - 1, c.sortcap, c.sortcap + 1, 4 * c.sortcap};
    for (int N : Ns) {
      const uint32_t lo = csort::class_lo(N), hi = (uint32_t)N;
      for (uint32_t mode = 0; mode <= csort::kModeMask; mode++) {
        for (uint32_t E : Es) {
          std::vector<uint32_t> len(E);
          for (auto& n : len) n = lo + rnd() % (hi - lo + 1);
          check_case("random", len, N, mode, c.sortcap, c.NT);
          for (auto& n : len) n = hi;
          check_case("one bucket (longest)", len, N, mode, c.sortcap, c.NT);
          for (auto& n : len) n = lo;
          check_case("one bucket (shortest)", len, N, mode, c.sortcap, c.NT);
          for (uint32_t i = 0; i < E; i++) len[i] = (i & 1u) ? hi : lo;
          check_case("alternating extremes", len, N, mode, c.sortcap, c.NT);
        }
      }
    }
  }
}

}  // namespace

int main() {
  check_tables();
  check_sort();
  if (g_bad) {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
