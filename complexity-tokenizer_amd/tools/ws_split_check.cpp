// CPU check of csrc/ws_split_hd.h (the whitespace split of the classic BPE trainer's k_ws_bits):
// its run starts against a split on the explicit set of the 25 White_Space code points, made on
// decoded code points.  Build: g++ -O2 -std=c++17 ws_split_check.cpp -o ws_split_check; prints
// "ok" or the first difference.
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../csrc/ws_split_hd.h"

static const uint32_t kWs[25] = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2000, 0x2001, 0x2002, 0x2003,
                                 0x2004, 0x2005, 0x2006, 0x2007, 0x2008, 0x2009, 0x200A, 0x2028, 0x2029, 0x202F, 0x205F,
                                 0x3000};

static std::string utf8(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) { s += (char)(0xC0 | (c >> 6)); s += (char)(0x80 | (c & 63)); }
  else if (c < 0x10000) { s += (char)(0xE0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  else { s += (char)(0xF0 | (c >> 18)); s += (char)(0x80 | ((c >> 12) & 63)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  return s;
}

static std::string join(const std::vector<uint32_t>& cps) {
  std::string s;
  for (uint32_t c : cps) s += utf8(c);
  return s;
}

// the byte offsets at which a run of whitespace or of non-whitespace starts, from the code points
static std::vector<uint64_t> want_starts(const std::vector<uint32_t>& cps) {
  static const std::set<uint32_t> ws(kWs, kWs + 25);
  std::vector<uint64_t> out;
  uint64_t pos = 0;
  bool prev = false;
  for (size_t i = 0; i < cps.size(); i++) {
    const bool w = ws.count(cps[i]) != 0;
    if (i == 0 || w != prev) out.push_back(pos);
    prev = w;
    pos += utf8(cps[i]).size();
  }
  return out;
}

static int n_checked = 0;

static bool check(const std::vector<uint32_t>& cps, const char* what) {
  const std::string s = join(cps);
  const uint64_t n = s.size();
  const std::vector<uint64_t> want = want_starts(cps);
  // the functions may read no byte at or past n: whatever follows must not change the answer
  for (uint8_t fill : {0x20, 0x80, 0xA0, 0x61}) {
    std::vector<uint8_t> buf(s.begin(), s.end());
    buf.resize(n + 40, fill);
    std::vector<uint64_t> got, got_bits;
    for (uint64_t g = 0; g < n; g++)
      if (wsplit::run_start(buf.data(), n, g)) got.push_back(g);
    for (uint64_t w = 0; w < (n + 31) / 32 + 1; w++) {
      const uint32_t v = wsplit::run_start_bits(buf.data(), n, w);
      for (uint32_t j = 0; j < 32; j++)
        if ((v >> j) & 1u) got_bits.push_back(w * 32 + j);
    }
    if (got != want || got_bits != want) {
      printf("FAIL %s (fill %02x): text", what, fill);
      for (unsigned char c : s) printf(" %02x", c);
      printf("\n want");
      for (uint64_t x : want) printf(" %llu", (unsigned long long)x);
      printf("\n got ");
      for (uint64_t x : got) printf(" %llu", (unsigned long long)x);
      printf("\n bits");
      for (uint64_t x : got_bits) printf(" %llu", (unsigned long long)x);
      printf("\n");
      return false;
    }
  }
  n_checked++;
  return true;
}

int main() {
  // every one of the 25 between letters, and alone: ws_at on each
  for (uint32_t w : kWs) {
    if (!check({'a', 'b', w, 'c', 'd'}, "a space between letters")) return 1;
    const std::string s = utf8(w);
    if (!wsplit::ws_at((const uint8_t*)s.data(), s.size(), 0)) {
      printf("FAIL ws_at(U+%04X)\n", w);
      return 1;
    }
    if (want_starts({'a', 'b', w, 'c', 'd'}).size() != 3) return 1;
  }
  // not White_Space: the separators Python's str.split also splits on, and ZERO WIDTH SPACE
  for (uint32_t c : {0x1Cu, 0x1Du, 0x1Eu, 0x1Fu, 0x200Bu, 0x180Eu, 0x2060u, 0xFEFFu, 0x84u, 0x86u, 0x200Cu, 0x2027u, 0x3001u}) {
    if (!check({'a', c, 'b'}, "not a space")) return 1;
    if (want_starts({'a', c, 'b'}).size() != 1) return 1;
  }
  // 2-, 3- and 4-byte letters next to 1-, 2- and 3-byte spaces
  for (uint32_t l : {0xE9u, 0x65E5u, 0x1F600u, 0x61u})
    for (uint32_t w : {0x20u, 0xA0u, 0x85u, 0x3000u, 0x1680u, 0x2028u})
      for (uint32_t l2 : {0xE9u, 0x65E5u, 0x1F600u, 0x61u})
        if (!check({l, w, l2, l, w, w, l2}, "multi-byte letters and spaces")) return 1;
  // empty, all-space, no space
  if (!check({}, "empty")) return 1;
  if (!check({0x20, 0x3000, 0x0A, 0xA0}, "all spaces")) return 1;
  if (!check({'x'}, "one letter")) return 1;
  if (!check({0x1F600, 0x1F600}, "two 4-byte letters")) return 1;
  // seeded random strings over a 40-symbol alphabet that holds all 25 (lengths cross the 32-byte words)
  std::vector<uint32_t> alpha(kWs, kWs + 25);
  for (uint32_t c : {0x61u, 0x62u, 0x7Au, 0x1Cu, 0x1Fu, 0xE9u, 0xC2u, 0x200Bu, 0x2010u, 0x205Eu, 0x3001u, 0x65E5u, 0x1F600u, 0x10FFFFu, 0x80u})
    alpha.push_back(c);
  if (alpha.size() != 40) return 1;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&] {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  for (int it = 0; it < 4000; it++) {
    std::vector<uint32_t> cps(next() % 60);
    for (auto& c : cps) c = alpha[next() % (it % 3 == 0 ? 40 : 28)];  // (two thirds: mostly spaces and a few letters)
    if (!check(cps, "random")) return 1;
  }
  if (n_checked < 4000) return 1;
  printf("ok\n");
  return 0;
}
