// CPU check of csrc/wp_table_hd.h (the string table behind wordpiece.hip's k_wp_match): builds
// tables and probes every pattern in both forms, near misses (a byte short, a byte more, the other
// form, one byte changed), the longest match at a position against a brute-force search, the word
// bound, and build()'s refusals.  Build: g++ -O2 -std=c++17 wp_table_check.cpp -o wp_table_check;
// prints "ok" or the first difference.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../csrc/wp_table_hd.h"

using namespace wptab;

static int fail(const char* what, const std::string& s = "") {
  printf("FAIL %s %s\n", what, s.c_str());
  return 1;
}

static uint32_t probe(const View& v, const std::string& s, uint32_t form) {
  return find(v, (const uint8_t*)s.data(), (uint32_t)s.size(), hash_of((const uint8_t*)s.data(), (uint32_t)s.size()), form);
}

static std::string utf8(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) { s += (char)(0xC0 | (c >> 6)); s += (char)(0x80 | (c & 63)); }
  else if (c < 0x10000) { s += (char)(0xE0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  else { s += (char)(0xF0 | (c >> 18)); s += (char)(0x80 | ((c >> 12) & 63)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  return s;
}

int main() {
  std::mt19937 rng(12345);
  const uint32_t alphabet[] = {'a', 'b', 'c', '#', 0xE9, 0x3C3, 0x4E2D, 0x1F600};
  for (int round = 0; round < 40; round++) {
    // distinct (form, bytes) patterns over a small alphabet, so that near misses are frequent
    std::map<std::pair<uint32_t, std::string>, uint32_t> want;
    const int n = round < 4 ? round : 1 << (round % 12);
    while ((int)want.size() < n) {
      std::string s;
      const int len = 1 + rng() % (round % 3 == 0 ? 12 : 4);
      for (int i = 0; i < len; i++) s += utf8(alphabet[rng() % 8]);
      want.emplace(std::make_pair(rng() % 2, s), (uint32_t)want.size() + 7);
    }
    std::vector<Pattern> pats;
    for (const auto& kv : want)
      pats.push_back(Pattern{(const uint8_t*)kv.first.second.data(), (uint32_t)kv.first.second.size(), kv.first.first, kv.second});
    Built b;
    if (build(pats, &b) != kOk) return fail("build");
    const View v = b.view();
    if (((uint64_t)v.mask + 1) & v.mask) return fail("capacity is no power of two");
    for (const auto& kv : want) {
      const std::string& s = kv.first.second;
      const uint32_t form = kv.first.first;
      if (probe(v, s, form) != kv.second) return fail("pattern not found", s);
      const auto other = want.find(std::make_pair(form ^ 1u, s));
      if (probe(v, s, form ^ 1u) != (other == want.end() ? kNone : other->second)) return fail("wrong form", s);
      for (const std::string& miss : {s.substr(0, s.size() - 1), s + "a", s + "\x80", std::string(1, (char)(s[0] ^ 1)) + s.substr(1)}) {
        if (miss.empty()) continue;
        const auto it = want.find(std::make_pair(form, miss));
        if (probe(v, miss, form) != (it == want.end() ? kNone : it->second)) return fail("near miss", miss);
      }
    }
    // longest(): texts of two words, every code-point start, against brute force
    for (int t = 0; t < 50; t++) {
      std::string text;
      std::vector<uint32_t> cp_starts;
      const int n_cp = 1 + rng() % 14;
      for (int i = 0; i < n_cp; i++) {
        cp_starts.push_back((uint32_t)text.size());
        text += utf8(alphabet[rng() % 8]);
      }
      const uint32_t second = cp_starts[rng() % n_cp];  // the second word starts here (0: one word)
      std::vector<uint32_t> starts(text.size() / 32 + 1, 0);
      starts[0] |= 1u;
      starts[second >> 5] |= 1u << (second & 31);
      const uint64_t nb = text.size();
      for (uint32_t p : cp_starts) {
        const uint32_t form = bit_at(starts.data(), p) ? 0u : 1u;
        const uint64_t end = p < second ? second : nb;
        Match m = {kNone, 0};
        for (uint32_t q : cp_starts)
          if (q > p && q <= end) {
            const auto it = want.find(std::make_pair(form, text.substr(p, q - p)));
            if (it != want.end()) m = Match{it->second, q - p};
          }
        {
          const auto it = want.find(std::make_pair(form, text.substr(p, end - p)));
          if (it != want.end()) m = Match{it->second, (uint32_t)(end - p)};
        }
        const Match g = longest(v, (const uint8_t*)text.data(), nb, starts.data(), p, form);
        if (g.sym != m.sym || g.len != m.len) return fail("longest", text);
      }
    }
  }
  {  // refusals
    Built b;
    const std::string s = "ab";
    std::vector<Pattern> dup = {{(const uint8_t*)s.data(), 2, 0, 1}, {(const uint8_t*)s.data(), 2, 0, 2}};
    if (build(dup, &b) != kDuplicate) return fail("duplicate accepted");
    dup[1].sym = 1;
    if (build(dup, &b) != kOk || probe(b.view(), s, 0) != 1) return fail("equal pattern with one symbol");
    dup[1].form = 1;
    dup[1].sym = 2;
    if (build(dup, &b) != kOk || probe(b.view(), s, 0) != 1 || probe(b.view(), s, 1) != 2) return fail("two forms");
    std::vector<Pattern> empty = {{(const uint8_t*)s.data(), 0, 0, 1}};
    if (build(empty, &b) != kEmptyPattern) return fail("empty pattern accepted");
    if (build({}, &b) != kOk || probe(b.view(), s, 0) != kNone) return fail("empty table");
  }
  printf("ok\n");
  return 0;
}
