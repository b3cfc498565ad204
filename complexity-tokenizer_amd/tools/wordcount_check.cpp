// Host-side check of the word-counting kernels' pure functions (csrc/wordcount_hd.h): descriptor
// pack / unpack at the field limits, length clipping, the unaligned dword loads, and hash + compare
// against plain string equality, through a sequential restatement of the kernel's probing.
//   g++ -O2 -std=c++17 tools/wordcount_check.cpp -o wordcount_check && ./wordcount_check
// Exit status 0 and "ok" when every check holds, else 1 and the failing check.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../csrc/wordcount_hd.h"

static int g_bad = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_bad++;                                                  \
    }                                                           \
  } while (0)

// text in a 4-byte aligned buffer with 16 spare bytes, as the device buffers are
struct Buf {
  std::vector<uint32_t> w;
  uint64_t n;
  explicit Buf(const std::string& s) : w((s.size() + 16 + 3) / 4, 0xA5A5A5A5u), n(s.size()) { std::memcpy(w.data(), s.data(), s.size()); }
  const uint8_t* p() const { return reinterpret_cast<const uint8_t*>(w.data()); }
};

int main() {
  // pack / unpack round trips at the field limits
  const uint32_t poss[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xEFFFFFFFu, 0xFFFFFFFEu};
  const uint32_t lens[] = {1u, 2u, 0xFFu, 0x100u, 0xFFFEu, 0xFFFFu};
  const uint32_t tags[] = {0u, 1u, 0x8000u, 0xFFFFu};
  for (uint32_t pos : poss)
    for (uint32_t len : lens)
      for (uint32_t tag : tags) {
        const uint64_t d = wc::pack(pos, len, tag);
        CHECK(wc::pos_of(d) == pos && wc::len_of(d) == len && wc::tag_of(d) == tag);
        CHECK(d != wc::kEmpty);  // (no text position is 0xFFFFFFFF)
        CHECK(wc::may_match(d, len, tag));
        CHECK(!wc::may_match(d, len ^ 1u, tag) && !wc::may_match(d, len, tag ^ 1u));
        CHECK(wc::may_match(wc::pack(pos ^ 0x55u, len, tag), len, tag));  // the position is not compared
      }
  CHECK(wc::pack(0xFFFFFFFFu, 0xFFFFu, 0xFFFFu) == wc::kEmpty);  // why positions stop below 2^32 - 1
  // bits above a field's width do not leak into its neighbours
  CHECK(wc::pack(5, 0x12345u, 0x6789Au) == wc::pack(5, 0x2345u, 0x789Au));

  // length clipping: exact below kLenClip, kLenClip from there on
  CHECK(wc::clip_len(0) == 0 && wc::clip_len(1) == 1 && wc::clip_len(0xFFFE) == 0xFFFE);
  CHECK(wc::clip_len(0xFFFF) == 0xFFFF && wc::clip_len(0x10000) == 0xFFFF && wc::clip_len(0xEFFFFFFFull) == 0xFFFF);
  // two words of >= kLenClip bytes have the same clipped length whatever their lengths: the
  // descriptor compare alone must not tell them apart (the bitmap does)
  CHECK(wc::may_match(wc::pack(0, wc::clip_len(70000), 7), wc::clip_len(65535), 7));
  CHECK(!wc::may_match(wc::pack(0, wc::clip_len(65534), 7), wc::clip_len(65535), 7));

  // load4 at every alignment
  {
    std::string s;
    for (int i = 0; i < 64; i++) s += (char)(i * 7 + 1);
    Buf b(s);
    for (uint64_t p = 0; p + 4 <= s.size(); p++) {
      uint32_t want;
      std::memcpy(&want, s.data() + p, 4);
      CHECK(wc::load4(b.p(), p) == want);
    }
    CHECK(wc::tail_mask(0xAABBCCDDu, 1) == 0xDDu && wc::tail_mask(0xAABBCCDDu, 3) == 0xBBCCDDu);
  }

  // words_equal / word_hash against string equality on every pair of substrings of a text built
  // to hold near misses: equal words at different alignments, words that differ only in the last
  // byte, prefixes of each other, NUL bytes, and lengths around the dword and kHashBytes limits
  {
    std::string s;
    const int lens2[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300};
    std::vector<std::pair<uint64_t, uint64_t>> words;  // (pos, len)
    auto add = [&](const std::string& w) {
      words.emplace_back(s.size(), w.size());
      s += w;
    };
    for (int rep = 0; rep < 3; rep++)  // every word three times, at shifting alignments
      for (int n : lens2) {
        add(std::string(n, 'x'));
        add(std::string(n - 1, 'x') + "y");
        add(std::string(n - 1, 'x') + std::string(1, '\0'));
        if (rep == 1) add("z");  // (shifts what follows by one byte)
      }
    add(std::string("a\0", 2));
    add(std::string("a\0\0", 3));
    add("a");
    Buf b(s);
    for (size_t i = 0; i < words.size(); i++)
      for (size_t j = 0; j < words.size(); j++) {
        const auto [p, n] = words[i];
        const auto [r, m] = words[j];
        const bool same = s.substr(p, n) == s.substr(r, m);
        if (n == m) CHECK(wc::words_equal(b.p(), p, r, n) == same);
        if (same) CHECK(wc::word_hash(b.p(), p, n) == wc::word_hash(b.p(), r, m));
      }
    // the hash does not read past the word: the same word before different bytes hashes the same
    std::string s2 = s;
    for (auto& c : s2) c = (char)(c ^ 0x5A);
    Buf b1("ab" + s), b2("ab" + s2);
    CHECK(wc::word_hash(b1.p(), 0, 2) == wc::word_hash(b2.p(), 0, 2));
    CHECK(wc::word_hash(b1.p(), 1, 1) == wc::word_hash(b2.p(), 1, 1));

    // the kernel's probing, sequentially: a table of descriptors, counts beside them
    const uint32_t mask = 255;
    std::vector<uint64_t> keys(mask + 1, wc::kEmpty);
    std::vector<uint32_t> vals(mask + 1, 0);
    std::map<std::string, uint32_t> want;
    for (const auto& [p, n] : words) {
      want[s.substr(p, n)]++;
      const uint64_t h64 = wc::word_hash(b.p(), p, n);
      const uint32_t lc = wc::clip_len(n), tag = (uint32_t)h64 & 0xFFFFu;
      uint32_t h = (uint32_t)(h64 >> 32) & mask;
      bool done = false;
      for (uint32_t t = 0; t <= mask && !done; t++, h = (h + 1) & mask) {
        if (keys[h] == wc::kEmpty) keys[h] = wc::pack((uint32_t)p, lc, tag);
        if (wc::may_match(keys[h], lc, tag) && wc::words_equal(b.p(), p, wc::pos_of(keys[h]), n)) {
          vals[h]++;
          done = true;
        }
      }
      CHECK(done);
    }
    std::map<std::string, uint32_t> got;
    for (uint32_t h = 0; h <= mask; h++)
      if (keys[h] != wc::kEmpty) {
        const std::string w = s.substr(wc::pos_of(keys[h]), wc::len_of(keys[h]));
        CHECK(!got.count(w));
        got[w] = vals[h];
      }
    CHECK(got == want);
  }
  if (g_bad) return 1;
  std::printf("ok\n");
  return 0;
}
