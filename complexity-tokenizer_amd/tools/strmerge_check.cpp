// CPU check of the string-keyed merge engine's host side: csrc/strmerge_compile.{h,cpp} (interning,
// the foreign symbol, the pair table, the id map, the initial-token strings) and the merge loop of
// csrc/strmerge_hd.h, which the kernels of csrc/strmerge.hip share, against hard-coded cases.
//   g++ -O2 -std=c++17 -Wall tools/strmerge_check.cpp -o strmerge_check && ./strmerge_check
// prints "ok".  No GPU, no HIP.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/strmerge_compile.cpp"

using namespace strmerge;
typedef std::vector<std::pair<std::string, uint32_t>> Vocab;
typedef std::vector<std::pair<std::string, std::string>> Merges;

static int fails = 0;
#define CHECK(x)                                               \
  do {                                                         \
    if (!(x)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x);  \
      fails++;                                                 \
    }                                                          \
  } while (0)

// the chars of a word as the kernels cut them: from a code-point start to the next
static std::vector<std::string> chars_of(const std::string& w) {
  std::vector<std::string> out;
  for (size_t i = 0; i < w.size();) {
    size_t j = i + 1;
    while (j < w.size() && ((uint8_t)w[j] & 0xC0) == 0x80) j++;
    out.push_back(w.substr(i, j - i));
    i = j;
  }
  return out;
}

static uint32_t lookup(const Compiled& c, const std::string& s, uint32_t form) {
  if (s.empty() || s.size() > c.strings.max_len) return c.foreign;
  const wptab::View v = c.strings.view();
  const uint32_t r = wptab::find(v, (const uint8_t*)s.data(), (uint32_t)s.size(), wptab::hash_of((const uint8_t*)s.data(), (uint32_t)s.size()), form);
  return r == wptab::kNone ? c.foreign : r;
}

// one word through the tables: the ids
static std::vector<uint32_t> encode_word(const Compiled& c, Kind kind, const std::string& w) {
  std::vector<uint32_t> tok;
  if (kind == kByteLevel) {
    for (unsigned char b : w) tok.push_back(c.byte2sym[b]);
  } else if (kind == kWordLevel) {
    tok.push_back(lookup(c, w, 0));
  } else {
    const std::vector<std::string> ch = chars_of(w);
    for (size_t i = 0; i < ch.size(); i++) tok.push_back(lookup(c, ch[i], i + 1 == ch.size() ? 1 : 0));
  }
  std::vector<uint32_t> rank(tok.size() + 1);
  const uint32_t n = merge_word(c.pair_view(), tok.data(), rank.data(), 1, (uint32_t)tok.size());
  std::vector<uint32_t> ids;
  for (uint32_t i = 0; i < n; i++) ids.push_back(c.sym_id[tok[i]]);
  return ids;
}

static std::vector<uint32_t> run(Kind kind, const Vocab& v, const Merges& m, const std::string& suffix, const std::string& w,
                                 const std::string& unk = "<unk>") {
  Compiled c;
  std::string err;
  const int rc = compile(kind, v, m, suffix, unk, &c, &err);
  if (rc != kOk) {
    std::printf("compile failed: %s\n", err.c_str());
    fails++;
    return {};
  }
  return encode_word(c, kind, w);
}

typedef std::vector<uint32_t> Ids;

int main() {
  // one merge per step is not all occurrences of the best pair: abab -> aba b
  {
    const Vocab v = {{"<unk>", 0}, {"a", 1}, {"b", 2}, {"ab", 3}, {"aba", 4}};
    const Merges m = {{"ab", "a"}, {"a", "b"}};
    CHECK(run(kCharBpe, v, m, "", "abab") == (Ids{4, 2}));
    CHECK(run(kByteLevel, v, m, "", "abab") == (Ids{4, 2}));
  }
  // aaa -> aa a, aaaa -> aa aa
  {
    const Vocab v = {{"<unk>", 0}, {"a", 1}, {"aa", 2}};
    const Merges m = {{"a", "a"}};
    CHECK(run(kCharBpe, v, m, "", "aaa") == (Ids{2, 1}));
    CHECK(run(kCharBpe, v, m, "", "aaaa") == (Ids{2, 2}));
    CHECK(run(kByteLevel, v, m, "", "aaaaa") == (Ids{2, 2, 1}));
  }
  // the last duplicate of a pair wins: (a, b) ranks 2, behind (b, c)
  {
    const Vocab v = {{"<unk>", 0}, {"a", 1}, {"b", 2}, {"c", 3}, {"ab", 4}, {"bc", 5}};
    const Merges m = {{"a", "b"}, {"b", "c"}, {"a", "b"}};
    CHECK(run(kCharBpe, v, m, "", "abc") == (Ids{1, 5}));
    CHECK(run(kByteLevel, v, m, "", "abc") == (Ids{1, 5}));
  }
  // merge parts outside the vocab; unk only at the end
  {
    const Vocab v = {{"<unk>", 0}, {"abc", 5}};
    const Merges m = {{"a", "b"}, {"ab", "c"}};
    CHECK(run(kCharBpe, v, m, "", "abc") == (Ids{5}));
    CHECK(run(kCharBpe, v, m, "", "ab") == (Ids{0}));
    CHECK(run(kCharBpe, v, m, "", "ba") == (Ids{0, 0}));
    CHECK(run(kByteLevel, v, m, "", "abc") == (Ids{5}));
  }
  // an unk token that is not in the vocab is id 0; foreign chars never merge
  {
    const Vocab v = {{"x", 7}, {"zz", 9}};
    const Merges m = {{"z", "z"}};
    CHECK(run(kCharBpe, v, m, "", "qq", "[UNK]") == (Ids{0, 0}));
    CHECK(run(kCharBpe, v, m, "", "zz", "[UNK]") == (Ids{9}));
    CHECK(run(kCharBpe, v, m, "", "\xE4\xB8\xAD\xE4\xB8\xADx", "x") == (Ids{7, 7, 7}));
  }
  // the suffix: the last char's token is char + suffix, also of a one-char word
  {
    const Vocab v = {{"<unk>", 0}, {"a", 1}, {"a</w>", 2}, {"aa</w>", 3}};
    const Merges m = {{"a", "a</w>"}};
    CHECK(run(kCharBpe, v, m, "</w>", "a") == (Ids{2}));
    CHECK(run(kCharBpe, v, m, "</w>", "aa") == (Ids{3}));
    CHECK(run(kCharBpe, v, m, "</w>", "aaa") == (Ids{1, 3}));
  }
  // the word-level model: whole words only
  {
    const Vocab v = {{"<unk>", 3}, {"hello", 0xFFFFFFFFu}, {"he", 0x10000}};
    CHECK(run(kWordLevel, v, {}, "", "hello") == (Ids{0xFFFFFFFFu}));
    CHECK(run(kWordLevel, v, {}, "", "hell") == (Ids{3}));
    CHECK(run(kWordLevel, v, {}, "", "helloo") == (Ids{3}));
    CHECK(run(kWordLevel, v, {}, "", "he") == (Ids{0x10000}));
    CHECK(run(kWordLevel, {}, {}, "", "he") == (Ids{0}));
  }
  // the tables themselves
  {
    const Vocab v = {{"<unk>", 0}, {"a", 1}};
    const Merges m = {{"a", "b"}, {"ab", "a"}, {"a", "b"}};
    Compiled c;
    std::string err;
    CHECK(compile(kByteLevel, v, m, "", "<unk>", &c, &err) == kOk);
    // vocab 2, byte chars 256 ("a", "b" among them), "ab", "aba"
    CHECK(c.foreign == 2 + 255 + 2 && c.sym_id.size() == c.foreign + 1 && c.sym_id[c.foreign] == 0);
    const uint32_t a = c.byte2sym['a'], b = c.byte2sym['b'];
    CHECK(c.sym_str[a] == "a" && c.sym_str[b] == "b" && c.sym_id[a] == 1 && c.sym_id[b] == 0);
    const Merge ab = pair_find(c.pair_view(), a, b);
    CHECK(ab.rank == 2 && c.sym_str[ab.sym] == "ab");
    CHECK(pair_find(c.pair_view(), ab.sym, a).rank == 1);
    CHECK(pair_find(c.pair_view(), b, a).rank == kNoRank);
    CHECK(pair_find(c.pair_view(), c.foreign, c.foreign).rank == kNoRank);
    CHECK(byte_char(0x20) == "\xC4\xA0" && byte_char('!') == "!" && byte_char(0) == "\xC4\x80" && byte_char(0xFF) == "\xC3\xBF");
    // duplicates and bad strings
    CHECK(compile(kCharBpe, {{"a", 1}, {"a", 2}}, {}, "", "<unk>", &c, &err) == kErrArg);
    CHECK(compile(kCharBpe, {{"\xFF", 1}}, {}, "", "<unk>", &c, &err) == kErrArg);
    CHECK(one_char("\xE4\xB8\xAD") == 3 && one_char("ab") == 0 && one_char("") == 0 && one_char("\xE4\xB8") == 0);
  }
  // many pairs: every one is found with its rank, and none that was not given
  {
    Vocab v;
    Merges m;
    for (int i = 0; i < 3000; i++) m.emplace_back("t" + std::to_string(i), "u" + std::to_string(i % 7));
    Compiled c;
    std::string err;
    CHECK(compile(kCharBpe, v, m, "", "<unk>", &c, &err) == kOk);
    std::vector<uint32_t> sym_of_t(3000), sym_of_u(7);
    for (uint32_t s = 0; s < c.foreign; s++) {
      const std::string& t = c.sym_str[s];
      if (t[0] == 't' && t.find('u') == std::string::npos) sym_of_t[std::stoi(t.substr(1))] = s;
      if (t[0] == 'u') sym_of_u[std::stoi(t.substr(1))] = s;
    }
    bool all = true;
    for (int i = 0; i < 3000; i++) {
      const Merge r = pair_find(c.pair_view(), sym_of_t[i], sym_of_u[i % 7]);
      all = all && r.rank == (uint32_t)i && c.sym_str[r.sym] == m[i].first + m[i].second;
      all = all && pair_find(c.pair_view(), sym_of_t[i], sym_of_u[(i + 1) % 7]).rank == kNoRank;
    }
    CHECK(all);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
