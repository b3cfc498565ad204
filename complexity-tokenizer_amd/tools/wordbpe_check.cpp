// CPU check of the id-keyed word BPE's host side: csrc/wordbpe_compile.{h,cpp} (the code-point table,
// the pair table with the rank / new-id quirk and the panic mark, the added-token pool) and the
// scalar loops of csrc/wordbpe_hd.h, which the kernels of csrc/wordbpe.hip share (the added-token
// loop, the merge loop with the panic mark).
//   g++ -O2 -std=c++17 -Wall tools/wordbpe_check.cpp -o wordbpe_check && ./wordbpe_check
// prints "ok" after the hard-coded cases.  With a file argument it also runs that case table
// (tests/test_pipeline_cpu.py writes it from tests/pipeline_cases.py with the oracle's answers):
//   u32 n_cases; per case: u32 n_vocab {str, u32 id}, u32 n_merges {str, str}, u32 n_added {str, u32 id,
//   u32 flags}, u32 n_words {str, u32 tokenize, u32 panics, u32 n, u32 expected[n]}; str: u32 len, bytes.
// No GPU, no HIP.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/gen/alnum_data.h"
#include "../csrc/wordbpe_compile.cpp"

using namespace wordbpe;
typedef std::vector<std::pair<std::string, uint32_t>> Vocab;
typedef std::vector<std::pair<std::string, std::string>> Merges;
typedef std::vector<AddedToken> Added;
typedef std::vector<uint32_t> Ids;

static int fails = 0;
#define CHECK(x)                                               \
  do {                                                         \
    if (!(x)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x);  \
      fails++;                                                 \
    }                                                          \
  } while (0)

// BpeTokenizer::encode of the bytes [a, b): false when a marked pair is seen (*rank: its rank)
static bool bpe(const Compiled& c, const std::string& w, size_t a, size_t b, Ids* out, uint32_t* rank) {
  Ids tok;
  const uint8_t* t = (const uint8_t*)w.data();
  for (size_t p = a; p < b;) {
    uint32_t cp = 0;
    const uint32_t l = dec_char(t, p, b, &cp);
    if (!l) {  // (an ill-formed byte is a unit in no vocab string)
      p++;
      continue;
    }
    const uint32_t id = cp_find(c.cp_view(), cp);
    if (id != kNoId) tok.push_back(id);
    p += l;
  }
  Ids cache(tok.size() + 1);
  uint32_t pr = kNoPanic;
  const uint32_t n = merge_ids(c.pair_view(), tok.data(), cache.data(), 1, (uint32_t)tok.size(), &pr);
  if (pr != kNoPanic) {
    *rank = pr;
    return false;
  }
  out->insert(out->end(), tok.begin(), tok.begin() + n);
  return true;
}

// one word through the tables: the ids
static bool encode_word(const Compiled& c, const std::string& w, bool tokenize, Ids* out, uint32_t* rank) {
  if (tokenize || c.a_id.empty()) return bpe(c, w, 0, w.size(), out, rank);
  const AddedView av = c.added_view(wb_alnum_lo, wb_alnum_hi, WB_N_ALNUM);
  const uint8_t* t = (const uint8_t*)w.data();
  const uint32_t n = split_word(av, t, 0, w.size(), nullptr, nullptr);
  std::vector<Seg> segs(n);
  CHECK(split_word(av, t, 0, w.size(), nullptr, segs.data()) == n);
  for (const Seg& s : segs) {
    if (s.a == kNoId) out->push_back(s.b);
    else if (!bpe(c, w, s.a, s.b, out, rank)) return false;
  }
  return true;
}

static Ids run(const Vocab& v, const Merges& m, const Added& a, const std::string& w, bool tokenize = false) {
  Compiled c;
  std::string err;
  if (compile(v, m, a, &c, &err) != kOk) {
    std::printf("compile failed: %s\n", err.c_str());
    fails++;
    return {};
  }
  Ids out;
  uint32_t rank = 0;
  if (!encode_word(c, w, tokenize, &out, &rank)) return Ids{0xDEADu, rank, (uint32_t)c.n_filtered};
  return out;
}

static void hard_coded() {
  const Vocab abc = {{"a", 0}, {"b", 1}, {"c", 2}, {"ab", 3}, {"bc", 4}, {"abc", 5}, {"aa", 6}, {"aaaa", 7}};
  // src/bpe.rs:219-250 in the small: lowest rank, leftmost, one merge per step
  CHECK(run(abc, {{"a", "a"}}, {}, "aaa") == (Ids{6, 0}));
  CHECK(run(abc, {{"a", "a"}, {"aa", "aa"}}, {}, "aaaaa") == (Ids{7, 0}));
  CHECK(run(abc, {{"a", "b"}, {"ab", "c"}}, {}, "abcab") == (Ids{5, 3}));
  CHECK(run(abc, {}, {}, "") == (Ids{}));
  // a char without a one-char vocab string is dropped: its neighbours become adjacent and merge
  CHECK(run(abc, {{"a", "b"}}, {}, "a?b") == (Ids{3}));
  CHECK(run(abc, {{"a", "b"}}, {}, "\xE4\xB8\xAD??") == (Ids{}));
  // the duplicate pair: the later rank wins, so (b, c) at rank 1 goes first ...
  CHECK(run(abc, {{"a", "b"}, {"b", "c"}, {"a", "b"}}, {}, "abc") == (Ids{0, 4}));
  // ... and the pair's new id is the filtered list's entry at that rank: filtered = [ab, bc, ab]
  {
    Compiled c;
    std::string err;
    CHECK(compile(abc, {{"a", "b"}, {"b", "c"}, {"a", "b"}}, {}, &c, &err) == kOk);
    CHECK(c.n_filtered == 3 && c.n_pairs == 2 && c.n_panic == 0);
    const strmerge::Merge ab = strmerge::pair_find(c.pair_view(), 0, 1);
    CHECK(ab.rank == 2 && ab.sym == 3);
  }
  // the rank shift after an invalid merge: (x, y) is dropped, so filtered = [ab, bc]; (a, b) keeps
  // rank 1 and takes filtered[1] = bc's id; (b, c) has rank 2 >= 2: the panic mark
  {
    const Merges m = {{"x", "y"}, {"a", "b"}, {"b", "c"}};
    Compiled c;
    std::string err;
    CHECK(compile(abc, m, {}, &c, &err) == kOk);
    CHECK(c.n_filtered == 2 && c.n_pairs == 2 && c.n_panic == 1);
    const strmerge::Merge ab = strmerge::pair_find(c.pair_view(), 0, 1), bc = strmerge::pair_find(c.pair_view(), 1, 2);
    CHECK(ab.rank == 1 && ab.sym == 4 && !is_panic(ab.rank));
    CHECK(is_panic(bc.rank) && (bc.rank & ~kPanicBit) == 2);
    CHECK(run(abc, m, {}, "ab") == (Ids{4}));
    CHECK(run(abc, m, {}, "abab") == (Ids{4, 4}));
    CHECK(run(abc, m, {}, "bc") == (Ids{0xDEADu, 2, 2}));
    CHECK(run(abc, m, {}, "aabc") == (Ids{0xDEADu, 2, 2}));  // seen adjacent, not the best pair
    CHECK(run(abc, m, {}, "cb") == (Ids{2, 1}));
  }
  // the marked pair only becomes adjacent after a merge.  filtered = [aa, cb, cbb]: (a, a) has rank 1
  // and so the new id of "cb"; (cb, b) has rank 3 >= 3.  a a b -> cb b, and that pair is marked.
  {
    const Vocab v = {{"a", 0}, {"b", 1}, {"c", 2}, {"aa", 3}, {"cb", 4}, {"cbb", 5}};
    const Merges m = {{"q", "q"}, {"a", "a"}, {"c", "b"}, {"cb", "b"}};
    CHECK(run(v, m, {}, "aab") == (Ids{0xDEADu, 3, 3}));
    CHECK(run(v, m, {}, "baab") == (Ids{0xDEADu, 3, 3}));
    CHECK(run(v, m, {}, "aa") == (Ids{4}));
    CHECK(run(v, m, {}, "cb") == (Ids{5}));
  }
  // two vocab strings share an id: their pairs share a table entry, the later merge's rank wins
  {
    const Vocab v = {{"a", 0}, {"A", 0}, {"b", 1}, {"ab", 2}, {"Ab", 3}};
    Compiled c;
    std::string err;
    CHECK(compile(v, {{"a", "b"}, {"A", "b"}}, {}, &c, &err) == kOk);
    CHECK(c.n_pairs == 1 && c.n_filtered == 2);
    const strmerge::Merge e = strmerge::pair_find(c.pair_view(), 0, 1);
    CHECK(e.rank == 1 && e.sym == 3);
    CHECK(run(v, {{"a", "b"}, {"A", "b"}}, {}, "ab") == (Ids{3}));
  }
  // added tokens: start, middle, end, two adjacent, a prefix of another (the longest wins)
  {
    const Added a = {{"<s>", 100, 0}, {"<s>>", 101, 0}, {"[X]", 102, 0}};
    CHECK(run(abc, {{"a", "b"}}, a, "<s>ab") == (Ids{100, 3}));
    CHECK(run(abc, {{"a", "b"}}, a, "ab<s>ab") == (Ids{3, 100, 3}));
    CHECK(run(abc, {{"a", "b"}}, a, "ab[X]") == (Ids{3, 102}));
    CHECK(run(abc, {{"a", "b"}}, a, "<s>[X]") == (Ids{100, 102}));
    CHECK(run(abc, {{"a", "b"}}, a, "a<s>>b") == (Ids{0, 101, 1}));
    CHECK(run(abc, {{"a", "b"}}, a, "a<s>>b", true) == (Ids{3}));  // tokenize: no added-token loop, so a and b meet
  }
  // single_word, and the first-occurrence rule: the first "<w>" fails (a letter before it) and hides
  // the second, which would pass
  {
    const Added a = {{"<w>", 100, kSingleWord}};
    CHECK(run(abc, {}, a, "a <w> b") == (Ids{0, 100, 1}));
    CHECK(run(abc, {}, a, "a<w> <w>") == (Ids{0}));
    CHECK(run(abc, {}, a, "<w>a") == (Ids{0}));
    CHECK(run(abc, {}, a, "\xC3\xA9<w>") == (Ids{}));  // U+00E9 is a letter
  }
  // lstrip / rstrip
  {
    const Added l = {{"<l>", 100, kLstrip}}, r = {{"<r>", 101, kRstrip}};
    CHECK(run(abc, {}, l, "a <l>b") == (Ids{0, 100, 1}));
    CHECK(run(abc, {}, l, "a<l>b") == (Ids{0, 1}));
    CHECK(run(abc, {}, l, "<l>b") == (Ids{100, 1}));
    CHECK(run(abc, {}, l, "a\xE3\x80\x80<l>") == (Ids{0, 100}));  // U+3000 is white space
    CHECK(run(abc, {}, r, "a<r> b") == (Ids{0, 101, 1}));
    CHECK(run(abc, {}, r, "a<r>b") == (Ids{0, 1}));
    CHECK(run(abc, {}, r, "a<r>") == (Ids{0, 101}));
  }
  // refusals
  {
    Compiled c;
    std::string err;
    CHECK(compile(abc, {}, {{"", 1, 0}}, &c, &err) == kErrUnsupported);
    CHECK(compile({{"a", 0xFFFFFFFFu}}, {}, {}, &c, &err) == kErrUnsupported);
    Added many;
    for (uint32_t i = 0; i <= kMaxAdded; i++) many.push_back(AddedToken{"<" + std::to_string(i) + ">", i, 0});
    CHECK(compile(abc, {}, many, &c, &err) == kErrUnsupported);
    many.pop_back();
    CHECK(compile(abc, {}, many, &c, &err) == kOk && c.a_id.size() == kMaxAdded);
    // a content given twice keeps its last entry
    CHECK(compile(abc, {}, {{"<s>", 1, 0}, {"<s>", 2, kLstrip}}, &c, &err) == kOk && c.a_id == (Ids{2}) && c.a_flags == (Ids{kLstrip}));
  }
  // many chars and pairs: every one is found, and none that was not given
  {
    Vocab v;
    Merges m;
    for (uint32_t i = 0; i < 3000; i++) {
      const uint32_t cp = 0x4E00 + i;
      std::string s;
      s += (char)(0xE0 | (cp >> 12));
      s += (char)(0x80 | ((cp >> 6) & 63));
      s += (char)(0x80 | (cp & 63));
      v.emplace_back(s, i);
    }
    for (uint32_t i = 0; i + 1 < 3000; i++) {
      v.emplace_back(v[i].first + v[i + 1].first, 3000 + i);
      m.emplace_back(v[i].first, v[i + 1].first);
    }
    Compiled c;
    std::string err;
    CHECK(compile(v, m, {}, &c, &err) == kOk);
    bool all = true;
    for (uint32_t i = 0; i < 3000; i++) all = all && cp_find(c.cp_view(), 0x4E00 + i) == i;
    all = all && cp_find(c.cp_view(), 0x4E00 + 3000) == kNoId && cp_find(c.cp_view(), 'a') == kNoId;
    for (uint32_t i = 0; i + 1 < 3000; i++) {
      const strmerge::Merge r = strmerge::pair_find(c.pair_view(), i, i + 1);
      all = all && r.rank == i && r.sym == 3000 + i;
      all = all && strmerge::pair_find(c.pair_view(), i + 1, i).rank == kNoRank;
    }
    CHECK(all);
  }
  // the char helpers
  {
    const uint8_t t[] = {'a', 0xC3, 0xA9, 0xE4, 0xB8, 0xAD, 0xF0, 0x9F, 0x98, 0x80, 0xC3, 'x', 0x80};
    CHECK(char_at(t, 0, 13) == 'a' && char_at(t, 1, 13) == 0xE9 && char_at(t, 3, 13) == 0x4E2D && char_at(t, 6, 13) == 0x1F600);
    CHECK(char_at(t, 10, 13) == kNoId && char_at(t, 12, 13) == kNoId && char_at(t, 1, 2) == kNoId);
    CHECK(char_before(t, 0, 1) == 'a' && char_before(t, 0, 3) == 0xE9 && char_before(t, 0, 6) == 0x4E2D && char_before(t, 0, 10) == 0x1F600);
    CHECK(char_before(t, 0, 0) == kNoId && char_before(t, 2, 3) == kNoId && char_before(t, 0, 13) == kNoId);
    const AddedView av{nullptr, nullptr, nullptr, nullptr, nullptr, wb_alnum_lo, wb_alnum_hi, WB_N_ALNUM, 0};
    CHECK(is_alnum(av, 'a') && is_alnum(av, '7') && is_alnum(av, 0xE9) && is_alnum(av, 0x4E2D) && is_alnum(av, 0xBD));
    CHECK(!is_alnum(av, ' ') && !is_alnum(av, '_') && !is_alnum(av, 0x300) && !is_alnum(av, 0x1F600) && !is_alnum(av, kNoId));
    CHECK(is_ws(0x20) && is_ws(0x85) && is_ws(0x3000) && !is_ws(0x200B) && !is_ws(0x1C));
  }
}

// ---- the case table --------------------------------------------------------------------------------

static bool rd_u32(std::FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }
static bool rd_str(std::FILE* f, std::string* s) {
  uint32_t n = 0;
  if (!rd_u32(f, &n) || n > (1u << 26)) return false;
  s->resize(n);
  return !n || std::fread(&(*s)[0], 1, n, f) == n;
}

static void case_table(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::printf("cannot open %s\n", path);
    fails++;
    return;
  }
  uint32_t n_cases = 0, words = 0;
  bool ok = rd_u32(f, &n_cases);
  for (uint32_t ci = 0; ok && ci < n_cases; ci++) {
    Vocab v;
    Merges m;
    Added a;
    uint32_t n = 0;
    ok = rd_u32(f, &n);
    for (uint32_t i = 0; ok && i < n; i++) {
      std::string s;
      uint32_t id = 0;
      ok = rd_str(f, &s) && rd_u32(f, &id);
      v.emplace_back(s, id);
    }
    ok = ok && rd_u32(f, &n);
    for (uint32_t i = 0; ok && i < n; i++) {
      std::string x, y;
      ok = rd_str(f, &x) && rd_str(f, &y);
      m.emplace_back(x, y);
    }
    ok = ok && rd_u32(f, &n);
    for (uint32_t i = 0; ok && i < n; i++) {
      AddedToken t;
      ok = rd_str(f, &t.content) && rd_u32(f, &t.id) && rd_u32(f, &t.flags);
      a.push_back(t);
    }
    Compiled c;
    std::string err;
    if (ok && compile(v, m, a, &c, &err) != kOk) {
      std::printf("case %u: compile failed: %s\n", ci, err.c_str());
      fails++;
      ok = false;
    }
    ok = ok && rd_u32(f, &n);
    for (uint32_t i = 0; ok && i < n; i++) {
      std::string w;
      uint32_t tokenize = 0, panics = 0, k = 0;
      ok = rd_str(f, &w) && rd_u32(f, &tokenize) && rd_u32(f, &panics) && rd_u32(f, &k);
      Ids want(k);
      for (uint32_t j = 0; ok && j < k; j++) ok = rd_u32(f, &want[j]);
      if (!ok) break;
      Ids got;
      uint32_t rank = 0;
      const bool fine = encode_word(c, w, tokenize != 0, &got, &rank);
      const bool same = panics ? (!fine && k == 2 && want[0] == c.n_filtered && want[1] == rank) : (fine && got == want);
      if (!same) {
        std::printf("FAIL case %u word %u (%s)\n", ci, i, w.c_str());
        fails++;
      }
      words++;
    }
  }
  if (!ok) {
    std::printf("the case table is cut short\n");
    fails++;
  }
  std::fclose(f);
  std::fprintf(stderr, "%u cases, %u words\n", n_cases, words);
}

int main(int argc, char** argv) {
  hard_coded();
  if (argc > 1) case_table(argv[1]);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
