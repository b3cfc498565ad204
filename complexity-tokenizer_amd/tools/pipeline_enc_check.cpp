// CPU check of csrc/pipeline_enc_hd.h, the rules the kernels of csrc/pipeline_enc.hip share: the needle
// trim, the search with its fallback and work count, the boundary test, the closed form of the token
// spans and the row cell rule, each against a literal restatement of the reference's loop
// (src/huggingface/mod.rs:358-480), over hard-coded cases and the case file a test writes.
//   g++ -O2 -std=c++17 -Wall tools/pipeline_enc_check.cpp -o pipeline_enc_check && ./pipeline_enc_check [cases]
// Case file, one record a line, bytes in hex ("-" for none):
//   S <original> <n_words> <panic byte index or -1> <work or -1>   then n_words lines
//   W <word> <start> <end>        (a sequence that panics lists the words before the panic)
//   T <word start> <word end> <n> <len>*n <start end>*n
// Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/pipeline_enc_hd.h"

using namespace pipeline_enc;
using Bytes = std::vector<uint8_t>;

static int g_fail = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);         \
      std::printf("\n");                \
      if (++g_fail > 20) std::exit(1);  \
    }                                   \
  } while (0)

static Bytes bytes_of(const std::string& s) { return Bytes(s.begin(), s.end()); }

static Bytes unhex(const std::string& h) {
  Bytes b;
  if (h == "-") return b;
  for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
  return b;
}

// ---- literal restatements ---------------------------------------------------------------------------

// trim_start_matches(|c| c == 'Ġ' || c == '▁') char by char; if empty, the word itself
static Bytes lit_needle(const Bytes& w) {
  size_t t = 0;
  while (t < w.size()) {
    if (w.size() - t >= 2 && w[t] == 0xC4 && w[t + 1] == 0xA0) t += 2;
    else if (w.size() - t >= 3 && w[t] == 0xE2 && w[t + 1] == 0x96 && w[t + 2] == 0x81) t += 3;
    else break;
  }
  Bytes n(w.begin() + t, w.end());
  return n.empty() ? w : n;
}

// original[s..].find(needle): memcmp at every position of a copy that ends at the text's end
static int64_t lit_find(const Bytes& o, size_t s, const Bytes& needle) {
  const Bytes tail(o.begin() + s, o.end());  // (a copy: a read past the end is the sanitizer's to see)
  if (needle.empty()) return (int64_t)s;
  for (size_t p = 0; p + needle.size() <= tail.size(); p++)
    if (!std::memcmp(tail.data() + p, needle.data(), needle.size())) return (int64_t)(s + p);
  return -1;
}

struct Span {
  uint64_t start, end;
};

// pre_tokenize_with_offsets; returns the byte index of the panic or -1; *work: the work of the words walked
static int64_t lit_words(const Bytes& o, const std::vector<Bytes>& words, std::vector<Span>* out, uint64_t* work) {
  size_t s = 0;
  *work = 0;
  for (const Bytes& w : words) {
    if (s < o.size() && (o[s] & 0xC0) == 0x80) return (int64_t)s;
    const Bytes needle = lit_needle(w);
    const int64_t pos = lit_find(o, s, needle);
    Span sp;
    if (pos >= 0) {
      sp = Span{(uint64_t)pos, (uint64_t)pos + needle.size()};
      *work += (uint64_t)pos - s + needle.size();
    } else {
      sp = Span{s, std::min<uint64_t>(s + w.size(), o.size())};
      *work += o.size() - s;
    }
    out->push_back(sp);
    s = sp.end;
  }
  return -1;
}

// ---- the header's forms, driven as the kernel drives them -----------------------------------------------

// the window search of k_pe_word_find: 64 candidates a window, the lowest lane of the first window with a match
static uint64_t window_find(const uint8_t* text, uint64_t L, uint64_t s, const uint8_t* needle, uint64_t m) {
  if (!m) return s;
  for (uint64_t base = s; base <= L && m <= L - base; base += 64)
    for (uint64_t lane = 0; lane < 64; lane++)
      if (match_at(text, L, base + lane, needle, m)) return base + lane;
  return L + 1;
}

static int64_t hd_words(const Bytes& o_in, const std::vector<Bytes>& words, std::vector<Span>* out, uint64_t* work) {
  // the text in an allocation of its own size, so that a read at or past its end is an error under the sanitizer
  const Bytes o(o_in);
  const uint64_t L = o.size();
  uint64_t s = 0;
  *work = 0;
  for (const Bytes& w : words) {
    if (boundary_panic(o.data(), L, s)) return (int64_t)s;
    const uint64_t skip = needle_skip(w.data(), w.size());
    const uint8_t* needle = w.data() + skip;
    const uint64_t m = w.size() - skip;
    const uint64_t pos = window_find(o.data(), L, s, needle, m);
    const uint64_t pos2 = find_scalar(o.data(), L, s, needle, m);
    CHECK(pos == pos2, "window search %llu, scalar search %llu", (unsigned long long)pos, (unsigned long long)pos2);
    Span sp;
    uint64_t wk;
    word_span(pos, s, m, w.size(), L, &sp.start, &sp.end, &wk);
    CHECK(sp.start <= sp.end && sp.end <= L, "a span out of order");
    out->push_back(sp);
    *work += wk;
    s = sp.end;
  }
  return -1;
}

static void check_sequence(const Bytes& o, const std::vector<Bytes>& words, const std::vector<Span>* want, int64_t want_panic,
                           int64_t want_work) {
  std::vector<Span> a, b;
  uint64_t wa = 0, wb = 0;
  const int64_t pa = lit_words(o, words, &a, &wa), pb = hd_words(o, words, &b, &wb);
  CHECK(pa == pb, "panic %lld, literal %lld", (long long)pb, (long long)pa);
  CHECK(wa == wb, "work %llu, literal %llu", (unsigned long long)wb, (unsigned long long)wa);
  CHECK(a.size() == b.size(), "%zu spans, literal %zu", b.size(), a.size());
  for (size_t i = 0; i < a.size() && i < b.size(); i++)
    CHECK(a[i].start == b[i].start && a[i].end == b[i].end, "word %zu: (%llu, %llu), literal (%llu, %llu)", i,
          (unsigned long long)b[i].start, (unsigned long long)b[i].end, (unsigned long long)a[i].start, (unsigned long long)a[i].end);
  if (!want) return;
  CHECK(pb == want_panic, "panic %lld, the case file has %lld", (long long)pb, (long long)want_panic);
  if (want_work >= 0) CHECK((int64_t)wb == want_work, "work %llu, the case file has %lld", (unsigned long long)wb, (long long)want_work);
  CHECK(b.size() == want->size(), "%zu spans, the case file has %zu", b.size(), want->size());
  for (size_t i = 0; i < b.size() && i < want->size(); i++)
    CHECK(b[i].start == (*want)[i].start && b[i].end == (*want)[i].end, "word %zu differs from the case file", i);
}

// the token loop of encode_single_to_encoding against tok_span over an exclusive scan that starts anywhere
static void check_tokens(uint64_t ws, uint64_t we, const std::vector<uint64_t>& lens, const std::vector<Span>* want) {
  std::vector<uint64_t> scan(lens.size() + 1);
  scan[0] = 12345;  // the ids before this word
  for (size_t k = 0; k < lens.size(); k++) scan[k + 1] = scan[k] + lens[k];
  uint64_t p = ws;
  for (size_t k = 0; k < lens.size(); k++) {
    const uint64_t e = std::min(p + lens[k], we);
    uint64_t a, b;
    tok_span(ws, we, scan[k], scan[k + 1], scan[0], &a, &b);
    CHECK(a == p && b == e, "token %zu: (%llu, %llu), literal (%llu, %llu)", k, (unsigned long long)a, (unsigned long long)b,
          (unsigned long long)p, (unsigned long long)e);
    if (want) CHECK((*want)[k].start == a && (*want)[k].end == b, "token %zu differs from the case file", k);
    p = e;
  }
}

static void check_rows() {
  const uint32_t special[] = {3, 7, 900};
  for (uint64_t n = 0; n < 6; n++)
    for (uint64_t na = 0; na <= n; na++)
      for (uint64_t L = n; L < n + 4; L++) {
        // the literal lists: type ids na zeros, n - na ones, then zeros; special n zeros, then ones; then the ids' own
        std::vector<uint32_t> type(na, 0), spec(n, 0), ids;
        type.insert(type.end(), n - na, 1);
        type.insert(type.end(), L - n, 0);
        spec.insert(spec.end(), L - n, 1);
        for (uint64_t i = 0; i < L; i++) ids.push_back((uint32_t)((i * 7 + n) % 11));
        for (uint64_t i = 0; i < L; i++)
          if (ids[i] == 3 || ids[i] == 7) spec[i] = 1;
        for (uint64_t i = 0; i < L; i++) {
          uint32_t t, s;
          row_cell(i, n, na, is_special(special, 3, ids[i]), &t, &s);
          CHECK(t == type[i] && s == spec[i], "row cell %llu of n %llu, na %llu", (unsigned long long)i, (unsigned long long)n,
                (unsigned long long)na);
        }
      }
  const uint32_t ids[] = {2, 5, 9, 4000000000u}, lens[] = {1, 0, 7, 3};
  CHECK(table_len(ids, lens, 4, 9) == 7 && table_len(ids, lens, 4, 5) == 0 && table_len(ids, lens, 4, 3) == 0 &&
            table_len(ids, lens, 4, 4000000000u) == 3 && table_len(ids, lens, 4, 4294967295u) == 0 && table_len(ids, lens, 0, 1) == 0,
        "table_len");
  const uint64_t pos[] = {0, 0, 2, 2, 2, 5};  // owners of an id: the last entry at or below it
  CHECK(find_owner(pos, 5, 0) == 1 && find_owner(pos, 5, 1) == 1 && find_owner(pos, 5, 2) == 4 && find_owner(pos, 5, 4) == 4, "find_owner");
  const uint32_t pos32[] = {0, 3, 3, 4};
  CHECK(find_owner32(pos32, 3, 0) == 0 && find_owner32(pos32, 3, 2) == 0 && find_owner32(pos32, 3, 3) == 2, "find_owner32");
}

static std::vector<Bytes> split(const std::string& s) {
  std::vector<Bytes> out;
  std::istringstream in(s);
  std::string w;
  while (in >> w) out.push_back(bytes_of(w));
  return out;
}

static void hard_coded() {
  const std::string G = "\xC4\xA0", U = "\xE2\x96\x81";
  // the trim
  CHECK(needle_skip((const uint8_t*)G.data(), 2) == 0, "a word of only trimmed chars is its own needle");
  CHECK(needle_skip((const uint8_t*)(G + G + "a").data(), 5) == 4 && needle_skip((const uint8_t*)U.data(), 3) == 0 &&
            needle_skip((const uint8_t*)(G + U + "a").data(), 6) == 5 && needle_skip((const uint8_t*)"\xC4", 1) == 0 &&
            needle_skip((const uint8_t*)"", 0) == 0 && needle_skip((const uint8_t*)("a" + G).data(), 3) == 0,
        "needle_skip");
  // lowercased "Hello hello hello": the first word finds the second hello, the third misses and falls back
  {
    std::vector<Span> s;
    uint64_t work = 0;
    CHECK(hd_words(bytes_of("Hello hello hello"), split("hello hello hello"), &s, &work) == -1 && s.size() == 3 && s[0].start == 6 &&
              s[0].end == 11 && s[1].start == 12 && s[1].end == 17 && s[2].start == 17 && s[2].end == 17 && work == 11 + 6 + 0,
          "the lowercase case");
  }
  check_sequence(bytes_of("a a a"), split("a a a"), nullptr, 0, 0);
  check_sequence(bytes_of("\xC3\xA9\xE2\x82\xAC"), {bytes_of("\xC3\x83\xC2\xA9\xC3\xA2\xC4\xA4\xC2\xAC")}, nullptr, 0, 0);
  // a fallback that ends inside a char: the last word does not panic, a word after it does, at byte 4
  {
    std::vector<Span> s;
    uint64_t work = 0;
    const Bytes o = bytes_of("\xC3\xA9\xE2\x82\xAC");
    CHECK(hd_words(o, {bytes_of("xxxx")}, &s, &work) == -1 && s[0].end == 4, "no panic at the last word");
    s.clear();
    CHECK(hd_words(o, {bytes_of("xxxx"), bytes_of("y")}, &s, &work) == 4, "byte index 4 is not a char boundary");
  }
  check_sequence(bytes_of(""), {Bytes()}, nullptr, 0, 0);
  check_sequence(bytes_of("ab"), {bytes_of("ab"), bytes_of("c"), bytes_of("d")}, nullptr, 0, 0);  // search_start == len with words to come
  // windows: a hit at 0, 63, 64, 65 and 127; needles of 1, 63, 64, 65 and 200 bytes; the completion past the end
  for (size_t at : {0u, 63u, 64u, 65u, 127u})
    for (size_t m : {1u, 63u, 64u, 65u, 200u}) {
      std::string o(at, 'x'), needle(m, 'q');
      needle[m - 1] = 'r';
      check_sequence(bytes_of(o + needle), {bytes_of(needle)}, nullptr, 0, 0);            // ends exactly at the end
      check_sequence(bytes_of(o + needle.substr(0, m - 1)), {bytes_of(needle)}, nullptr, 0, 0);  // one byte short
      check_sequence(bytes_of(o + needle.substr(0, m - 1) + "z" + needle + needle), {bytes_of(needle)}, nullptr, 0, 0);
    }
  check_sequence(bytes_of(std::string(70, 'a') + "ab" + std::string(10, 'a') + "ab"), {bytes_of("ab")}, nullptr, 0, 0);
  // the spans: a token longer than its word, tokens of no bytes, a word of no bytes
  check_tokens(3, 8, {6, 2}, nullptr);
  check_tokens(3, 8, {0, 2, 0, 0, 9, 1}, nullptr);
  check_tokens(5, 5, {1, 2}, nullptr);
  check_tokens(0, 1ull << 40, {1ull << 32, 5, 1ull << 39, 1ull << 39}, nullptr);
  check_rows();
}

int main(int argc, char** argv) {
  hard_coded();
  size_t n_seq = 0, n_words = 0;
  if (argc > 1) {
    std::ifstream f(argv[1]);
    if (!f) {
      std::printf("cannot open %s\n", argv[1]);
      return 1;
    }
    std::string tag;
    while (f >> tag) {
      if (tag == "S") {
        std::string o;
        size_t n;
        long long panic, work;
        f >> o >> n >> panic >> work;
        std::vector<Bytes> words;
        std::vector<Span> want;
        for (size_t i = 0; i < n; i++) {
          std::string w, h;
          Span sp;
          f >> w >> h >> sp.start >> sp.end;
          words.push_back(unhex(h));
          want.push_back(sp);
        }
        if (panic >= 0) {  // the listed words do not panic; one more word does
          words.push_back(bytes_of("z"));
        }
        check_sequence(unhex(o), words, &want, panic, work);
        n_seq++;
        n_words += n;
      } else if (tag == "T") {
        uint64_t ws, we;
        size_t n;
        f >> ws >> we >> n;
        std::vector<uint64_t> lens(n);
        std::vector<Span> want(n);
        for (auto& l : lens) f >> l;
        for (auto& s : want) f >> s.start >> s.end;
        check_tokens(ws, we, lens, &want);
      } else {
        std::printf("bad record %s\n", tag.c_str());
        return 1;
      }
    }
  }
  if (g_fail) return 1;
  std::printf("ok (%zu sequences, %zu words from the case file)\n", n_seq, n_words);
  return 0;
}
