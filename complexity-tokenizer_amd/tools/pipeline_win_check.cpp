// Host-side check of csrc/pipeline_win_hd.h: the closed forms the kernels of PipelineTokenizer's padded
// batches and stride windows use, against a literal walk of Encoding::truncate, truncate_with_stride and
// pad (src/encoding.rs:87-223) over lists that are kept as (first, one past last) views of a row's
// positions.  Every P, n <= P, m and stride in 0..40, each padding target in {0, m, 7, 45}.  A stand-alone
// program: no device, no library.
//   g++ -std=c++17 -O2 tools/pipeline_win_check.cpp -o pipeline_win_check && ./pipeline_win_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pipeline_win_hd.h"

namespace {

struct View {
  uint64_t a = 0, e = 0;  // list[a .. e)
  uint64_t size() const { return e - a; }
};

struct Enc {
  View ids, tokens, lists;  // lists: offsets, word_ids and sequence_ids before the padding
  uint64_t pad = 0;         // None entries that pad added to sequence_ids, and padding ids
};

struct Result {
  std::vector<Enc> windows;  // the main encoding, then its overflowing list
  bool panicked = false;
  uint64_t panic_end = 0, panic_len = 0;
};

// Rust `v[a..b]` of a list of len entries
bool slice(uint64_t len, uint64_t a, uint64_t b, View* out, Result* r) {
  if (b > len || a > b) {
    r->panicked = true;
    r->panic_end = b;
    r->panic_len = len;
    return false;
  }
  *out = View{a, b};
  return true;
}

View opt(uint64_t len, uint64_t a, uint64_t e) { return len > a ? View{a, std::min(e, len)} : View{}; }

Enc whole(uint64_t P, uint64_t t, uint64_t n) { return Enc{View{0, P}, View{0, t}, View{0, n}, 0}; }

void cut_main(Enc* e, uint64_t m) {
  e->ids.e = std::min(e->ids.e, m);
  e->tokens.e = std::min(e->tokens.e, m);
  e->lists.e = std::min(e->lists.e, m);
}

// Encoding::truncate: the remainder is sliced first (and dropped by the caller), then the main encoding is cut
Result truncate(uint64_t P, uint64_t t, uint64_t n, uint64_t m) {
  Result r;
  Enc e = whole(P, t, n);
  if (P > m) {
    Enc over;
    if (!slice(P, m, P, &over.ids, &r) || !slice(t, m, t, &over.tokens, &r)) return r;
    cut_main(&e, m);
  }
  r.windows.push_back(e);
  return r;
}

// Encoding::truncate_with_stride
Result truncate_with_stride(uint64_t P, uint64_t t, uint64_t n, uint64_t m, uint64_t stride) {
  Result r;
  Enc e = whole(P, t, n);
  std::vector<Enc> over;
  if (P > m) {
    uint64_t pos = m;
    while (pos < P) {
      const uint64_t start = pos > stride ? pos - stride : 0;
      const uint64_t end = std::min(start + m, P);
      Enc o;
      if (!slice(P, start, end, &o.ids, &r) || !slice(t, start, end, &o.tokens, &r)) return r;
      o.lists = opt(n, start, end);
      over.push_back(o);
      pos = end;
    }
    cut_main(&e, m);
  }
  r.windows.push_back(e);
  r.windows.insert(r.windows.end(), over.begin(), over.end());
  return r;
}

void pad(Enc* e, uint64_t target) {
  if (e->ids.size() < target) e->pad = target - e->ids.size();
}

#define CHECK(c)                                                                                                        \
  do {                                                                                                                  \
    if (!(c)) {                                                                                                         \
      std::printf("FAIL %s: mode %u P %llu t %llu m %llu stride %llu target %llu (line %d)\n", #c, mode, (unsigned long long)P, \
                  (unsigned long long)t, (unsigned long long)m, (unsigned long long)s, (unsigned long long)target, __LINE__);   \
      std::exit(1);                                                                                                     \
    }                                                                                                                   \
  } while (0)

uint64_t check(uint32_t mode, uint64_t P, uint64_t t, uint64_t m, uint64_t s) {
  uint64_t target = 0;
  const uint64_t n = t;  // with special tokens the lists are as long as `tokens`; check_tokens varies t alone
  Result r = mode == pwin::kWindows ? truncate_with_stride(P, t, n, m, s) : mode == pwin::kCut ? truncate(P, t, n, m) : Result{{whole(P, t, n)}};
  CHECK(pwin::panics(mode, P, t, m) == r.panicked);
  if (r.panicked) {
    CHECK(pwin::panic_end(mode, P, t, m, s) == r.panic_end && r.panic_len == t);
    return 0;
  }
  CHECK(pwin::count(mode, P, m, s) == r.windows.size());
  CHECK(pwin::main_len(mode, P, m) == r.windows[0].ids.size());
  for (uint64_t tg : {(uint64_t)0, m, (uint64_t)7, (uint64_t)45}) {
    target = tg;
    for (uint64_t k = 0; k < r.windows.size(); k++) {
      Enc e = r.windows[k];
      if (!k) pad(&e, target);
      const uint64_t a = pwin::start(k, m, s), b = pwin::end(mode, k, P, m, s);
      CHECK(a == e.ids.a && b == e.ids.e);
      CHECK(pwin::list_len(n, a, b) == e.lists.size() && (e.lists.size() == 0 || e.lists.a == a));
      CHECK(pwin::enc_len(k, b - a, target) == e.ids.size() + e.pad);
      CHECK(pwin::list_len(n, a, b) + (pwin::enc_len(k, b - a, target) - (b - a)) == e.lists.size() + e.pad);
    }
  }
  return r.windows.size();
}

// Encoding::from_ids rows: `tokens` is shorter than the lists (P = n ids, t <= n tokens)
void check_tokens(uint32_t mode, uint64_t P, uint64_t t, uint64_t m, uint64_t s) {
  const uint64_t target = 0;
  Result r = mode == pwin::kWindows ? truncate_with_stride(P, t, P, m, s) : truncate(P, t, P, m);
  CHECK(pwin::panics(mode, P, t, m) == r.panicked);
  if (r.panicked) CHECK(pwin::panic_end(mode, P, t, m, s) == r.panic_end && r.panic_len == t);
}

}  // namespace

int main() {
  constexpr uint64_t N = 40;
  uint64_t rows = 0, windows = 0;
  for (uint64_t P = 0; P <= N; P++) {
    for (uint64_t t = 0; t <= P; t++) {
      for (uint64_t m = 0; m <= N; m++) {
        windows += check(pwin::kNone, P, t, m, 0);
        windows += check(pwin::kCut, P, t, m, 0);
        check_tokens(pwin::kCut, P, t, m, 0);
        rows += 2;
        for (uint64_t s = 0; s <= N; s++) {
          if (!pwin::valid(pwin::kWindows, m, s)) {
            if (s < m) {
              std::printf("FAIL valid: m %llu stride %llu\n", (unsigned long long)m, (unsigned long long)s);
              return 1;
            }
            continue;
          }
          windows += check(pwin::kWindows, P, t, m, s);
          check_tokens(pwin::kWindows, P, t, m, s);
          rows++;
        }
      }
    }
  }
  std::printf("rows ok: %llu\n", (unsigned long long)rows);
  std::printf("windows ok: %llu\n", (unsigned long long)windows);
  std::printf("all ok\n");
  return 0;
}
