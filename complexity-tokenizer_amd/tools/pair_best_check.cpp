// CPU check of csrc/pair_best_hd.h (the order in which the classic BPE trainer's k_pair_best picks
// the next merge) against cases written out by hand.  Build: g++ -O2 -std=c++17 pair_best_check.cpp
// -o pair_best_check; prints "ok" or the failing case.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/pair_best_hd.h"

using pbest::Cand;

static int fails = 0;
#define EXPECT(c)                                      \
  do {                                                 \
    if (!(c)) {                                        \
      printf("FAIL line %d: %s\n", __LINE__, #c);      \
      fails++;                                         \
    }                                                  \
  } while (0)

static Cand reduce(std::vector<Cand> v) {
  Cand c = pbest::kNone;
  for (const Cand& x : v) c = pbest::best_of(c, x);
  return c;
}

int main() {
  const uint64_t k12 = pbest::pair_key(1, 2), k13 = pbest::pair_key(1, 3), k21 = pbest::pair_key(2, 1);
  EXPECT(k12 == 0x0000000100000002ull);
  EXPECT(k12 < k13 && k13 < k21);  // (first, second) compares as the key does
  // a higher count wins, whatever the keys
  EXPECT(pbest::better(Cand{5, k21}, Cand{4, k12}));
  EXPECT(!pbest::better(Cand{4, k12}, Cand{5, k21}));
  // on equal counts the smaller key wins
  EXPECT(pbest::better(Cand{5, k12}, Cand{5, k13}));
  EXPECT(!pbest::better(Cand{5, k13}, Cand{5, k12}));
  EXPECT(pbest::better(Cand{5, k13}, Cand{5, k21}));
  // nothing is chosen before itself
  EXPECT(!pbest::better(Cand{5, k12}, Cand{5, k12}));
  // zero and negative counts never win, not against each other and not against kNone
  EXPECT(!pbest::better(Cand{0, k12}, Cand{0, k13}));
  EXPECT(!pbest::better(Cand{0, k12}, pbest::kNone));
  EXPECT(!pbest::better(Cand{-3, k12}, Cand{-7, k13}));
  EXPECT(!pbest::better(Cand{-3, k12}, Cand{1, k13}));
  EXPECT(pbest::better(Cand{1, k21}, Cand{0, k12}));
  EXPECT(pbest::better(Cand{1, k21}, Cand{-1, k12}));
  EXPECT(pbest::better(Cand{1, k21}, pbest::kNone));
  // counts past 2^32 compare as 64-bit numbers
  EXPECT(pbest::better(Cand{(int64_t)1 << 33, k21}, Cand{((int64_t)1 << 32) + 5, k12}));
  // a reduction in any order gives the same winner
  std::vector<Cand> v = {{3, k21}, {7, k13}, {0, 0}, {7, k12}, {-2, 1}, {7, k21}, {6, 0}};
  std::sort(v.begin(), v.end(), [](const Cand& x, const Cand& y) { return x.key != y.key ? x.key < y.key : x.count < y.count; });
  int perms = 0;
  do {
    const Cand c = reduce(v);
    EXPECT(c.count == 7 && c.key == k12);
    perms++;
  } while (perms < 2000 && std::next_permutation(v.begin(), v.end(), [](const Cand& x, const Cand& y) {
    return x.key != y.key ? x.key < y.key : x.count < y.count;
  }));
  // no live pair: the search reports count 0
  const Cand none = reduce({{0, k12}, {-1, k13}});
  EXPECT(none.count <= 0);
  EXPECT(reduce({}).count == 0);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
