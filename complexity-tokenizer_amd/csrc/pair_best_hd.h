// The order in which the classic BPE trainer picks its next merge (bpe_train.hip k_pair_best),
// shared with the host (bpe_train_host.cpp) and the CPU check (tools/pair_best_check.cpp): plain
// integer code, no HIP include.
//
// A candidate is (count, key) with key = symbol id of first << 32 | symbol id of second.  The
// largest count wins; among equal counts the smallest key, i.e. the smallest (first, second) pair
// of symbol ids (the reference's max_by_key over a HashMap leaves ties to hash order,
// src/bpe_trainer.rs:152-155).  A count <= 0 never wins: kNone is what a search over no live pair
// returns.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PB_HD __host__ __device__ __forceinline__
#else
#define PB_HD inline
#endif

namespace pbest {

struct Cand {
  int64_t count;
  uint64_t key;
};

constexpr Cand kNone = {0, ~0ull};

// x is chosen before y
PB_HD bool better(const Cand& x, const Cand& y) {
  if (x.count <= 0) return false;
  if (y.count <= 0) return true;
  return x.count != y.count ? x.count > y.count : x.key < y.key;
}

PB_HD Cand best_of(const Cand& x, const Cand& y) { return better(y, x) ? y : x; }

PB_HD uint64_t pair_key(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | b; }

}  // namespace pbest
