// The pair table and the scalar merge loop of the string-keyed merge engine (strmerge.hip), shared
// with the host (strmerge_compile.cpp builds the table) and the CPU check (tools/strmerge_check.cpp):
// plain integer code, no HIP include, no intrinsics.
//
// A token is a symbol: the index of its string among the model's interned strings (strmerge_compile.h).
// The table maps (symA, symB) -> (rank, sym(A + B)): open addressing with linear probing, read-only
// after the build.  Insertion and lookup look at no more than kPairProbe slots, so a lookup is
// bounded and ends early at an empty slot; the builder doubles the capacity until every pair is
// within the bound.  The foreign symbol (strmerge_compile.h) is in no pair, so it never merges.
//
// merge_word is the reference's loop (src/models.rs:487-514, :662-689) as it stands: every step
// takes the pair with the lowest rank, the leftmost among equals, and merges that one occurrence.
// After a merge only the two neighbouring pairs are looked up again; the other cached ranks still
// belong to the pairs they were read for.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SM_HD __host__ __device__ __forceinline__
#else
#define SM_HD inline
#endif

namespace strmerge {

constexpr uint32_t kPairProbe = 32;
constexpr uint32_t kNoRank = 0xFFFFFFFFu;  // no merge for the pair; also an empty slot's `a`
constexpr uint32_t kDead = 0xFFFFFFFFu;    // a position whose token went into its left neighbour

struct PairSlot {
  uint32_t a;  // kNoRank: empty
  uint32_t b;
  uint32_t rank;
  uint32_t sym;  // the symbol of the string a + b
};

struct PairView {
  const PairSlot* slots;
  uint32_t mask;  // capacity - 1 (a power of two)
};

struct Merge {
  uint32_t rank;  // kNoRank: the pair has no merge
  uint32_t sym;
};

SM_HD uint32_t pair_slot(uint32_t a, uint32_t b, uint32_t mask) {
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0xC2B2AE35u;
  h ^= h >> 13;
  return h & mask;
}

SM_HD Merge pair_find(const PairView& v, uint32_t a, uint32_t b) {
  uint32_t s = pair_slot(a, b, v.mask);
  for (uint32_t i = 0; i < kPairProbe; i++) {
    const PairSlot e = v.slots[s];
    if (e.a == kNoRank) break;
    if (e.a == a && e.b == b) return Merge{e.rank, e.sym};
    s = (s + 1) & v.mask;
  }
  return Merge{kNoRank, 0};
}

// The merge loop over n tokens held at tok[i * stride], with room for n cached ranks at
// rank[i * stride] (rank[i]: the pair (tok[i], tok[i + 1])).  Returns the number of tokens left, in
// tok[0 .. ) in order.  At most n - 1 steps of at most n moves each.
SM_HD uint32_t merge_word(const PairView& v, uint32_t* tok, uint32_t* rank, uint32_t stride, uint32_t n) {
  for (uint32_t i = 0; i + 1 < n; i++) rank[i * stride] = pair_find(v, tok[i * stride], tok[(i + 1) * stride]).rank;
  while (n > 1) {
    uint32_t best = kNoRank, at = 0;
    for (uint32_t i = 0; i + 1 < n; i++) {
      const uint32_t r = rank[i * stride];
      if (r < best) best = r, at = i;  // (strictly: the leftmost of equal ranks stays)
    }
    if (best == kNoRank) break;
    tok[at * stride] = pair_find(v, tok[at * stride], tok[(at + 1) * stride]).sym;
    for (uint32_t i = at + 1; i + 1 < n; i++) {
      tok[i * stride] = tok[(i + 1) * stride];
      rank[i * stride] = rank[(i + 1) * stride];
    }
    n--;
    if (at + 1 < n) rank[at * stride] = pair_find(v, tok[at * stride], tok[(at + 1) * stride]).rank;
    if (at > 0) rank[(at - 1) * stride] = pair_find(v, tok[(at - 1) * stride], tok[at * stride]).rank;
  }
  return n;
}

}  // namespace strmerge
