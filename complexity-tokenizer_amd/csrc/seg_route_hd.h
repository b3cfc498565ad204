// k_segment: the tile's doc-start bits by piece number.  Plain integer code for the device and the
// host alike (checked on the host by tools/seg_route_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SEG_RT_HD __host__ __device__ __forceinline__
#else
#define SEG_RT_HD inline
#endif

namespace seg {

// Doc-start bits of one word by piece number.  st: the word's piece starts; D: its doc starts
// (only D & st counts); prew: the tile's pieces before the word.  Calls set(j) for every piece j
// of the word whose start is a doc start.
template <class F>
SEG_RT_HD void doc_pieces(uint64_t st, uint64_t D, uint32_t prew, F set) {
  for (uint64_t m = D & st; m; m &= m - 1ull) {
    const uint64_t below = (m & (0ull - m)) - 1ull;  // the bits under m's lowest
    set(prew + (uint32_t)__builtin_popcountll(st & below));
  }
}

}  // namespace seg
