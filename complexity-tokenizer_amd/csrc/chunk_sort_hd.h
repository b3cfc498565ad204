// The length order of a merge-pass chunk (kernels.hip, class_pass), shared with the host-side check
// in tests (tools/chunk_sort_check.cpp): integer code only.
//
// A pass gives one piece to a thread, and every loop of a piece is divergent per lane: a wavefront
// runs its slowest lane's trip count.  The packed and register tiers run n - N / 2 steps on a piece
// of n bytes (a 9..32 B piece ends well below the tier's stop), merge_lds8 about one step per byte,
// so a wavefront whose 64 pieces have one byte length idles no lane in them.  The chunk's first
// SORTCAP list entries are therefore counting-sorted by a bucket of the byte length, and the waves
// take blocks of 64 in that order; entries past SORTCAP follow in list order.
//
// Bucket rules of a pass of N slots (class lengths N / 2 + 1 .. N; 1 .. 8 at N = 8):
//   exact    N = 16: one bucket per length 9..16 (8); N = 32: one per length 17..32 (16);
//            N = 8: lengths <= 5, 6, 7, 8 (4: 2 % of the class is below 5 B on C4)
//   coarse   four buckets of width 2 (N = 8, 16), 4 (N = 32), 8 (N = 64): the rule before the
//            exact one, kept as the A/B arm; the only rule at N = 64
// The walk order is a parameter: a bucket's code is its place in the walk, so the sort itself is
// always ascending in the code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CSORT_HD __host__ __device__ __forceinline__
#else
#define CSORT_HD inline
#endif

namespace csort {

constexpr uint32_t kMaxBuckets = 16;

// Work::chunk_sort (CTOK_CHUNK_SORT): bits 0..2 the exact rule for the <= 8 B, 9..16 B and 17..32 B
// pass (clear: the <= 8 B pass walks in list order, the other two use the coarse rule); bit 3
// shortest bucket first (clear: longest first, the short merge chains at the chunk's barrier).
// The default is what the A/B on C4 kept (profiles/chunk_sort/ab_summary.txt): exact order in the
// 9..16 B and 17..32 B passes, longest first.  The <= 8 B pass stays in list order: sorted, it
// issues 13 % fewer VALU instructions in the same time (its waves wait more instead), and pays
// for the sort.
constexpr uint32_t kExact8 = 1u, kExact16 = 2u, kExact32 = 4u, kAscending = 8u;
constexpr uint32_t kModeMask = 15u;
constexpr uint32_t kModeDefault = kExact16 | kExact32;

// the mode bit of the pass of N slots (none at N = 64: always coarse)
CSORT_HD constexpr uint32_t exact_bit(int N) { return N == 8 ? kExact8 : N == 16 ? kExact16 : N == 32 ? kExact32 : 0u; }
// is the chunk sorted at all?  (coarse at N = 8 is the unsorted arm)
CSORT_HD constexpr bool sorts(int N, uint32_t mode) { return N != 8 || (mode & kExact8) != 0; }
CSORT_HD constexpr bool exact(int N, uint32_t mode) { return (mode & exact_bit(N)) != 0; }

CSORT_HD constexpr uint32_t class_lo(int N) { return N == 8 ? 1u : (uint32_t)N / 2 + 1; }
CSORT_HD constexpr uint32_t coarse_shift(int N) { return N == 64 ? 3u : N == 32 ? 2u : 1u; }  // widths 8, 4, 2

CSORT_HD constexpr uint32_t n_buckets(int N, bool ex) { return !ex ? 4u : N == 16 ? 8u : N == 32 ? 16u : 4u; }

// the bucket of a piece of n bytes, ascending in n (a length outside the class, which no list
// holds, takes the nearest bucket: the result always indexes n_buckets counters)
CSORT_HD uint32_t bucket(int N, bool ex, uint32_t n) {
  const uint32_t lo = ex && N == 8 ? 5u : class_lo(N), nb = n_buckets(N, ex);
  const uint32_t b = (n < lo ? 0u : n - lo) >> (ex ? 0u : coarse_shift(N));
  return b < nb ? b : nb - 1u;
}

// the sort key: the bucket's place in the walk
CSORT_HD uint32_t code(int N, uint32_t mode, uint32_t n) {
  const bool ex = exact(N, mode);
  const uint32_t b = bucket(N, ex, n);
  return (mode & kAscending) ? b : n_buckets(N, ex) - 1u - b;
}

}  // namespace csort
