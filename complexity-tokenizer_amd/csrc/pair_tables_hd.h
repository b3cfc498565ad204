// The format of the pair tables (merge table, LDS images, narrow tables) and of the whole-piece
// table: entry layouts, hashes and sizes.  Shared by the kernels that read the tables
// (pair_lookup_dev.h, segment.hip, long.hip), the table compiler that writes them
// (table_compile.cpp) and its host-side check (tools/table_compile_check.cpp): integer code only,
// no HIP header.  In a HIP translation unit it is included after hip_runtime.h (ctok_internal.h).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PTAB_HD __host__ __device__ inline
#else
#define PTAB_HD inline
#endif

namespace ctok_dev {

// Merge table entry (u64): bits [0,21) = right id, [21,42) = left id, [42,64) = rank.
// Token ids must be < 2^21 - 1; ranks < 2^22 - 2.  All-ones = empty slot.
constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kIdBits = 21;
constexpr uint64_t kKeyMask = (1ull << 42) - 1;
constexpr uint32_t kNoRank = 0x3FFFFFu;      // "no merge" (22-bit all ones)
constexpr uint32_t kMaxId = (1u << kIdBits) - 2;
constexpr uint32_t kPanicVal = kNoRank - 1;  // compact-table value of an entry whose lookup panics

// 24-bit multiply (v_mul_u32_u24: full rate; a 32-bit v_mul_lo_u32 is quarter rate on CDNA)
PTAB_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#endif
}

// Merge-table hashes of a pair (a, b) of token ids (< 2^21): mhash picks the global table slot
// (open addressing) and, with mhash2, the two candidate buckets of the LDS hot table and the two
// Bloom-filter bits.  Built from 24-bit multiplies and shift-xors only.
PTAB_HD uint32_t mhash(uint32_t a, uint32_t b) {
  uint32_t h = mul24(a, 0x9E3779u) + mul24(b ^ 0x5A5A5Au, 0x85EBCBu);
  h ^= h >> 15;
  h = mul24(h, 0xC2B2AFu) ^ (h >> 9);
  return h ^ (h >> 16);
}
PTAB_HD uint32_t mhash2(uint32_t h1) {
  uint32_t h = mul24(h1 ^ (h1 >> 24), 0x27D4EBu) + (h1 >> 11);
  h ^= h >> 13;
  h = mul24(h, 0x165667u) ^ (h >> 8);
  return h ^ (h >> 16);
}

// LDS image for the merge passes (loaded once per workgroup): a hot table of the lowest-rank
// mergeable pairs, kHotBuckets buckets of two merge-table entries, a pair in bucket
// mhash & mask or mhash2 & mask; and a Bloom filter over the merge-table entries that are not in
// the hot table (bits (mhash >> 12) and (mhash2 >> 12) mod kBloomBits).  A pair found in neither
// LDS structure goes to the global table only when both Bloom bits are set.  A second filter over
// every entry follows the image in memory, for the kernels that load the filter alone.
constexpr uint32_t kHotBuckets = 4096;                 // 64 KiB
constexpr uint32_t kBloomBits = 1u << 18;              // 32 KiB
constexpr uint32_t kHotU64 = 2 * kHotBuckets;
constexpr uint32_t kBloomWords = kBloomBits / 32;
constexpr uint32_t kLdsImageBytes = kHotU64 * 8 + kBloomWords * 4;

// Narrow vocabularies (every id < 2^16, Tables::narrow): the register merge passes use a second
// set of pair tables keyed by the 32-bit pair key a << 16 | b, whose lookups cost about half the
// VALU of the 42-bit ones above.  Entries are u64 value << 32 | key; ~0 = empty (no id is 0xFFFF).
//   LDS image (kLdsImageBytes): hot table of kHotBuckets buckets of two entries, a pair in bucket
//   hash16_h >> 20 or hash16_g >> 20; then a Bloom filter (kBloomBits) over the other entries,
//   bits hash16_h & (kBloomBits - 1) and hash16_g >> 14.
//   Global table (merge16, load <= 1/8): open addressing from hash16_h & mask.
PTAB_HD uint32_t key16(uint32_t a, uint32_t b) { return (a << 16) | b; }
PTAB_HD uint32_t hash16_h(uint32_t a, uint32_t b) {
  const uint32_t h = mul24(a, 0x9E3779u) + mul24(b, 0x85EBCBu);
  return h ^ (h >> 13);
}
PTAB_HD uint32_t hash16_g(uint32_t a, uint32_t b) {
  return mul24(b, 0xC2B2AFu) + mul24(a ^ 0x5A5Au, 0x27D4EBu);
}

// Whole-piece table: raw byte strings of <= 8 bytes whose BPE is exactly one token (checked at
// load time by running the merge loop on every vocab entry).  Entry = {lo32, hi32, len, id} of
// the zero-padded bytes; len == 0 marks an empty slot.
PTAB_HD uint32_t piece_hash(uint32_t lo, uint32_t hi, uint32_t len) {
  uint32_t h = mul24(lo, 0x9E3779u) + mul24((lo >> 24) | (hi << 8), 0x85EBCBu) + mul24((hi >> 16) | (len << 16), 0xC2B2AFu);
  h ^= h >> 15;
  h = mul24(h, 0x27D4EBu) ^ (h >> 9);
  return h ^ (h >> 16);
}

}  // namespace ctok_dev
