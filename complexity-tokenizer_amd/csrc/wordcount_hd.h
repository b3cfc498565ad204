// Pure functions of the trainer's device word counting (wordcount.hip), shared with the host-side
// check in tests (tools/wordcount_check.cpp): plain integer code, no intrinsics.
//
// A word is identified by reference into the chunk's text, which is immutable and resident while
// the chunk is counted.  A table slot is ONE 64-bit descriptor, written once by a compare-and-swap
// from kEmpty and never changed afterwards:
//     bits 63..32  text position of the word's first occurrence (a call is < 3.75 GiB: 32 bits)
//     bits 31..16  its length in bytes, clipped to kLenClip (0xFFFF = "kLenClip or longer")
//     bits 15..0   tag: the low 16 bits of the word's hash
// A probe compares tag and clipped length with one 32-bit compare, then the bytes against the
// first occurrence; a clipped length is settled by the piece-start bitmap (wordcount.hip).  No
// position is 0xFFFFFFFF, so no descriptor equals kEmpty.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define WC_HD __host__ __device__ __forceinline__
#else
#define WC_HD inline
#endif

namespace wc {

constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kLenClip = 0xFFFFu;
constexpr uint32_t kHashBytes = 256;  // the hash reads a word's first kHashBytes bytes (and its length)

WC_HD uint32_t clip_len(uint64_t len) { return len < kLenClip ? (uint32_t)len : kLenClip; }
WC_HD uint64_t pack(uint32_t pos, uint32_t len_clipped, uint32_t tag) {
  return ((uint64_t)pos << 32) | ((uint64_t)(len_clipped & 0xFFFFu) << 16) | (tag & 0xFFFFu);
}
WC_HD uint32_t pos_of(uint64_t d) { return (uint32_t)(d >> 32); }
WC_HD uint32_t len_of(uint64_t d) { return (uint32_t)(d >> 16) & 0xFFFFu; }
WC_HD uint32_t tag_of(uint64_t d) { return (uint32_t)d & 0xFFFFu; }
// same tag and same clipped length (the bytes still have to be compared)
WC_HD bool may_match(uint64_t d, uint32_t len_clipped, uint32_t tag) { return (uint32_t)d == (uint32_t)pack(0, len_clipped, tag); }

// Bytes p .. p + 3 of the text as a little-endian dword, by two aligned dword loads: text must be
// 4-byte aligned and readable through byte (p & ~3) + 7 (the device text buffers end in 16 spare
// bytes).
WC_HD uint32_t load4(const uint8_t* text, uint64_t p) {
  const uint64_t a = p & ~3ull;
  uint32_t lo, hi;
#if defined(__HIP_DEVICE_COMPILE__)
  lo = *reinterpret_cast<const uint32_t*>(text + a);
  hi = *reinterpret_cast<const uint32_t*>(text + a + 4);
#else
  std::memcpy(&lo, text + a, 4);
  std::memcpy(&hi, text + a + 4, 4);
#endif
  const uint32_t sh = 8u * (uint32_t)(p & 3);
  return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
}

// the low rem (1..3) bytes of v
WC_HD uint32_t tail_mask(uint32_t v, uint64_t rem) { return v & ((1u << (8u * (uint32_t)rem)) - 1u); }

// 64-bit hash of the word text[p .. p + len): bits 63..32 choose the global slot, bits 31..16 the
// workgroup's LDS slot, bits 15..0 are the tag.
WC_HD uint64_t word_hash(const uint8_t* text, uint64_t p, uint64_t len) {
  uint64_t h = 0x243F6A8885A308D3ull ^ (len * 0xD6E8FEB86659FD93ull);
  const uint64_t n = len < kHashBytes ? len : kHashBytes;
  for (uint64_t i = 0; i < n; i += 4) {
    uint32_t v = load4(text, p + i);
    if (n - i < 4) v = tail_mask(v, n - i);
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h;
}

// text[p .. p + len) == text[r .. r + len); both ranges must lie inside the text
WC_HD bool words_equal(const uint8_t* text, uint64_t p, uint64_t r, uint64_t len) {
  if (p == r) return true;
  for (uint64_t i = 0; i < len; i += 4) {
    uint32_t a = load4(text, p + i), b = load4(text, r + i);
    if (len - i < 4) {
      a = tail_mask(a, len - i);
      b = tail_mask(b, len - i);
    }
    if (a != b) return false;
  }
  return true;
}

}  // namespace wc
