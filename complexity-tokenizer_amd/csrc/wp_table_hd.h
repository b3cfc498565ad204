// The string table of the WordPiece kernels (wordpiece.hip k_wp_match), shared with the host
// (wordpiece_host.cpp builds it) and the CPU check (tools/wp_table_check.cpp): plain integer code,
// no HIP include, no intrinsics.
//
// A vocab string V gives up to two patterns (include/ctok_wordpiece.h): V itself in form 0 (at a
// word's first char) and V without the continuing-subword prefix in form 1 (at any later char).
// The table maps (form, bytes) -> symbol: open addressing with linear probing over a byte blob.
// A slot holds the pattern's place in the blob, its length, its symbol and a tag (31 hash bits and
// the form); len 0 is an empty slot.  Insertion and lookup look at no more than kMaxProbe slots, so
// a lookup is bounded and ends early at an empty slot; build() doubles the capacity until every
// pattern is within the bound and reports a table that cannot be built instead of spinning.
//
// The hash is FNV-1a over the bytes, so a position hashes its code points incrementally and probes
// once per code-point boundary (longest()).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define WPT_HD __host__ __device__ __forceinline__
#else
#define WPT_HD inline
#endif

namespace wptab {

constexpr uint32_t kMaxProbe = 32;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // no symbol
constexpr uint32_t kSeed = 2166136261u;

struct Slot {
  uint32_t off;  // pattern = blob[off .. off + len)
  uint32_t len;  // 0: empty
  uint32_t sym;
  uint32_t tag;  // fin(hash, form) with the form in bit 0
};

struct View {
  const Slot* slots;
  const uint8_t* blob;
  uint32_t mask;     // capacity - 1 (a power of two)
  uint32_t max_len;  // bytes of the longest pattern
};

struct Match {
  uint32_t sym;  // kNone: nothing matches
  uint32_t len;  // bytes
};

WPT_HD uint32_t step(uint32_t h, uint8_t b) { return (h ^ b) * 16777619u; }

WPT_HD uint32_t fin(uint32_t h, uint32_t form) {
  h ^= h >> 15;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return (h & ~1u) | (form & 1u);
}

WPT_HD bool bit_at(const uint32_t* bits, uint64_t g) { return (bits[g >> 5] >> (g & 31)) & 1u; }

// bytes of the code point with lead byte b (a stray continuation byte counts as one)
WPT_HD uint32_t cp_len(uint8_t b) { return b < 0xC0u ? 1u : b < 0xE0u ? 2u : b < 0xF0u ? 3u : 4u; }

// the symbol of pattern p[0 .. len) in `form`, h = the FNV-1a hash of its bytes; kNone if absent
WPT_HD uint32_t find(const View& v, const uint8_t* p, uint32_t len, uint32_t h, uint32_t form) {
  const uint32_t tag = fin(h, form);
  uint32_t s = (tag >> 1) & v.mask;
  for (uint32_t i = 0; i < kMaxProbe; i++) {
    const Slot e = v.slots[s];
    if (!e.len) return kNone;
    if (e.tag == tag && e.len == len) {
      const uint8_t* q = v.blob + e.off;
      uint32_t j = 0;
      while (j < len && q[j] == p[j]) j++;
      if (j == len) return e.sym;
    }
    s = (s + 1) & v.mask;
  }
  return kNone;
}

// The longest pattern of `form` that starts at byte p (a code-point start, p < n) and ends inside
// p's word: the word ends at n or at the first set bit of starts behind p (starts: a bit per text
// byte, set at every word's first byte; may be null for one word).  Reads no byte at or past n and
// looks at no more than max_len bytes.
WPT_HD Match longest(const View& v, const uint8_t* text, uint64_t n, const uint32_t* starts, uint64_t p,
                     uint32_t form) {
  Match m = {kNone, 0};
  uint32_t h = kSeed;
  uint64_t q = p;
  while (q < n) {
    const uint32_t l = cp_len(text[q]);
    if (q + l > n || q + l - p > v.max_len) break;
    for (uint32_t j = 0; j < l; j++) h = step(h, text[q + j]);
    q += l;
    const uint32_t s = find(v, text + p, (uint32_t)(q - p), h, form);
    if (s != kNone) m = Match{s, (uint32_t)(q - p)};
    if (q < n && starts && bit_at(starts, q)) break;
  }
  return m;
}

// ---- host: building ----------------------------------------------------------------------------------

struct Pattern {
  const uint8_t* p;
  uint32_t len;  // >= 1
  uint32_t form;
  uint32_t sym;
};

struct Built {
  std::vector<Slot> slots;
  std::vector<uint8_t> blob;
  uint32_t max_len = 0;
  View view() const { return View{slots.data(), blob.data(), (uint32_t)slots.size() - 1, max_len}; }
};

inline uint32_t hash_of(const uint8_t* p, uint32_t len) {
  uint32_t h = kSeed;
  for (uint32_t j = 0; j < len; j++) h = step(h, p[j]);
  return h;
}

constexpr int kOk = 0, kDuplicate = -1, kFull = -2, kEmptyPattern = -3;

// 0, or why the table cannot be built: two patterns equal in form and bytes with different
// symbols, an empty pattern, or no capacity up to 2^28 slots keeps every probe within kMaxProbe.
// An equal pattern with the same symbol is stored once.
inline int build(const std::vector<Pattern>& pats, Built* out) {
  uint64_t bytes = 0;
  out->max_len = 0;
  for (const auto& x : pats) {
    if (!x.len) return kEmptyPattern;
    bytes += x.len;
    if (x.len > out->max_len) out->max_len = x.len;
  }
  if (bytes >= 0xFFFFFFFFull) return kFull;
  uint64_t cap = 16;
  while (cap < 2 * (uint64_t)pats.size()) cap <<= 1;
  for (; cap <= (1ull << 28); cap <<= 1) {
    out->slots.assign(cap, Slot{0, 0, 0, 0});
    out->blob.clear();
    out->blob.reserve(bytes + 1);
    const uint32_t mask = (uint32_t)cap - 1;
    bool full = false;
    for (const auto& x : pats) {
      const uint32_t tag = fin(hash_of(x.p, x.len), x.form);
      uint32_t s = (tag >> 1) & mask, i = 0;
      bool same = false;
      for (; i < kMaxProbe; i++) {
        Slot& e = out->slots[s];
        if (!e.len) {
          e = Slot{(uint32_t)out->blob.size(), x.len, x.sym, tag};
          out->blob.insert(out->blob.end(), x.p, x.p + x.len);
          break;
        }
        if (e.tag == tag && e.len == x.len && !std::memcmp(out->blob.data() + e.off, x.p, x.len)) {
          if (e.sym != x.sym) return kDuplicate;
          same = true;
          break;
        }
        s = (s + 1) & mask;
      }
      if (i == kMaxProbe && !same) {
        full = true;
        break;
      }
    }
    if (!full) {
      out->blob.push_back(0);  // (never empty: the device copy has a byte to point at)
      return kOk;
    }
  }
  return kFull;
}

}  // namespace wptab
