// Lowercase as Rust's str::to_lowercase does it (the reference's Normalizer::Lowercase,
// src/normalizers.rs), shared by the kernels (lowercase.hip), the host and the CPU check
// (tools/lowercase_check.cpp): plain integer code, no HIP include, no intrinsics.
//
//   - every code point maps through the table (gen/lowercase_data.h, Unicode 13.0); only U+0130
//     maps to two code points, U+0069 U+0307;
//   - U+03A3 becomes U+03C2 (final sigma) when, skipping Case_Ignorable code points, a Cased one
//     precedes it and none follows it, else U+03C3.  A code point that is both cased and ignorable
//     is skipped like any ignorable one.
// The context of a sigma never leaves its text: every function takes the text's bounds [lo, hi)
// and reads no byte outside them, and both context loops are bounded by the text.
//
// The text is taken as UTF-8; a byte that starts no well-formed code point inside [lo, hi) is
// copied as it is (one byte), so the functions are total.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LC_HD __host__ __device__ __forceinline__
#else
#define LC_HD inline
#endif

namespace lowercase {

struct Tables {          // gen/lowercase_data.h (the device's copy in lowercase.hip)
  const uint32_t* from;  // ascending
  const uint32_t* to;
  uint32_t n_map;
  const uint32_t* cased;  // [first, last] pairs, ascending
  uint32_t n_cased;
  const uint32_t* ignorable;
  uint32_t n_ignorable;
};

constexpr uint32_t kRaw = 0xFFFFFFFFu;  // decode(): no code point, one raw byte

LC_HD bool is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// the code point that starts at byte p (lo <= p < hi) and its length; kRaw / 1 when none does
LC_HD uint32_t decode(const uint8_t* t, uint64_t hi, uint64_t p, uint32_t* len) {
  const uint8_t b = t[p];
  *len = 1;
  if (b < 0x80u) return b;
  const uint32_t l = (b >> 5) == 6 ? 2u : (b >> 4) == 14 ? 3u : (b >> 3) == 30 ? 4u : 0u;
  if (!l || l > hi - p) return kRaw;
  uint32_t c = b & (0xFFu >> (l + 1));
  for (uint32_t j = 1; j < l; j++) {
    if (!is_cont(t[p + j])) return kRaw;
    c = (c << 6) | (t[p + j] & 63u);
  }
  *len = l;
  return c;
}

// byte p of the text [lo, hi) starts a unit of decode(): a code point, or a raw byte no code point
// before it takes in.  Looks back at most 3 bytes.
LC_HD bool is_start(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t p) {
  if (!is_cont(t[p])) return true;
  uint64_t r = p;
  for (int back = 0; back < 3 && r > lo; back++) {
    r--;
    if (!is_cont(t[r])) {
      uint32_t l;
      (void)decode(t, hi, r, &l);
      return r + l <= p;
    }
  }
  return true;
}

LC_HD uint32_t utf8_len(uint32_t c) { return c < 0x80u ? 1u : c < 0x800u ? 2u : c < 0x10000u ? 3u : 4u; }

LC_HD uint32_t put(uint8_t* out, uint32_t c) {
  if (c < 0x80u) {
    out[0] = (uint8_t)c;
    return 1;
  }
  if (c < 0x800u) {
    out[0] = (uint8_t)(0xC0u | (c >> 6));
    out[1] = (uint8_t)(0x80u | (c & 63u));
    return 2;
  }
  if (c < 0x10000u) {
    out[0] = (uint8_t)(0xE0u | (c >> 12));
    out[1] = (uint8_t)(0x80u | ((c >> 6) & 63u));
    out[2] = (uint8_t)(0x80u | (c & 63u));
    return 3;
  }
  out[0] = (uint8_t)(0xF0u | (c >> 18));
  out[1] = (uint8_t)(0x80u | ((c >> 12) & 63u));
  out[2] = (uint8_t)(0x80u | ((c >> 6) & 63u));
  out[3] = (uint8_t)(0x80u | (c & 63u));
  return 4;
}

LC_HD bool in_ranges(const uint32_t* r, uint32_t n, uint32_t c) {
  uint32_t lo = 0, hi = n;  // the first range whose last >= c
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (r[2 * mid + 1] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && r[2 * lo] <= c;
}

// the table's mapping of one code point (U+03A3 and the second code point of U+0130 are the caller's)
LC_HD uint32_t map_cp(const Tables& T, uint32_t c) {
  if (c < 0x80u) return c >= 'A' && c <= 'Z' ? c + 32u : c;
  uint32_t lo = 0, hi = T.n_map;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (T.from[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < T.n_map && T.from[lo] == c ? T.to[lo] : c;
}

// the sigma at [p, p + 2) of the text [lo, hi) is final
LC_HD bool final_sigma(const Tables& T, const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t p) {
  bool cased_before = false;
  for (uint64_t q = p; q > lo;) {
    uint64_t r = q - 1;
    for (int back = 1; back < 4 && r > lo && is_cont(t[r]); back++) r--;
    uint32_t l;
    uint32_t c = decode(t, q, r, &l);
    if (c == kRaw || r + l != q) {  // (not a code point that ends at q: a raw byte, neither class)
      r = q - 1;
      c = kRaw;
    }
    if (c != kRaw && in_ranges(T.ignorable, T.n_ignorable, c)) {
      q = r;
      continue;
    }
    cased_before = c != kRaw && in_ranges(T.cased, T.n_cased, c);
    break;
  }
  if (!cased_before) return false;
  for (uint64_t q = p + 2; q < hi;) {
    uint32_t l;
    const uint32_t c = decode(t, hi, q, &l);
    if (c != kRaw && in_ranges(T.ignorable, T.n_ignorable, c)) {
      q += l;
      continue;
    }
    return !(c != kRaw && in_ranges(T.cased, T.n_cased, c));
  }
  return true;
}

// Lowercase of the code point (or raw byte) that starts at p of the text [lo, hi): the input
// length in *in_len, the output's bytes returned and, when out is non-null, written (at most 4;
// no input byte changes where the result equals *in_len raw bytes: *same says so).
LC_HD uint32_t lower_at(const Tables& T, const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t p, uint32_t* in_len,
                        bool* same, uint8_t* out) {
  const uint32_t c = decode(t, hi, p, in_len);
  if (c < 0x80u || c == kRaw) {
    const uint8_t b = c == kRaw ? t[p] : (uint8_t)map_cp(T, c);
    *same = b == t[p];
    if (out) out[0] = b;
    return 1;
  }
  if (c == 0x130u) {
    *same = false;
    if (out) {
      out[0] = 'i';
      out[1] = 0xCC;
      out[2] = 0x87;
    }
    return 3;
  }
  const uint32_t m = c == 0x3A3u ? (final_sigma(T, t, lo, hi, p) ? 0x3C2u : 0x3C3u) : map_cp(T, c);
  *same = m == c;
  if (m == c) {  // (the input's own bytes, whatever their form)
    if (out)
      for (uint32_t j = 0; j < *in_len; j++) out[j] = t[p + j];
    return *in_len;
  }
  if (out) return put(out, m);
  return utf8_len(m);
}

}  // namespace lowercase
