// Pair lookups of the merge passes and the long-piece tiers: the LDS image
// (hot table + Bloom filter), the two-stage Probe of kernels.hip's class passes, rank_pair of
// long.hip's wave tiers; and the one-thread-per-piece BPE with the added-token match, which the
// generic pass (kernels.hip) and k_bpe_long (long.hip) share.  Device-only; every function is __forceinline__ or defined inside its class.
#pragma once
#include "dev_common.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// BPE, short pieces: one thread per piece, the working tokens and pair ranks in LDS
// (thread-interleaved columns: entry j of thread t at [j*256 + t], conflict-free).

struct AddedMatch {  // first occurrence of added token k in bytes[0, n) honouring its flags
  __device__ static int64_t find(const Tables& t, uint32_t k, const uint8_t* s, uint32_t n) {
    const uint8_t* pat = t.at_bytes + t.at_off[k];
    const uint32_t m = t.at_off[k + 1] - t.at_off[k];
    if (m > n) return -1;
    for (uint32_t pos = 0; pos + m <= n; pos++) {
      uint32_t j = 0;
      while (j < m && s[pos + j] == pat[j]) j++;
      if (j < m) continue;
      // first occurrence found: the flags are checked only here (src/huggingface/mod.rs:637-675)
      const uint8_t f = t.at_flags[k];
      if (f & 1) {  // single_word: Rust is_alphanumeric of the neighbouring byte-mapped chars
        if (pos > 0 && t.bytemap_alnum[s[pos - 1]]) return -1;
        if (pos + m < n && t.bytemap_alnum[s[pos + m]]) return -1;
      }
      // byte-mapped chars are never White_Space: lstrip/rstrip pass only at the edges
      if ((f & 2) && pos > 0) return -1;
      if ((f & 4) && pos + m < n) return -1;
      return pos;
    }
    return -1;
  }
};

#define TOK(i) s_tok[(i) * NT + tid]
#define RK(i) s_rk[(i) * NT + tid]

// BPE over bytes[0, n) (n <= the slots per thread), appending ids to out; returns the id count.
// s_tok / s_rk hold NT threads' slots interleaved.
template <uint32_t NT>
__device__ __forceinline__ uint32_t bpe_short(const Tables& t, const uint8_t* bytes, uint32_t n,
                                              const int32_t* s_b2id, uint32_t* s_tok, uint32_t* s_rk,
                                              uint32_t tid, uint32_t* out, uint32_t* err) {
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; i++) {
    const int32_t id = s_b2id[bytes[i]];
    if (id >= 0) TOK(m++) = (uint32_t)id;
  }
  if (m >= 2) {
    for (uint32_t i = 0; i + 1 < m; i++) RK(i) = rank_of(t, TOK(i), TOK(i + 1), err);
    while (m >= 2) {
      uint32_t best = kNoRank, bi = 0;
      for (uint32_t i = 0; i + 1 < m; i++) {
        const uint32_t r = RK(i);
        if (r < best) { best = r; bi = i; }
      }
      if (best == kNoRank) break;
      TOK(bi) = new_id_of(t, best);
      for (uint32_t i = bi + 1; i + 1 < m; i++) TOK(i) = TOK(i + 1);
      for (uint32_t i = bi + 1; i + 2 < m; i++) RK(i) = RK(i + 1);
      m--;
      if (bi > 0) RK(bi - 1) = rank_of(t, TOK(bi - 1), TOK(bi), err);
      if (bi + 1 < m) RK(bi) = rank_of(t, TOK(bi), TOK(bi + 1), err);
    }
  }
  for (uint32_t i = 0; i < m; i++) out[i] = TOK(i);
  return m;
}

// ------------------------------------------------------------------------------------------
// pair lookups through the LDS image

__device__ __forceinline__ uint32_t resolve_rank(const Tables& t, uint64_t key, uint32_t h, uint64_t e, uint32_t* err) {
  for (;;) {
    if ((e & kKeyMask) == key) {
      const uint32_t r = (uint32_t)(e >> 42);
      if (value_panics(t, r)) { atomicOr(err, kErrPanic); return kNoRank; }
      return r;
    }
    if (e == kEmpty) return kNoRank;
    h = (h + 1) & t.merge_mask;
    e = t.merge_tab[h];
  }
}

__device__ __forceinline__ uint64_t pair_key(uint32_t a, uint32_t b) { return ((uint64_t)a << kIdBits) | b; }

// The LDS image of the merge passes: hot table + Bloom filter (pair_tables_hd.h).
struct PairLds {
  const lds_u64* hot;  // bucket c = hot[2c], hot[2c + 1]
  const lds_u32* bloom;
};

// Rank lookup, LDS stage: the pair's value from the hot table, else kNoRank; `global` is set
// when the hot table missed and the Bloom filter cannot rule the pair out.  HOT = false: the
// Bloom filter only (workgroups that keep 32 KiB of LDS instead of 96).
template <bool HOT>
__device__ __forceinline__ uint32_t rank_lds(const PairLds& P, uint32_t a, uint32_t b, uint32_t h1, uint32_t h2,
                                             bool& global) {
  const uint32_t b1 = (h1 >> 12) & (kBloomBits - 1), b2 = (h2 >> 12) & (kBloomBits - 1);
  const uint32_t f = (P.bloom[b1 >> 5] >> (b1 & 31)) & (P.bloom[b2 >> 5] >> (b2 & 31)) & 1u;
  if constexpr (!HOT) {
    global = f != 0;
    return kNoRank;
  }
  const uint32_t c1 = 2 * (h1 & (kHotBuckets - 1)), c2 = 2 * (h2 & (kHotBuckets - 1));
  const uint64_t x0 = P.hot[c1], x1 = P.hot[c1 + 1], y0 = P.hot[c2], y1 = P.hot[c2 + 1];
  // entry = value << 42 | a << 21 | b: compare the 42-bit key as (lo 32, hi 10)
  const uint32_t klo = (a << kIdBits) | b, khi = a >> (32 - kIdBits);
  uint32_t v = kNoRank;
  bool hit = false;
  auto chk = [&](uint64_t e) {
    const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
    const bool m = lo == klo && (hi & 0x3FFu) == khi;
    v = m ? (hi >> 10) : v;
    hit |= m;
  };
  chk(x0);
  chk(x1);
  chk(y0);
  chk(y1);
  global = !hit && f;
  return v;
}

// One pair lookup of a merge pass, split in two so that the global-table load (issued by
// start, only when the LDS stage cannot decide) overlaps the caller's other work before finish.
// NARROW = false: the 42-bit-key tables (mhash / mhash2); true: the 32-bit-key tables (key16,
// pair_tables_hd.h), whose hashes and bucket compares take about half the VALU.
template <bool NARROW, bool HOT> struct Probe;

template <bool HOT>
struct Probe<false, HOT> {
  uint32_t a, b, h, r;
  uint64_t e;
  bool g;
  __device__ __forceinline__ void start(const Tables& t, const PairLds& P, uint32_t a_, uint32_t b_, bool live) {
    a = a_;
    b = b_;
    h = mhash(a, b);
    r = rank_lds<HOT>(P, a, b, h, mhash2(h), g);
    g = g && live;
    e = 0;
    if (g) e = t.merge_tab[h & t.merge_mask];
  }
  __device__ __forceinline__ uint32_t finish(const Tables& t, uint32_t* err) {
    if (g) r = resolve_rank(t, pair_key(a, b), h & t.merge_mask, e, err);
    return r;
  }
};

template <bool HOT>
struct Probe<true, HOT> {
  uint32_t k, h, r;
  uint64_t e;
  bool g;
  __device__ __forceinline__ void start(const Tables& t, const PairLds& P, uint32_t a, uint32_t b, bool live) {
    a &= 0xFFFFu;  // (ids < 2^16; known to the compiler, the hashes use 24-bit multiplies)
    b &= 0xFFFFu;
    k = key16(a, b);
    h = hash16_h(a, b);
    const uint32_t h2 = hash16_g(a, b);
    const uint32_t b1 = h & (kBloomBits - 1), b2 = h2 >> 14;
    const uint32_t f = (P.bloom[b1 >> 5] >> (b1 & 31)) & (P.bloom[b2 >> 5] >> (b2 & 31)) & 1u;
    const uint32_t c1 = 2 * (h >> 20), c2 = 2 * (h2 >> 20);
    const uint64_t x0 = P.hot[c1], x1 = P.hot[c1 + 1], y0 = P.hot[c2], y1 = P.hot[c2 + 1];
    uint32_t v = kNoRank;
    bool hit = false;
    auto chk = [&](uint64_t x) {
      const bool m = (uint32_t)x == k;
      v = m ? (uint32_t)(x >> 32) : v;
      hit |= m;
    };
    chk(x0);
    chk(x1);
    chk(y0);
    chk(y1);
    r = v;
    g = !hit && f && live;
    e = 0;
    if (g) e = t.merge16[h & t.merge16_mask];
  }
  __device__ __forceinline__ uint32_t finish(const Tables& t, uint32_t* err) {
    if (g) {
      uint32_t s = h & t.merge16_mask;
      for (;;) {
        if ((uint32_t)e == k) {
          r = (uint32_t)(e >> 32);
          if (value_panics(t, r)) { atomicOr(err, kErrPanic); r = kNoRank; }
          break;
        }
        if (e == kEmpty) { r = kNoRank; break; }
        s = (s + 1) & t.merge16_mask;
        e = t.merge16[s];
      }
    }
    return r;
  }
};

// value of pair (a, b) (never a byte pair): LDS hot table (HOT) and Bloom filter, the global
// table when neither settles it
template <bool HOT>
__device__ __forceinline__ uint32_t rank_pair(const Tables& t, const PairLds& P, uint32_t a, uint32_t b,
                                              uint32_t* err) {
  const uint32_t h1 = mhash(a, b);
  bool g;
  const uint32_t v = rank_lds<HOT>(P, a, b, h1, mhash2(h1), g);
  if (!g) return v;
  const uint32_t h = h1 & t.merge_mask;
  return resolve_rank(t, pair_key(a, b), h, t.merge_tab[h], err);
}

}  // namespace ctok_dev
