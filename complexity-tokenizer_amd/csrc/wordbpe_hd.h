// The tables and the scalar loops of the id-keyed word BPE (wordbpe.hip), shared with the host
// (wordbpe_compile.cpp builds the tables) and the CPU check (tools/wordbpe_check.cpp): plain integer
// code, no HIP include, no intrinsics.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   BpeTokenizer::new / encode_with_dropout(0)   src/bpe.rs:52-153
//   the added-token loop of encode               src/huggingface/mod.rs:566-675
// A symbol is a vocab id.  The pair table is strmerge_hd.h's, keyed (id_a, id_b): `rank` holds the
// merge's unfiltered rank, `sym` the new id filtered[rank].new_id.  A pair whose rank is at or past the
// filtered list's length carries kPanicBit in `rank`: the reference indexes out of bounds as soon as
// it sees such a pair adjacent, so every rank lookup tests the bit (is_panic) before it is used.
// Ranks stay below kMaxMerges = 2^24, so a marked rank is never kNoRank.
#pragma once
#include <cstdint>

#include "strmerge_hd.h"

namespace wordbpe {

using strmerge::kDead;
using strmerge::kNoRank;
using strmerge::PairView;

constexpr uint32_t kPanicBit = 0x80000000u;
constexpr uint32_t kMaxMerges = 1u << 24;
constexpr uint32_t kMaxAdded = 1024;        // added tokens of one tokenizer (the loop's seen-set: kMaxAdded bits)
constexpr uint32_t kMaxAddedBytes = 1024;   // bytes of one added token
// bytes of the added tokens that share a first byte: what one candidate position can cost in compares
constexpr uint32_t kMaxGroupBytes = 1u << 15;
constexpr uint32_t kNoId = 0xFFFFFFFFu;     // no vocab id; an empty code-point slot; a segment that is an added token
constexpr uint32_t kCpProbe = 32;
constexpr uint32_t kNoPanic = 0xFFFFFFFFu;

SM_HD bool is_panic(uint32_t rank) { return rank != kNoRank && (rank & kPanicBit); }

// ---- code point -> id of the one-char vocab string ---------------------------------------------------

struct CpSlot {
  uint32_t cp;  // kNoId: empty
  uint32_t id;
};

struct CpView {
  const CpSlot* slots;
  uint32_t mask;
};

SM_HD uint32_t cp_slot(uint32_t cp, uint32_t mask) {
  uint32_t h = cp * 0x9E3779B1u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return h & mask;
}

// the id of the char, or kNoId (no vocab id is kNoId: wordbpe_compile.cpp refuses it)
SM_HD uint32_t cp_find(const CpView& v, uint32_t cp) {
  uint32_t s = cp_slot(cp, v.mask);
  for (uint32_t i = 0; i < kCpProbe; i++) {
    const CpSlot e = v.slots[s];
    if (e.cp == kNoId) break;
    if (e.cp == cp) return e.id;
    s = (s + 1) & v.mask;
  }
  return kNoId;
}

// ---- UTF-8 -------------------------------------------------------------------------------------------

SM_HD bool is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// the bytes of the well-formed char at t[p] that ends at or before `end`, and its code point; 0: none
SM_HD uint32_t dec_char(const uint8_t* t, uint64_t p, uint64_t end, uint32_t* cp) {
  if (p >= end) return 0;
  const uint32_t b0 = t[p];
  if (b0 < 0x80u) {
    *cp = b0;
    return 1;
  }
  uint32_t len, c;
  if (b0 >= 0xC2u && b0 < 0xE0u) len = 2, c = b0 & 0x1Fu;
  else if (b0 >= 0xE0u && b0 < 0xF0u) len = 3, c = b0 & 0x0Fu;
  else if (b0 >= 0xF0u && b0 < 0xF5u) len = 4, c = b0 & 0x07u;
  else return 0;
  if (p + len > end) return 0;
  for (uint32_t j = 1; j < len; j++) {
    const uint32_t b = t[p + j];
    if ((b & 0xC0u) != 0x80u) return 0;
    c = (c << 6) | (b & 0x3Fu);
  }
  if (len == 3 && (c < 0x800u || (c >= 0xD800u && c < 0xE000u))) return 0;
  if (len == 4 && (c < 0x10000u || c > 0x10FFFFu)) return 0;
  *cp = c;
  return len;
}

// the code point of the char that ends at t[p) and starts at or after lo; kNoId: there is none, or
// the bytes before p are not a well-formed char (such a unit is no letter, number or white space)
SM_HD uint32_t char_before(const uint8_t* t, uint64_t lo, uint64_t p) {
  if (p <= lo) return kNoId;
  uint64_t q = p - 1;
  while (q > lo && p - q < 4 && is_cont(t[q])) q--;
  uint32_t cp = 0;
  return dec_char(t, q, p, &cp) == p - q ? cp : kNoId;
}

SM_HD uint32_t char_at(const uint8_t* t, uint64_t p, uint64_t end) {
  uint32_t cp = 0;
  return dec_char(t, p, end, &cp) ? cp : kNoId;
}

SM_HD bool is_ws(uint32_t c) {  // char::is_whitespace: the 25 White_Space code points
  return (c >= 0x09u && c <= 0x0Du) || c == 0x20u || c == 0x85u || c == 0xA0u || c == 0x1680u || (c >= 0x2000u && c <= 0x200Au) ||
         c == 0x2028u || c == 0x2029u || c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}

// ---- the added tokens --------------------------------------------------------------------------------

enum : uint32_t { kSingleWord = 1, kLstrip = 2, kRstrip = 4 };

// The tokens ordered by first byte: group[b] .. group[b + 1] are those that start with byte b; token
// i is bytes[off[i] .. off[i + 1]).  alnum_lo / alnum_hi: the n_alnum ascending runs of csrc/gen/alnum_data.h.
struct AddedView {
  const uint8_t* bytes;
  const uint32_t* off;    // [n + 1]
  const uint32_t* id;     // [n]
  const uint32_t* flags;  // [n]
  const uint32_t* group;  // [257]
  const uint32_t* alnum_lo;
  const uint32_t* alnum_hi;
  uint32_t n_alnum;
  uint32_t n;
};

SM_HD bool is_alnum(const AddedView& a, uint32_t c) {
  if (c == kNoId) return false;
  uint32_t lo = 0, hi = a.n_alnum;  // the first run with alnum_hi >= c
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (a.alnum_hi[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_alnum && a.alnum_lo[lo] <= c;
}

// does token i stand at t[p ..) and end at or before `end`?
SM_HD bool added_at(const AddedView& a, uint32_t i, const uint8_t* t, uint64_t p, uint64_t end) {
  const uint32_t o = a.off[i], len = a.off[i + 1] - o;
  if (p + len > end) return false;
  for (uint32_t j = 0; j < len; j++)
    if (t[p + j] != a.bytes[o + j]) return false;
  return true;
}

// find_added_token's checks (mod.rs:640-672) for token i found at p inside the remaining text
// t[r .. end): at p == r nothing stands before the token, so only the checks on what follows apply
SM_HD bool added_ok(const AddedView& a, uint32_t i, const uint8_t* t, uint64_t r, uint64_t p, uint64_t end) {
  const uint32_t f = a.flags[i];
  if (!f) return true;
  const uint64_t q = p + (a.off[i + 1] - a.off[i]);
  if (f & kSingleWord) {
    if (p > r && is_alnum(a, char_before(t, r, p))) return false;
    if (q < end && is_alnum(a, char_at(t, q, end))) return false;
  }
  if ((f & kLstrip) && p > r) {
    const uint32_t c = char_before(t, r, p);
    if (c == kNoId || !is_ws(c)) return false;
  }
  if ((f & kRstrip) && q < end) {
    const uint32_t c = char_at(t, q, end);
    if (c == kNoId || !is_ws(c)) return false;
  }
  return true;
}

// One segment of a word: an added token (a == kNoId, b its id) or the bytes [a, b) for the word BPE.
struct Seg {
  uint32_t a, b;
};

// The literal loop of encode (mod.rs:566-610) over the word t[wb .. we): the segments in order,
// written to out when it is not null; returns their number.  Every byte position is visited at most
// once by the search for the next token and once as a start; a visit compares the tokens that share
// the position's first byte.  `seen` marks the tokens whose first occurrence in the remaining text
// is already behind the cursor: find_added_token looks at the first occurrence only, so a later one
// is hidden whether or not the first passed its checks.
// mbits (may be null): a bit per byte of t, set where some added token's bytes stand; the search skips
// the clear stretches a bitmap word at a time.
SM_HD uint64_t next_candidate(const uint32_t* mbits, uint64_t p, uint64_t we) {
  if (!mbits) return p;
  while (p < we) {
    const uint32_t v = mbits[p >> 5] >> (p & 31);
    if (v & 1u) return p;
    if (!v) p = (p | 31u) + 1;
    else p++;
  }
  return we;
}

SM_HD uint32_t split_word(const AddedView& a, const uint8_t* t, uint64_t wb, uint64_t we, const uint32_t* mbits, Seg* out) {
  uint32_t seen[kMaxAdded / 32];
  const uint32_t n_seen = (a.n + 31) / 32;
  uint32_t n = 0;
  uint64_t r = wb;
  if (r >= we) {  // the empty word: one empty segment
    if (out) out[0] = Seg{(uint32_t)wb, (uint32_t)we};
    return 1;
  }
  while (r < we) {
    for (uint32_t k = 0; k < n_seen; k++) seen[k] = 0;
    // the longest token at the cursor that passes its checks
    uint32_t best_len = 0, best_id = 0;
    for (uint32_t i = a.group[t[r]]; i < a.group[t[r] + 1u]; i++) {
      if (!added_at(a, i, t, r, we)) continue;
      seen[i >> 5] |= 1u << (i & 31);
      const uint32_t len = a.off[i + 1] - a.off[i];
      if (len > best_len && added_ok(a, i, t, r, r, we)) best_len = len, best_id = a.id[i];
    }
    if (best_len) {
      if (out) out[n] = Seg{kNoId, best_id};
      n++;
      r += best_len;
      continue;
    }
    // the nearest first occurrence behind the cursor that passes its checks
    uint64_t nxt = we;
    for (uint64_t p = next_candidate(mbits, r + 1, we); p < we && nxt == we; p = next_candidate(mbits, p + 1, we)) {
      for (uint32_t i = a.group[t[p]]; i < a.group[t[p] + 1u]; i++) {
        if ((seen[i >> 5] >> (i & 31)) & 1u) continue;
        if (!added_at(a, i, t, p, we)) continue;
        seen[i >> 5] |= 1u << (i & 31);
        if (added_ok(a, i, t, r, p, we)) {
          nxt = p;
          break;
        }
      }
    }
    if (out) out[n] = Seg{(uint32_t)r, (uint32_t)nxt};
    n++;
    r = nxt;
  }
  return n;
}

// ---- the merge loop ----------------------------------------------------------------------------------

// strmerge::merge_word over ids with the panic mark: n tokens at tok[i * stride], n cached ranks at
// rank[i * stride].  Returns the tokens left and leaves *panic_rank as it is (the caller sets it to
// kNoPanic); when a marked pair is seen, stores its rank in *panic_rank and returns 0.
// The reference scans the pairs left to right at every step and fails at the first marked one: at
// the first step that is the leftmost marked pair, later only the two pairs a merge created can be
// new, the left one first.
SM_HD uint32_t merge_ids(const PairView& v, uint32_t* tok, uint32_t* rank, uint32_t stride, uint32_t n, uint32_t* panic_rank) {
  for (uint32_t i = 0; i + 1 < n; i++) {
    const uint32_t r = strmerge::pair_find(v, tok[i * stride], tok[(i + 1) * stride]).rank;
    if (is_panic(r)) {
      *panic_rank = r & ~kPanicBit;
      return 0;
    }
    rank[i * stride] = r;
  }
  while (n > 1) {
    uint32_t best = kNoRank, at = 0;
    for (uint32_t i = 0; i + 1 < n; i++) {
      const uint32_t r = rank[i * stride];
      if (r < best) best = r, at = i;
    }
    if (best == kNoRank) break;
    tok[at * stride] = strmerge::pair_find(v, tok[at * stride], tok[(at + 1) * stride]).sym;
    for (uint32_t i = at + 1; i + 1 < n; i++) {
      tok[i * stride] = tok[(i + 1) * stride];
      rank[i * stride] = rank[(i + 1) * stride];
    }
    n--;
    if (at > 0) {
      const uint32_t r = strmerge::pair_find(v, tok[(at - 1) * stride], tok[at * stride]).rank;
      if (is_panic(r)) {
        *panic_rank = r & ~kPanicBit;
        return 0;
      }
      rank[(at - 1) * stride] = r;
    }
    if (at + 1 < n) {
      const uint32_t r = strmerge::pair_find(v, tok[at * stride], tok[(at + 1) * stride]).rank;
      if (is_panic(r)) {
        *panic_rank = r & ~kPanicBit;
        return 0;
      }
      rank[at * stride] = r;
    }
  }
  return n;
}

}  // namespace wordbpe
