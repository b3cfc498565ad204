// What the Unigram kernels (unigram.hip) share with the CPU check (tools/unigram_check.cpp): the
// Metaspace rules, the walk that finds every vocab string starting at a char, and the rule by which
// a Viterbi step keeps one candidate.  Plain integer and f64 code, no HIP include, no intrinsics.
//
// A char is a lead byte with the continuation bytes behind it: a position is a char start when its
// byte is no continuation byte, and a walk moves from one char start to the next.  For valid UTF-8
// that is the code point; for any other bytes it is still consistent between the kernels (which
// count the same char starts), and no function reads a byte at or past the length it is given.
#pragma once
#include <cstdint>

#include "wp_table_hd.h"
#include "ws_split_hd.h"

#if defined(__HIPCC__)
#define UNI_HD __host__ __device__ __forceinline__
#else
#define UNI_HD inline
#endif

namespace uni {

constexpr uint32_t kNone = wptab::kNone;
constexpr uint32_t kSpan = 64;  // input bytes a thread of the Metaspace kernels owns

UNI_HD bool is_lead(uint8_t b) { return (b & 0xC0u) != 0x80u; }

// the next char start behind byte q (q < n), or n
UNI_HD uint64_t next_lead(const uint8_t* text, uint64_t n, uint64_t q) {
  q++;
  while (q < n && !is_lead(text[q])) q++;
  return q;
}

// ---- Metaspace (src/pretokenizers.rs:188-200 with '▁', add_prefix_space) --------------------------
// The text of document [lo, hi) becomes: E2 96 81, then its chars with U+0020 rewritten to E2 96 81,
// cut at (and without) the other 24 White_Space code points.

// the char at lead byte p of a document that ends at hi is one of the 24 that split
UNI_HD bool splits_at(const uint8_t* text, uint64_t hi, uint64_t p) { return text[p] != 0x20u && wsplit::ws_at(text, hi, p); }

// the char before lead byte p (lo < p) of the document that starts at lo splits
UNI_HD bool prev_splits(const uint8_t* text, uint64_t lo, uint64_t p) {
  uint64_t q = p - 1;
  int back = 1;
  while (back < 4 && q > lo && !is_lead(text[q])) {
    q--;
    back++;
  }
  return is_lead(text[q]) && splits_at(text, p, q);
}

struct Meta {  // what the char at lead byte p gives
  uint32_t in_len;   // its bytes in the input
  uint32_t out_len;  // its bytes in the output: 0 (it splits), 3 (a space) or in_len
  bool starts;       // a sentence starts with it
};

UNI_HD Meta meta_at(const uint8_t* text, uint64_t lo, uint64_t hi, uint64_t p) {
  Meta m;
  m.in_len = (uint32_t)(next_lead(text, hi, p) - p);
  if (splits_at(text, hi, p)) {
    m.out_len = 0;
    m.starts = false;
    return m;
  }
  m.out_len = text[p] == 0x20u ? 3u : m.in_len;
  m.starts = p > lo && prev_splits(text, lo, p);  // (the document's first char follows the prefix)
  return m;
}

// the first d in [0, n_docs] with doc_off[d] >= p (doc_off[n_docs] counts as past everything)
UNI_HD uint64_t first_doc_at(const uint64_t* doc_off, uint64_t n_docs, uint64_t p) {
  uint64_t lo = 0, hi = n_docs;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (doc_off[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The output of the positions [b0, b1) (b1 <= n_bytes + 1): bytes and sentence starts.  With out
// non-null the bytes go to out[0 ..] and the sentences' offsets (base + the byte) to sent[0 ..].
// (the span of a thread of k_meta_measure / k_meta_write; doc_off has n_docs + 1 entries)
UNI_HD void meta_range(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs, uint64_t b0,
                       uint64_t b1, uint8_t* out, uint64_t base, uint64_t* sent, uint64_t* n_out, uint64_t* n_sent) {
  uint64_t d = first_doc_at(doc_off, n_docs, b0), o = 0, k = 0;
  for (uint64_t p = b0; p < b1; p++) {
    while (d < n_docs && doc_off[d] == p) {  // the documents that start here: the prefix
      if (out) {
        out[o] = 0xE2u;
        out[o + 1] = 0x96u;
        out[o + 2] = 0x81u;
        sent[k] = base + o;
      }
      o += 3;
      k++;
      d++;
    }
    if (p >= n_bytes || d == 0) continue;
    const uint64_t lo = doc_off[d - 1];
    uint64_t hi = d < n_docs ? doc_off[d] : n_bytes;
    if (hi > n_bytes) hi = n_bytes;
    if (lo > p || hi <= p) continue;  // (offsets out of order: nothing is read outside [lo, hi))
    if (!uni::is_lead(text[p]) && p != lo) continue;
    const uni::Meta m = uni::meta_at(text, lo, hi, p);
    if (!m.out_len) continue;
    if (out) {
      if (m.starts) sent[k] = base + o;
      if (text[p] == 0x20u) {
        out[o] = 0xE2u;
        out[o + 1] = 0x96u;
        out[o + 2] = 0x81u;
      } else {
        for (uint32_t j = 0; j < m.out_len; j++) out[o + j] = text[p + j];
      }
    }
    if (m.starts) k++;
    o += m.out_len;
  }
  *n_out = o;
  *n_sent = k;
}

// ---- every vocab string that starts at a char -----------------------------------------------------
// hit(j, sym) for every pattern of form 0 that starts at char start p (p < n) and is j + 1 chars
// long, j < max_chars, inside p's sentence: the sentence ends at n or at the first set bit of
// starts behind p.  Hashes char by char (FNV-1a) and probes once per boundary; looks at no more
// than v.max_len bytes.  Returns the chars walked.
template <typename Hit>
UNI_HD uint32_t matches(const wptab::View& v, const uint8_t* text, uint64_t n, const uint32_t* starts, uint64_t p,
                        uint32_t max_chars, Hit hit) {
  uint32_t h = wptab::kSeed, j = 0;
  uint64_t q = p;
  while (q < n && j < max_chars) {
    const uint64_t e = next_lead(text, n, q);
    if (e - p > v.max_len) break;
    for (; q < e; q++) h = wptab::step(h, text[q]);
    const uint32_t s = wptab::find(v, text + p, (uint32_t)(e - p), h, 0);
    if (s != kNone) hit(j, s);
    j++;
    if (e < n && wptab::bit_at(starts, e)) break;
  }
  return j;
}

// the ends of the substrings of 1 .. max_chars chars that start at char start p inside its sentence:
// each(end byte) in ascending order
template <typename Each>
UNI_HD void substrings(const uint8_t* text, uint64_t n, const uint32_t* starts, uint64_t p, uint64_t max_chars, Each each) {
  uint64_t q = p;
  for (uint64_t j = 0; q < n && j < max_chars; j++) {
    q = next_lead(text, n, q);
    each(q);
    if (q < n && wptab::bit_at(starts, q)) break;
  }
}

// ---- one Viterbi step -----------------------------------------------------------------------------
// The reference runs the starts of one end in ascending order and replaces best[end] when
// best[start] + score > best[end].score, from (-inf, -1): the maximum of the sums above -inf wins,
// a NaN never does, and among equal sums the smallest start, which is the longest token.
// (sum, j) replaces (best_sum, best_j); j + 1 is the token's length in chars, best_sum = -inf: none yet.
// The callers move every field of a candidate under this one predicate, as scalars.
UNI_HD bool takes(double sum, uint32_t j, double best_sum, uint32_t best_j) {
  if (!(sum > -__builtin_inf())) return false;
  return sum > best_sum || (sum == best_sum && j > best_j);
}

}  // namespace uni
