// The rules of PipelineTokenizer's Encoding path (the reference's src/huggingface/mod.rs:340-480), shared
// by the kernels (pipeline_enc.hip) and the CPU check (tools/pipeline_enc_check.cpp): plain integer
// code, no HIP include.  All positions are byte indices into a sequence's original text.
//
//   pre_tokenize_with_offsets (mod.rs:448-480)   needle_skip, boundary_panic, match_at, find_scalar, word_span
//   the token offsets (mod.rs:395-443)           tok_span, table_len
//   encode_to_encoding_impl (mod.rs:358-392)     row_cell, is_special
//
// Invariant: word_start <= word_end for every word.  A hit gives (pos, pos + m); a miss gives
// (s, min(s + wl, L)) with s <= L, because s is 0 or an earlier word's end and every end is at most L.
// tok_span's closed form rests on it: clipping a running position to word_end at every step equals
// clipping the unclipped sum once, since the sum never decreases and word_start <= word_end.
//
// No function reads a text byte at or past the length it is given, or a table entry past its count.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PE_HD __host__ __device__ inline
#else
#define PE_HD inline
#endif

namespace pipeline_enc {

// The bytes of a word's leading 'Ġ' (C4 A0) and '▁' (E2 96 81) chars that the needle leaves out
// (str::trim_start_matches); 0 when nothing would be left: the needle is then the whole word.
PE_HD uint64_t needle_skip(const uint8_t* w, uint64_t wl) {
  uint64_t t = 0;
  for (;;) {
    if (t + 2 <= wl && w[t] == 0xC4 && w[t + 1] == 0xA0) t += 2;
    else if (t + 3 <= wl && w[t] == 0xE2 && w[t + 1] == 0x96 && w[t + 2] == 0x81) t += 3;
    else break;
  }
  return t == wl ? 0 : t;
}

// `&original[s..]` panics when s is inside a UTF-8 char (s == L is a boundary)
PE_HD bool boundary_panic(const uint8_t* text, uint64_t L, uint64_t s) { return s < L && (text[s] & 0xC0) == 0x80; }

// does the needle (m > 0 bytes) stand at pos?  A candidate that would end past L is no match.
// *compared grows by the bytes after the first that were equal: what a partial match costs.
PE_HD bool match_at(const uint8_t* text, uint64_t L, uint64_t pos, const uint8_t* needle, uint64_t m, uint64_t* compared) {
  if (pos > L || m > L - pos) return false;
  if (text[pos] != needle[0]) return false;
  uint64_t j = 1;
  while (j < m && text[pos + j] == needle[j]) j++;
  *compared += j - 1;
  return j == m;
}
PE_HD bool match_at(const uint8_t* text, uint64_t L, uint64_t pos, const uint8_t* needle, uint64_t m) {
  uint64_t compared = 0;
  return match_at(text, L, pos, needle, m, &compared);
}

// str::find from s (s <= L): the leftmost match, or L + 1 for none; an empty needle is found at s
PE_HD uint64_t find_scalar(const uint8_t* text, uint64_t L, uint64_t s, const uint8_t* needle, uint64_t m) {
  if (!m) return s;
  for (uint64_t pos = s; pos <= L && m <= L - pos; pos++)
    if (match_at(text, L, pos, needle, m)) return pos;
  return L + 1;
}

// A word's span and the work of its search.  pos: where the needle (m bytes) was found, or > L; s: where
// the search began; wl: the untrimmed word's bytes.
PE_HD void word_span(uint64_t pos, uint64_t s, uint64_t m, uint64_t wl, uint64_t L, uint64_t* start, uint64_t* end,
                     uint64_t* work) {
  if (pos <= L) {
    *start = pos;
    *end = pos + m;
    *work = pos - s + m;
  } else {
    *start = s;
    *end = wl < L - s ? s + wl : L;
    *work = L - s;
  }
}

// the bytes of an id's vocab string: ids sorted, no duplicates; an id without a string has none
PE_HD uint32_t table_len(const uint32_t* ids, const uint32_t* lens, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == id ? lens[lo] : 0;
}

// is the id in the sorted list?
PE_HD bool is_special(const uint32_t* ids, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == id;
}

// the last j in [0, n] with pos[j] <= k, for pos not decreasing with pos[0] <= k (among equal entries the
// last: a word or a sequence without ids is never an id's own)
PE_HD uint64_t find_owner(const uint64_t* pos, uint64_t n, uint64_t k) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (pos[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
PE_HD uint32_t find_owner32(const uint32_t* pos, uint32_t n, uint32_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (pos[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Token k's offsets inside its word (ws, we): sk, sk1 and sf are the exclusive scan of the token byte
// lengths at k, at k + 1 and at the word's first id.
PE_HD void tok_span(uint64_t ws, uint64_t we, uint64_t sk, uint64_t sk1, uint64_t sf, uint64_t* p, uint64_t* e) {
  const uint64_t a = ws + (sk - sf), b = ws + (sk1 - sf);
  *p = a < we ? a : we;
  *e = b < we ? b : we;
}

// Cell i of a processed row: n ids before the post-processor, of which the first na are A's.
PE_HD void row_cell(uint64_t i, uint64_t n, uint64_t na, bool special_id, uint32_t* type_id, uint32_t* special) {
  *type_id = i >= na && i < n ? 1u : 0u;
  *special = i >= n || special_id ? 1u : 0u;
}

}  // namespace pipeline_enc
