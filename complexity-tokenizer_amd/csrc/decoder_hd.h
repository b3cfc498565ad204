// The rules of the Decoder (the reference's src/decoders.rs:30-243), shared by the kernels
// (decoder.hip) and the CPU check (tools/decoder_check.cpp): plain integer code, no HIP include.
//
// A batch is its bytes, the tokens' offsets and the documents' token ranges: token j is
// bytes[tok_off[j] .. tok_off[j + 1]), document d owns tokens doc_tok[d] .. doc_tok[d + 1].  Tokens lie
// back to back, so a document's concatenation (tokens.join("")) is bytes[doc_off[d] .. doc_off[d + 1])
// with doc_off[d] = tok_off[doc_tok[d]], and costs nothing.
//
// A decoder is a program of ops (expand() of decoder_internal.h makes them from the steps).  Every op
// has one shape: a unit -- a byte for the text rules, a token for WordPiece, BPE and CTC -- emits a
// number of bytes that unit_emit() gives, with out == nullptr to count and with the unit's place in the
// output to write; the caller counts, scans and writes.  What a unit cannot see from its neighbourhood
// is made before by the preparing functions: a kept range per document (strip_range, trim_range), the
// first token of a document that contributes a byte (wp_first), the marks of the literal matches
// (rep_cand, rep_chain) and of the spaces the clean-up deletes (cleanup_run).
//
// No function reads outside its document, and every loop is bounded by its document's, token's or
// pattern's length.  The bytes are taken as they are: what is not well-formed UTF-8 is a one-byte
// unit that no rule's string matches except byte for byte.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DEC_HD __host__ __device__ inline
#else
#define DEC_HD inline
#endif

namespace decoder {

enum Op : uint32_t {
  OP_FUSE,       // every byte as it is
  OP_BL_MAP,     // ByteLevel, first pass: a char of the byte map gives its byte, other ASCII itself, the rest nothing
  OP_LOSSY,      // ByteLevel, second pass: String::from_utf8_lossy
  OP_METASPACE,  // a: the replacement's UTF-8; flags & 1: add_prefix_space
  OP_RANGE,      // the bytes of [lo[d], hi[d]) (Strip, and the trim_end of BPE)
  OP_MARK,       // Replace with a pattern: a match start gives b, the rest of a match nothing (mark)
  OP_INSERT,     // Replace with the empty pattern: b before every code point, and after the text (the tail)
  OP_DEAD,       // WordPiece clean-up: the bytes that are not marked
  OP_WORDPIECE,  // a: the prefix
  OP_BPE,        // a: the suffix
  OP_CTC         // a: the pad token; b: the delimiter when flags & 1
};

constexpr uint8_t kMatchStart = 1, kInMatch = 2;  // OP_MARK's marks
constexpr uint8_t kDead = 1;                      // OP_DEAD's mark
constexpr uint64_t kNone = ~0ull;

struct Step {
  uint32_t op, flags;
  const uint8_t* a;
  uint64_t a_len;
  const uint8_t* b;
  uint64_t b_len;
};

struct In {
  const uint8_t* bytes;
  uint64_t n;
  const uint64_t* tok_off;  // n_tok + 1
  uint64_t n_tok;
  const uint64_t* doc_tok;  // n_docs + 1
  uint64_t n_docs;
  const uint64_t* doc_off;  // n_docs + 1: tok_off[doc_tok[d]]
  const uint64_t* lo;       // OP_RANGE: n_docs each
  const uint64_t* hi;
  const uint8_t* mark;      // OP_MARK, OP_DEAD: n
  const uint64_t* first;    // OP_WORDPIECE: n_docs
};

DEC_HD bool is_tok_op(uint32_t op) { return op >= OP_WORDPIECE; }
// the bytes every document gets after its units' (OP_INSERT)
DEC_HD uint64_t tail_len(const Step& st) { return st.op == OP_INSERT ? st.b_len : 0; }

DEC_HD bool eq(const uint8_t* x, const uint8_t* y, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (x[i] != y[i]) return false;
  return true;
}

DEC_HD void put(uint8_t* out, const uint8_t* src, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) out[i] = src[i];
}

// the document of unit u < off[n_docs]: the d with off[d] <= u < off[d + 1] (off[0] = 0, non-decreasing)
DEC_HD uint64_t doc_of(const uint64_t* off, uint64_t n_docs, uint64_t u) {
  uint64_t lo = 0, hi = n_docs - 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] <= u) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the first d in [0, n_docs] with off[d] >= x, n_docs + 1 when there is none
DEC_HD uint64_t first_doc_from(const uint64_t* off, uint64_t n_docs, uint64_t x) {
  uint64_t lo = 0, hi = n_docs + 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- UTF-8 units (core::str::lossy::Utf8Chunks, as csrc/decode.hip words it) --------------------------

DEC_HD bool is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// The unit (a well-formed sequence, or a maximal invalid subpart) that starts at byte q < de, a unit
// start: its length, | 0x100 when well-formed.  Bytes from de on read as 0.
DEC_HD uint32_t unit_at(const uint8_t* raw, uint64_t de, uint64_t q) {
  const uint32_t c = raw[q];
  if (c < 0x80) return 1 | 0x100;
  const uint32_t c1 = q + 1 < de ? raw[q + 1] : 0u, c2 = q + 2 < de ? raw[q + 2] : 0u, c3 = q + 3 < de ? raw[q + 3] : 0u;
  if (c >= 0xC2 && c <= 0xDF) return is_cont(c1) ? (2 | 0x100) : 1;
  if (c >= 0xE0 && c <= 0xEF) {
    const bool ok = c == 0xE0 ? (c1 >= 0xA0 && c1 <= 0xBF) : c == 0xED ? (c1 >= 0x80 && c1 <= 0x9F) : is_cont(c1);
    if (!ok) return 1;
    return is_cont(c2) ? (3 | 0x100) : 2;
  }
  if (c >= 0xF0 && c <= 0xF4) {
    const bool ok = c == 0xF0 ? (c1 >= 0x90 && c1 <= 0xBF) : c == 0xF4 ? (c1 >= 0x80 && c1 <= 0x8F) : is_cont(c1);
    if (!ok) return 1;
    if (!is_cont(c2)) return 2;
    return is_cont(c3) ? (4 | 0x100) : 3;
  }
  return 1;
}

// the start of the unit that holds byte p of the document [ds, de): the nearest non-continuation byte
// at most 3 before p whose unit reaches p, else p itself
DEC_HD uint64_t unit_start(const uint8_t* raw, uint64_t ds, uint64_t de, uint64_t p) {
  if (!is_cont(raw[p])) return p;
  for (uint64_t k = 1; k <= 3; k++) {
    if (p - ds < k) return p;
    const uint32_t c = raw[p - k];
    if (is_cont(c)) continue;
    if (c >= 0xC0 && (unit_at(raw, de, p - k) & 0xFF) > k) return p - k;
    return p;
  }
  return p;
}

// [s, e) is well-formed UTF-8 (what a Rust String holds)
DEC_HD bool is_utf8(const uint8_t* raw, uint64_t s, uint64_t e) {
  for (uint64_t p = s; p < e;) {
    const uint32_t u = unit_at(raw, e, p);
    if (!(u & 0x100)) return false;
    p += u & 0xFF;
  }
  return true;
}

// the length of the White_Space char (char::is_whitespace, 25 code points) that [lo, hi) ends with, or 0
DEC_HD uint32_t ws_suffix(const uint8_t* b, uint64_t lo, uint64_t hi) {
  const uint64_t n = hi - lo;
  if (n < 1) return 0;
  const uint32_t c2 = b[hi - 1];
  if ((c2 >= 0x09 && c2 <= 0x0D) || c2 == 0x20) return 1;
  if (n < 2) return 0;
  const uint32_t c1 = b[hi - 2];
  if (c1 == 0xC2 && (c2 == 0x85 || c2 == 0xA0)) return 2;
  if (n < 3) return 0;
  const uint32_t c0 = b[hi - 3];
  if (c0 == 0xE1) return c1 == 0x9A && c2 == 0x80 ? 3 : 0;
  if (c0 == 0xE3) return c1 == 0x80 && c2 == 0x80 ? 3 : 0;
  if (c0 != 0xE2) return 0;
  if (c1 == 0x80) return ((c2 >= 0x80 && c2 <= 0x8A) || c2 == 0xA8 || c2 == 0xA9 || c2 == 0xAF) ? 3 : 0;
  return c1 == 0x81 && c2 == 0x9F ? 3 : 0;
}

// ---- per document ------------------------------------------------------------------------------------

// Strip: min(start, leading run of the content a) copies off the front, then min(stop, trailing run of
// what is left) off the back
DEC_HD void strip_range(const uint8_t* b, const uint8_t* a, uint64_t L, uint64_t start, uint64_t stop, uint64_t ds, uint64_t de,
                        uint64_t* lo_out, uint64_t* hi_out) {
  uint64_t lo = ds, hi = de;
  for (uint64_t k = 0; k < start && hi - lo >= L && eq(b + lo, a, L); k++) lo += L;
  for (uint64_t k = 0; k < stop && hi - lo >= L && eq(b + hi - L, a, L); k++) hi -= L;
  *lo_out = lo;
  *hi_out = hi;
}

// str::trim_end
DEC_HD void trim_range(const uint8_t* b, uint64_t ds, uint64_t de, uint64_t* lo_out, uint64_t* hi_out) {
  uint64_t hi = de;
  for (;;) {
    const uint32_t l = ws_suffix(b, ds, hi);
    if (!l) break;
    hi -= l;
  }
  *lo_out = ds;
  *hi_out = hi;
}

DEC_HD bool wp_prefixed(const Step& st, const In& in, uint64_t j) {
  const uint64_t ts = in.tok_off[j], len = in.tok_off[j + 1] - ts;
  return len >= st.a_len && eq(in.bytes + ts, st.a, st.a_len);
}

// WordPiece: the first token of document d that adds a byte to the result (kNone: none does); the
// tokens behind it find the result non-empty
DEC_HD uint64_t wp_first(const Step& st, const In& in, uint64_t d) {
  for (uint64_t j = in.doc_tok[d]; j < in.doc_tok[d + 1]; j++) {
    const uint64_t len = in.tok_off[j + 1] - in.tok_off[j];
    if (wp_prefixed(st, in, j) ? len > st.a_len : len > 0) return j;
  }
  return kNone;
}

// ---- Replace: the leftmost non-overlapping matches of a literal ------------------------------------------

DEC_HD uint8_t rep_cand(const Step& st, const uint8_t* b, uint64_t de, uint64_t p) {
  return de - p >= st.a_len && eq(b + p, st.a, st.a_len) ? 1 : 0;
}

// Candidates less than a pattern's length apart form a chain; the thread of a chain's first candidate
// walks it and marks the matches str::replace takes.  mark is zero before.
DEC_HD void rep_chain(const Step& st, const uint8_t* cand, uint8_t* mark, uint64_t ds, uint64_t de, uint64_t p) {
  const uint64_t m = st.a_len;
  if (!cand[p]) return;
  for (uint64_t k = 1; k < m && k <= p - ds; k++)
    if (cand[p - k]) return;  // not the chain's first
  uint64_t q = p;
  for (;;) {
    mark[q] = kMatchStart;
    for (uint64_t i = 1; i < m; i++) mark[q + i] = kInMatch;
    uint64_t last = q, next = kNone;
    for (uint64_t j = q + 1; j < de && j - last < m; j++) {
      if (!cand[j]) continue;
      last = j;
      if (j - q >= m) {
        next = j;
        break;
      }
    }
    if (next == kNone) return;
    q = next;
  }
}

// ---- WordPiece clean-up: eight str::replace passes that only delete spaces --------------------------------

DEC_HD bool is_set_byte(uint32_t b) {
  return b == ' ' || b == '.' || b == ',' || b == '!' || b == '?' || b == ':' || b == ';' || b == '\'';
}

struct RegAlive {  // the alive positions of a run of n <= 64 bytes
  uint64_t m;
  uint32_t n;
  DEC_HD uint32_t next(uint32_t k) const {  // the first alive > k (n: none); k = ~0u: the first
    const uint64_t r = k == 0xFFFFFFFFu ? m : (k >= 63 ? 0ull : (m & (~0ull << (k + 1))));
    return r ? (uint32_t)__builtin_ctzll(r) : n;
  }
  DEC_HD void kill(uint32_t k) { m &= ~(1ull << k); }
};

struct MemAlive {  // a longer run: the dead positions are the marks, which the run's thread alone touches
  uint8_t* mark;
  uint32_t n;
  DEC_HD uint32_t next(uint32_t k) const {
    uint32_t j = k == 0xFFFFFFFFu ? 0 : k + 1;
    while (j < n && mark[j]) j++;
    return j;
  }
  DEC_HD void kill(uint32_t k) { mark[k] = kDead; }
};

template <typename A>
DEC_HD void replay_run(const uint8_t* run, A& al) {
  // pass k: the pattern and whether the space is its first (1) or second (2) byte
  const uint8_t pat[8][3] = {{' ', '.', 1}, {' ', ',', 1}, {' ', '!', 1}, {' ', '?', 1},
                             {' ', ':', 1}, {' ', ';', 1}, {' ', '\'', 1}, {'\'', ' ', 2}};
  const uint32_t n = al.n;
  for (int k = 0; k < 8; k++) {
    const uint32_t p0 = pat[k][0], p1 = pat[k][1], sp = pat[k][2];
    uint32_t i = al.next(0xFFFFFFFFu);
    while (i < n) {
      const uint32_t j = al.next(i);
      if (j >= n) break;
      if (run[i] == p0 && run[j] == p1) {
        al.kill(sp == 1 ? i : j);
        i = al.next(j);
      } else {
        i = j;
      }
    }
  }
}

// Byte p of the document [ds, de): when a run of set bytes starts there, the passes over it; the
// deleted spaces are marked.  mark is zero before.  A run is shorter than 4 GiB (the batch is).
DEC_HD void cleanup_run(const uint8_t* b, uint8_t* mark, uint64_t ds, uint64_t de, uint64_t p) {
  if (!is_set_byte(b[p])) return;
  if (p > ds && is_set_byte(b[p - 1])) return;
  uint64_t e = p + 1;
  while (e < de && is_set_byte(b[e])) e++;
  const uint32_t n = (uint32_t)(e - p);
  if (n < 2) return;
  if (n <= 64) {
    const uint64_t all = n == 64 ? ~0ull : ((1ull << n) - 1);
    RegAlive al{all, n};
    replay_run(b + p, al);
    const uint64_t dead = ~al.m & all;
    for (uint32_t q = 0; q < n; q++)
      if ((dead >> q) & 1ull) mark[p + q] = kDead;
  } else {
    MemAlive al{mark + p, n};
    replay_run(b + p, al);
  }
}

// ---- what a unit emits -----------------------------------------------------------------------------------

// the byte of code point 0x100 + k of the GPT-2 byte map: the k-th byte outside '!'..'~', A1..AC, AE..FF
DEC_HD uint32_t bl_extra(uint32_t k) { return k <= 32 ? k : k <= 66 ? 0x7Fu + (k - 33) : 0xADu; }

DEC_HD bool ms_match(const Step& st, const uint8_t* b, uint64_t de, uint64_t q) {
  return de - q >= st.a_len && eq(b + q, st.a, st.a_len);
}

// byte p of document d = [ds, de): the bytes it emits (written to out unless out is null)
DEC_HD uint64_t byte_emit(const Step& st, const In& in, uint64_t d, uint64_t ds, uint64_t de, uint64_t p, uint8_t* out) {
  const uint8_t* b = in.bytes;
  const uint32_t c = b[p];
  switch (st.op) {
    case OP_FUSE:
      if (out) out[0] = (uint8_t)c;
      return 1;
    case OP_BL_MAP: {
      uint32_t v;
      if (c < 0x80) {
        v = c;
      } else {
        if (c < 0xC2 || c > 0xC5 || p + 1 >= de || !is_cont(b[p + 1])) return 0;
        const uint32_t cp = ((c & 0x1Fu) << 6) | (b[p + 1] & 0x3Fu);
        if ((cp >= 0xA1 && cp <= 0xAC) || (cp >= 0xAE && cp <= 0xFF)) v = cp;
        else if (cp >= 0x100 && cp <= 0x143) v = bl_extra(cp - 0x100);
        else return 0;
      }
      if (out) out[0] = (uint8_t)v;
      return 1;
    }
    case OP_LOSSY: {
      if (c < 0x80) {
        if (out) out[0] = (uint8_t)c;
        return 1;
      }
      const uint64_t u0 = unit_start(b, ds, de, p);
      const bool valid = unit_at(b, de, u0) & 0x100;
      if (valid) {
        if (out) out[0] = (uint8_t)c;
        return 1;
      }
      if (u0 != p) return 0;
      if (out) out[0] = 0xEF, out[1] = 0xBF, out[2] = 0xBD;
      return 3;
    }
    case OP_METASPACE: {
      uint32_t v = c;
      if (ms_match(st, b, de, p)) {
        v = ' ';
      } else {
        for (uint64_t k = 1; k < st.a_len && k <= p - ds; k++)
          if (ms_match(st, b, de, p - k)) return 0;  // (a code point's UTF-8 never overlaps itself)
      }
      if ((st.flags & 1u) && p == ds && v == ' ') return 0;
      if (out) out[0] = (uint8_t)v;
      return 1;
    }
    case OP_RANGE:
      if (p < in.lo[d] || p >= in.hi[d]) return 0;
      if (out) out[0] = (uint8_t)c;
      return 1;
    case OP_MARK:
      if (in.mark[p] == kInMatch) return 0;
      if (in.mark[p] == kMatchStart) {
        if (out) put(out, st.b, st.b_len);
        return st.b_len;
      }
      if (out) out[0] = (uint8_t)c;
      return 1;
    case OP_INSERT: {
      const uint64_t r = is_cont(c) ? 0 : st.b_len;
      if (out) {
        put(out, st.b, r);
        out[r] = (uint8_t)c;
      }
      return r + 1;
    }
    case OP_DEAD:
      if (in.mark[p]) return 0;
      if (out) out[0] = (uint8_t)c;
      return 1;
    default:
      return 0;
  }
}

DEC_HD bool tok_is(const In& in, uint64_t j, const uint8_t* s, uint64_t len) {
  const uint64_t ts = in.tok_off[j];
  return in.tok_off[j + 1] - ts == len && eq(in.bytes + ts, s, len);
}
// CTC: 1 the pad token (the pad test comes first), 2 the delimiter, 0 neither
DEC_HD uint32_t ctc_class(const Step& st, const In& in, uint64_t j) {
  if (tok_is(in, j, st.a, st.a_len)) return 1;
  if ((st.flags & 1u) && tok_is(in, j, st.b, st.b_len)) return 2;
  return 0;
}

// token j of document d: the bytes it emits
DEC_HD uint64_t tok_emit(const Step& st, const In& in, uint64_t d, uint64_t j, uint8_t* out) {
  const uint64_t ts = in.tok_off[j], len = in.tok_off[j + 1] - ts;
  const uint8_t* t = in.bytes + ts;
  switch (st.op) {
    case OP_WORDPIECE: {
      if (wp_prefixed(st, in, j)) {
        if (out) put(out, t + st.a_len, len - st.a_len);
        return len - st.a_len;
      }
      const uint64_t sp = in.first[d] != kNone && j > in.first[d] ? 1 : 0;
      if (out) {
        if (sp) out[0] = ' ';
        put(out + sp, t, len);
      }
      return sp + len;
    }
    case OP_BPE: {
      if (len >= st.a_len && eq(t + len - st.a_len, st.a, st.a_len)) {
        const uint64_t l = len - st.a_len;
        if (out) {
          put(out, t, l);
          out[l] = ' ';
        }
        return l + 1;
      }
      if (out) put(out, t, len);
      return len;
    }
    case OP_CTC: {
      const uint32_t cls = ctc_class(st, in, j);
      if (cls == 1) return 0;
      if (cls == 2) {
        if (out) out[0] = ' ';
        return 1;
      }
      if (j > in.doc_tok[d] && !ctc_class(st, in, j - 1)) {
        const uint64_t ps = in.tok_off[j - 1];
        if (ts - ps == len && eq(in.bytes + ps, t, len)) return 0;  // the token before it, again
      }
      if (out) put(out, t, len);
      return len;
    }
    default:
      return 0;
  }
}

// the units of an op, and the offsets that give a unit's document
DEC_HD uint64_t n_units(const Step& st, const In& in) { return is_tok_op(st.op) ? in.n_tok : in.n; }
DEC_HD const uint64_t* unit_off(const Step& st, const In& in) { return is_tok_op(st.op) ? in.doc_tok : in.doc_off; }

DEC_HD uint64_t unit_emit(const Step& st, const In& in, uint64_t d, uint64_t u, uint8_t* out) {
  if (is_tok_op(st.op)) return tok_emit(st, in, d, u, out);
  return byte_emit(st, in, d, in.doc_off[d], in.doc_off[d + 1], u, out);
}

}  // namespace decoder
