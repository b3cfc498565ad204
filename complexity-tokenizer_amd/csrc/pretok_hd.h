// The rules of the PreTokenizer (the reference's src/pretokenizers.rs:69-594), shared by the kernels
// (pretok.hip) and the CPU check (tools/pretok_check.cpp): plain integer code, no HIP include, no
// intrinsics but the compilers' popcount builtin.
//
// A batch is its bytes and two bitmaps, one 64-bit word per 64 bytes: in_word (the byte belongs to a
// word) and begin (a word starts at the byte; begin implies in_word).  A word is a begin byte and the
// in_word bytes behind it up to the next begin, the next byte outside a word or the buffer's end, so
// words never cross texts: every non-empty text starts as one word.
//
//   pure splitters   everything but ByteLevel and Metaspace: split_bits() gives byte p's two new bits
//                    from the text and the old bitmaps.  A rule reads the code point at p, its
//                    predecessor in the same word and a bounded neighbourhood (GPT2_PATTERN: three
//                    bytes either way, as csrc/seg_lane.h words it).  Three things come from outside:
//                    the literal and DFA matches of `split` (lit_cand / lit_chain and dfa_len /
//                    dfa_walk mark them), whether a word
//                    holds a match at all (Removed without invert keeps a word that holds none), and
//                    the script carry of UnicodeScripts (script_val: the caller finds the nearest
//                    value before p).
//   rewriters        ByteLevel and Metaspace: rw_unit() gives the output bytes of input byte p and
//                    whether a word begins there; the caller counts, scans and writes.  Every byte
//                    a rewriter emits is inside a word.
// No function reads a byte outside [0, n) of the buffer or past its word's end.  Bytes that are not
// well-formed UTF-8 are single units (kRaw): no whitespace, punctuation, digit, letter or number, of
// script Unknown.
#pragma once
#include <cstdint>

#include "normalize_hd.h"

namespace pretok {

using normalize::kRaw;

constexpr uint32_t kSpan = 64;  // bytes per bitmap word: one wavefront's lanes

enum Kind : uint32_t {  // include/ctok_pretokenizer.h
  K_WHITESPACE, K_WHITESPACE_SPLIT, K_BYTE_LEVEL, K_METASPACE, K_PUNCTUATION, K_DIGITS, K_GPT2, K_BERT, K_CHAR_DELIM,
  K_SCRIPTS, K_SPLIT
};
enum Behavior : uint32_t { B_REMOVED, B_ISOLATED, B_MERGED_PREV, B_MERGED_NEXT, B_CONTIGUOUS };
enum Mode : uint32_t { M_IDENTITY, M_LITERAL, M_CLASS, M_DFA };  // how a `split` pattern runs
constexpr uint32_t kInvert = 8;                                  // flag bit of `split`
constexpr uint32_t kRegex = 16;                                  // flag bit of `split`: a general pattern may run as a DFA
// class items: type, lo, hi (three u32 each)
enum Item : uint32_t { I_RANGE, I_SPACE, I_DIGIT, I_LETTER, I_NUMBER, I_NEG = 0x100 };
// script values of script_val: 0 = nothing to say (Common, or no lead byte), kReset = a word ends or starts
constexpr uint32_t kCommon = 0, kUnknown = 11, kReset = 15;
// marks of the applied matches (literal and DFA)
constexpr uint8_t kInMatch = 1, kMatchStart = 2;
// a DFA transition entry (regex_dfa.h): kDfaDead, or the next state with kDfaAccept when it holds a match
constexpr uint16_t kDfaDead = 0xFFFF, kDfaAccept = 0x8000, kDfaState = 0x0FFF;
constexpr uint32_t kMaxUnit = 8;  // output bytes of one input byte under a rewriter: Metaspace, two replacements

struct Tables {
  const uint8_t* cls_s1;  // gen/unicode_data.h ct_cls_stage1 / ct_cls_stage2: 0 \s, 1 \p{L}, 2 \p{N}, 3 other
  const uint8_t* cls_s2;
  const uint32_t* nd_lo;  // gen/pretok_data.h
  const uint32_t* nd_hi;
  uint32_t n_nd;
};

// A general `split` pattern as regex_dfa.h compiled it.
struct Dfa {
  const uint16_t* trans;   // [state][symbol]
  const uint8_t* ascii;    // symbol of a code point below 0x80
  const uint32_t* bounds;  // interval starts, bounds[0] = 0
  const uint8_t* symmap;   // [interval][cls * 2 + nd]
  uint32_t n_bounds, n_symbols, n_states, raw_sym, use, start;
  uint32_t cap;            // code points a start may step through (the work bound of a cyclic DFA)
};

struct Step {
  uint32_t kind, flags, cp;
  uint32_t mode, plus, neg, n_items;  // split
  const uint32_t* items;              // split, M_CLASS
  const uint8_t* lit;                 // split, M_LITERAL: the literal's bytes
  uint32_t lit_len;
  uint32_t cp_len;                    // Metaspace: the replacement's UTF-8
  uint8_t cp_u8[4];
  const uint8_t* cand;                // literal: cand[p] = 1: the literal matches at p, inside p's word
  const uint8_t* mark;                // literal, DFA: kInMatch / kMatchStart of the applied matches
  Dfa dfa;                            // split, M_DFA
  const uint64_t* wpos;               // Removed: words that begin before bitmap word j
  const uint8_t* whit;                // Removed: whit[w] = 1: word w holds a match
};

struct Ctx {
  const uint8_t* t;
  uint64_t n;
  const uint64_t* inw;
  const uint64_t* beg;
};

NZ_HD bool bit(const uint64_t* bm, uint64_t i) { return (bm[i >> 6] >> (i & 63)) & 1u; }
NZ_HD bool in_word(const Ctx& x, uint64_t p) { return bit(x.inw, p); }
// p (inside a word) has a byte of the same word before it
NZ_HD bool has_prev(const Ctx& x, uint64_t p) { return p > 0 && !bit(x.beg, p) && bit(x.inw, p - 1); }
// q (inside a word) is the word's last byte
NZ_HD bool is_last(const Ctx& x, uint64_t q) { return q + 1 >= x.n || !bit(x.inw, q + 1) || bit(x.beg, q + 1); }

// where a unit that starts at r may end at most: 4 bytes on, the word's end or the buffer's
NZ_HD uint64_t unit_hi(const Ctx& x, uint64_t r) {
  uint64_t q = r + 1;
  while (q < r + 4 && q < x.n && bit(x.inw, q) && !bit(x.beg, q)) q++;
  return q;
}
NZ_HD uint32_t cp_at(const Ctx& x, uint64_t r, uint32_t* len) { return normalize::dec(x.t, unit_hi(x, r), r, len); }
// the first byte of the unit that holds byte p (inside a word): looks back at most 3 bytes
NZ_HD uint64_t unit_lead(const Ctx& x, uint64_t p) {
  if (!lowercase::is_cont(x.t[p])) return p;
  uint64_t r = p;
  for (int back = 0; back < 3 && has_prev(x, r); back++) {
    r--;
    if (!lowercase::is_cont(x.t[r])) {
      uint32_t l;
      (void)cp_at(x, r, &l);
      return r + l > p ? r : p;
    }
  }
  return p;
}

// ---- classes -------------------------------------------------------------------------------------------

NZ_HD bool is_ws(uint32_t c) {  // char::is_whitespace: the 25 White_Space code points
  if (c < 0x80u) return (c >= 9u && c <= 13u) || c == 0x20u;
  return c == 0x85u || c == 0xA0u || c == 0x1680u || (c >= 0x2000u && c <= 0x200Au) || c == 0x2028u || c == 0x2029u ||
         c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}
NZ_HD bool is_punct(uint32_t c) {  // is_ascii_punctuation || is_unicode_punctuation, :227-240
  return (c >= 0x21u && c <= 0x2Fu) || (c >= 0x3Au && c <= 0x40u) || (c >= 0x5Bu && c <= 0x60u) ||
         (c >= 0x7Bu && c <= 0x7Eu) || (c >= 0xA1u && c <= 0xBFu) || (c >= 0x2000u && c <= 0x206Fu) ||
         (c >= 0x2E00u && c <= 0x2E7Fu) || (c >= 0x3000u && c <= 0x303Fu);
}
NZ_HD bool is_chinese(uint32_t c) {  // is_chinese_char, :482-496
  return (c >= 0x4E00u && c <= 0x9FFFu) || (c >= 0x3400u && c <= 0x4DBFu) || (c >= 0x20000u && c <= 0x2A6DFu) ||
         (c >= 0x2A700u && c <= 0x2B73Fu) || (c >= 0x2B740u && c <= 0x2B81Fu) || (c >= 0x2B820u && c <= 0x2CEAFu) ||
         (c >= 0x2CEB0u && c <= 0x2EBEFu) || (c >= 0x30000u && c <= 0x3134Fu) || (c >= 0xF900u && c <= 0xFAFFu) ||
         (c >= 0x2F800u && c <= 0x2FA1Fu);
}
NZ_HD bool is_ascii_digit(uint32_t c) { return c >= '0' && c <= '9'; }

// get_unicode_script, :566-594: 1 Latin .. 10 Thai in the arms' order, kCommon, kUnknown
NZ_HD uint32_t script_of(uint32_t c) {
  if (c == kRaw) return kUnknown;
  if ((c >= 0x41u && c <= 0x7Au) || (c >= 0xC0u && c <= 0x24Fu) || (c >= 0x1E00u && c <= 0x1EFFu)) return 1;
  if ((c >= 0x370u && c <= 0x3FFu) || (c >= 0x1F00u && c <= 0x1FFFu)) return 2;
  if (c >= 0x400u && c <= 0x52Fu) return 3;
  if ((c >= 0x600u && c <= 0x6FFu) || (c >= 0x750u && c <= 0x77Fu) || (c >= 0x8A0u && c <= 0x8FFu)) return 4;
  if (c >= 0x590u && c <= 0x5FFu) return 5;
  if ((c >= 0x4E00u && c <= 0x9FFFu) || (c >= 0x3400u && c <= 0x4DBFu) || (c >= 0x20000u && c <= 0x2A6DFu)) return 6;
  if (c >= 0x3040u && c <= 0x309Fu) return 7;
  if ((c >= 0x30A0u && c <= 0x30FFu) || (c >= 0x31F0u && c <= 0x31FFu)) return 8;
  if ((c >= 0xAC00u && c <= 0xD7AFu) || (c >= 0x1100u && c <= 0x11FFu) || (c >= 0x3130u && c <= 0x318Fu)) return 9;
  if (c >= 0xE00u && c <= 0xE7Fu) return 10;
  if (c <= 0x40u || (c >= 0x5Bu && c <= 0x60u) || (c >= 0x7Bu && c <= 0xBFu) || (c >= 0x2000u && c <= 0x206Fu) ||
      (c >= 0x3000u && c <= 0x303Fu))
    return kCommon;
  return kUnknown;
}

// 0 \s, 1 \p{L}, 2 \p{N}, 3 other (cls_of of dev_common.h)
NZ_HD uint32_t cls(const Tables& T, uint32_t c) {
  if (c == kRaw || c >= 0x110000u) return 3;
  if (c < 0x80u) {
    if (c == 32u || (c >= 9u && c <= 13u)) return 0;
    if ((c | 32u) >= 'a' && (c | 32u) <= 'z') return 1;
    return is_ascii_digit(c) ? 2 : 3;
  }
  const uint32_t w = T.cls_s2[(uint32_t)T.cls_s1[c >> 8] * 64 + ((c & 255u) >> 2)];
  return (w >> ((c & 3u) * 2)) & 3u;
}
NZ_HD bool is_nd(const Tables& T, uint32_t c) {  // regex \d
  if (c < 0x80u) return is_ascii_digit(c);
  if (c == kRaw) return false;
  uint32_t lo = 0, hi = T.n_nd;  // the first run that starts past c
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (T.nd_lo[mid] <= c) lo = mid + 1;
    else hi = mid;
  }
  return lo && c <= T.nd_hi[lo - 1];
}

// the class atom of a `split` pattern matches c
NZ_HD bool class_match(const Tables& T, const Step& st, uint32_t c) {
  bool any = false;
  for (uint32_t i = 0; i < st.n_items && !any; i++) {
    const uint32_t type = st.items[3 * i];
    bool m;
    switch (type & 0xFFu) {
      case I_RANGE: m = c != kRaw && c >= st.items[3 * i + 1] && c <= st.items[3 * i + 2]; break;
      case I_SPACE: m = cls(T, c) == 0; break;
      case I_DIGIT: m = is_nd(T, c); break;
      case I_LETTER: m = cls(T, c) == 1; break;
      default: m = cls(T, c) == 2; break;
    }
    any = (type & I_NEG) ? !m : m;
  }
  return any != (st.neg != 0);
}

// ---- GPT2_PATTERN: a piece starts at byte p (seg_lane.h's predicate, byte by byte) -------------------
// W/L/N/other is the class of the unit a byte lies in.  prefix: ByteLevel's add_prefix_space puts a
// ' ' before a word that does not start with one; the word's first byte then continues that piece,
// and no contraction starts there.

NZ_HD uint32_t cls_b(const Tables& T, const Ctx& x, uint64_t q) {
  uint32_t l;
  return cls(T, cp_at(x, unit_lead(x, q), &l));
}
// the attached space: a single ' ' that begins the following run of non-space
NZ_HD bool g_attached(const Tables& T, const Ctx& x, uint64_t q) {
  return x.t[q] == ' ' && !is_last(x, q) && cls_b(T, x, q + 1) != 0 && (!has_prev(x, q) || cls_b(T, x, q - 1) != 0);
}
// '\'' that starts a contraction of 1 (*two = false) or 2 letters
NZ_HD bool g_contraction(const Tables& T, const Ctx& x, uint64_t q, bool prefix, bool* two) {
  if (x.t[q] != '\'' || is_last(x, q)) return false;
  if (!has_prev(x, q)) {
    if (prefix) return false;
  } else if (cls_b(T, x, q - 1) == 3 || g_attached(T, x, q - 1)) {
    return false;
  }
  const uint8_t a = x.t[q + 1];
  *two = false;
  if (a == 's' || a == 't' || a == 'm' || a == 'd') return true;
  if (is_last(x, q + 1)) return false;
  const uint8_t b = x.t[q + 2];
  *two = true;
  return ((a == 'r' || a == 'v') && b == 'e') || (a == 'l' && b == 'l');
}
NZ_HD bool gpt2_start(const Tables& T, const Ctx& x, uint64_t p, bool prefix) {
  if (!has_prev(x, p)) return true;
  if (unit_lead(x, p) != p) return false;
  const uint32_t c = cls_b(T, x, p);
  bool two;
  if (c != cls_b(T, x, p - 1)) return !g_attached(T, x, p - 1) && !g_contraction(T, x, p - 1, prefix, &two);
  if (c != 1 || !has_prev(x, p - 1)) return false;
  if (g_contraction(T, x, p - 2, prefix, &two) && !two) return true;
  return has_prev(x, p - 2) && g_contraction(T, x, p - 3, prefix, &two) && two;
}

// ---- literal matches of `split` -----------------------------------------------------------------------

// the literal matches at p and all of it lies in p's word
NZ_HD bool lit_cand(const Step& st, const Ctx& x, uint64_t p) {
  if (!in_word(x, p) || st.lit_len > x.n - p) return false;
  for (uint32_t j = 0; j < st.lit_len; j++)
    if (x.t[p + j] != st.lit[j] || (j && (!bit(x.inw, p + j) || bit(x.beg, p + j)))) return false;
  return true;
}
// Matches are leftmost and do not overlap.  Candidates closer than the literal's length to the one
// before them form a chain; the chain's first candidate is a match whatever lies before it, and the
// thread of that byte walks the chain and marks the matches' bytes.  A chain lies inside one word.
NZ_HD void lit_chain(const Step& st, uint64_t n, uint64_t p, uint8_t* mark) {
  const uint64_t L = st.lit_len;
  if (!st.cand[p]) return;
  for (uint64_t q = p; q > 0 && p - (q - 1) < L; q--)
    if (st.cand[q - 1]) return;
  uint64_t cur = p, last = p;  // cur: the last match; last: the last candidate seen
  for (uint64_t r = p;; r++) {
    if (r == cur) {
      mark[r] = kInMatch | kMatchStart;
      for (uint64_t j = 1; j < L; j++) mark[r + j] = kInMatch;
    }
    if (r + 1 >= n || r + 1 - last >= L) break;
    if (st.cand[r + 1]) {
      last = r + 1;
      if (r + 1 - cur >= L) cur = r + 1;
    }
  }
}

// ---- DFA matches of `split` ---------------------------------------------------------------------------

NZ_HD uint32_t dfa_sym(const Tables& T, const Dfa& d, uint32_t c) {
  if (c == kRaw || c >= 0x110000u) return d.raw_sym;
  if (c < 0x80u) return d.ascii[c];
  uint32_t lo = 0, hi = d.n_bounds;  // the first interval that starts past c
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (d.bounds[mid] <= c) lo = mid + 1;
    else hi = mid;
  }
  uint32_t key = 0;
  if (d.use & 1u) {
    const uint32_t cl = cls(T, c);
    key = cl * 2 + ((d.use & 2u) && cl == 2 && is_nd(T, c) ? 1 : 0);
  }
  return d.symmap[(lo - 1) * 8 + key];
}
// The leftmost-first match that starts at byte p, in bytes; 0: none, or p is no lead byte inside a word.
// The DFA steps code point by code point to the dead state or the word's end, and the last accepting
// state it saw ends the match.  *over: the run would pass d.cap code points (then 0 is returned).
// `trans` is d.trans or a copy of it.
NZ_HD uint32_t dfa_len(const Tables& T, const Dfa& d, const uint16_t* trans, const Ctx& x, uint64_t p, bool* over) {
  *over = false;
  if (!in_word(x, p) || unit_lead(x, p) != p) return 0;
  uint32_t state = d.start, best = 0, steps = 0;
  for (uint64_t q = p; q < x.n && in_word(x, q) && (q == p || !bit(x.beg, q));) {
    if (steps == d.cap) {
      *over = true;
      return 0;
    }
    uint32_t l;
    const uint32_t c = cp_at(x, q, &l);
    const uint16_t e = trans[state * d.n_symbols + dfa_sym(T, d, c)];
    if (e == kDfaDead) break;
    state = e & kDfaState;
    q += l;
    steps++;
    if (e & kDfaAccept) best = (uint32_t)(q - p);
  }
  return best;
}
// Matches are taken left to right and do not overlap.  reach(q) is the largest p + len[p] over the
// candidates p < q; a candidate q with reach(q) <= q is a chain head, a match whatever lies before
// it.  The head's thread walks its chain: it takes the match, goes on to the first candidate at or
// after the match's end and stops where the next head would stand, that is where no candidate since
// the head reaches.  It writes only inside [p, the chain's reach), which no other chain shares.
NZ_HD void dfa_walk(const uint32_t* len, uint64_t n, uint64_t p, uint8_t* mark) {
  uint64_t cur = p, end = p + len[p], reach = end;
  for (uint64_t r = p;; r++) {
    if (r < end) mark[r] = r == cur ? (kInMatch | kMatchStart) : kInMatch;
    if (r + 1 >= n || r + 1 >= reach) break;
    const uint64_t l = len[r + 1];
    if (!l) continue;
    if (r + 1 >= end) {
      cur = r + 1;
      end = cur + l;
    }
    if (r + 1 + l > reach) reach = r + 1 + l;
  }
}

// ---- the pure splitters --------------------------------------------------------------------------------

NZ_HD bool by_marks(const Step& st) { return st.mode == M_LITERAL || st.mode == M_DFA; }
// the unit at a lead byte lies in a match of the `split` step
NZ_HD bool split_in(const Tables& T, const Step& st, const Ctx& x, uint64_t lead, uint32_t c) {
  return by_marks(st) ? (st.mark[lead] & kInMatch) != 0 : class_match(T, st, c);
}

// the word ordinal of byte p (inside a word; 0 for bytes before the first begin, which a batch
// whose doc_off[0] is 0 does not have)
NZ_HD uint64_t word_of(const Step& st, const Ctx& x, uint64_t p) {
  const uint64_t upto = (p & 63) == 63 ? ~0ull : (1ull << ((p & 63) + 1)) - 1;
  const uint64_t c = st.wpos[p >> 6] + (uint64_t)__builtin_popcountll(x.beg[p >> 6] & upto);
  return c ? c - 1 : 0;
}

// what byte p says to the script carry of UnicodeScripts
NZ_HD uint32_t script_val(const Ctx& x, uint64_t p) {
  if (!in_word(x, p)) return kReset;
  if (unit_lead(x, p) != p) return 0;
  uint32_t l;
  const uint32_t c = cp_at(x, p, &l);
  if (c != kRaw && is_ws(c)) return kReset;
  const uint32_t s = script_of(c);
  return s != kCommon ? s : !has_prev(x, p) ? kReset : 0;
}

// Byte p's new bits.  sv: UnicodeScripts only, the nearest non-zero script_val before p (0: none).
NZ_HD void split_bits(const Tables& T, const Step& st, const Ctx& x, uint64_t p, uint32_t sv, bool* in, bool* bg) {
  *in = *bg = false;
  if (!in_word(x, p)) return;
  const bool old_bg = !has_prev(x, p);
  if (st.kind == K_GPT2) {
    *in = true;
    *bg = gpt2_start(T, x, p, false);
    return;
  }
  if (st.kind == K_SPLIT && st.mode == M_IDENTITY) {
    *in = true;
    *bg = old_bg;
    return;
  }
  const uint64_t lead = unit_lead(x, p);
  uint32_t l, lp = 0;
  const uint32_t c = cp_at(x, lead, &l);
  const bool prev = has_prev(x, lead);
  const uint64_t plead = prev ? unit_lead(x, lead - 1) : 0;
  const uint32_t pc = prev ? cp_at(x, plead, &lp) : kRaw;
  bool drop = false, pdrop = false, cut = false;
  switch (st.kind) {
    case K_WHITESPACE:
    case K_WHITESPACE_SPLIT:
      drop = is_ws(c);
      pdrop = prev && is_ws(pc);
      break;
    case K_PUNCTUATION:
      cut = is_punct(c) || (prev && is_punct(pc));
      break;
    case K_DIGITS:
      if (prev) cut = (st.flags & 1u) ? is_ascii_digit(c) || is_ascii_digit(pc) : is_ascii_digit(c) != is_ascii_digit(pc);
      break;
    case K_BERT:
      drop = is_ws(c);
      pdrop = prev && is_ws(pc);
      cut = is_chinese(c) || is_punct(c) || (prev && (is_chinese(pc) || is_punct(pc)));
      break;
    case K_CHAR_DELIM:
      drop = c == st.cp;
      pdrop = prev && pc == st.cp;
      break;
    case K_SCRIPTS: {
      drop = is_ws(c);
      pdrop = prev && is_ws(pc);
      const uint32_t s = script_of(c);
      cut = s != kCommon && sv != 0 && sv != kReset && sv != s;
      break;
    }
    default: {  // K_SPLIT
      const uint32_t b = st.flags & 7u;
      const bool m = split_in(T, st, x, lead, c), pm = prev && split_in(T, st, x, plead, pc);
      const bool s = by_marks(st) ? (st.mark[lead] & kMatchStart) != 0 : m && (!st.plus || !pm);
      if (b == B_REMOVED && (st.flags & kInvert)) {
        drop = m;
        pdrop = pm;
      } else if (b == B_REMOVED) {
        if (!st.whit[word_of(st, x, lead)]) break;  // no match in the word: the word as it is
        drop = !m;
        pdrop = prev && !pm;
        cut = s;
      } else if (b == B_ISOLATED) {
        cut = s || (pm && !m);
      } else if (b == B_MERGED_NEXT) {
        cut = s;
      } else if (b == B_MERGED_PREV) {
        cut = pm && !m;
      } else {
        cut = (s && !pm) || (pm && !m);
      }
      break;
    }
  }
  *in = !drop;
  *bg = p == lead && !drop && (old_bg || pdrop || cut);
}

// ---- the rewriters -------------------------------------------------------------------------------------

// bytes_to_unicode, :130-153: the code point a byte becomes
NZ_HD uint32_t byte_cp(uint32_t b) {
  if ((b >= 0x21u && b <= 0x7Eu) || (b >= 0xA1u && b <= 0xACu) || b >= 0xAEu) return b;
  return 256u + (b <= 0x20u ? b : b <= 0xA0u ? b - 0x7Fu + 33u : 67u);
}

// The output of input byte p into out (at most kMaxUnit bytes); *bg: a word begins at out[0].
NZ_HD uint32_t rw_unit(const Tables& T, const Step& st, const Ctx& x, uint64_t p, uint8_t* out, bool* bg) {
  *bg = false;
  if (!in_word(x, p)) return 0;
  uint32_t n = 0;
  const bool first = !has_prev(x, p);
  if (st.kind == K_BYTE_LEVEL) {
    const bool prefix = (st.flags & 1u) != 0;
    *bg = gpt2_start(T, x, p, prefix);
    if (prefix && first && x.t[p] != ' ') n += lowercase::put(out + n, byte_cp(' '));
    n += lowercase::put(out + n, byte_cp(x.t[p]));
    return n;
  }
  // Metaspace: the unit's lead byte emits the unit
  if (unit_lead(x, p) != p) return 0;
  uint32_t l, lp;
  const uint32_t c = cp_at(x, p, &l);
  const bool pre = first && (st.flags & 1u);
  if (pre) {
    for (uint32_t j = 0; j < st.cp_len; j++) out[n++] = st.cp_u8[j];
    *bg = true;
  }
  if (c == ' ') {
    for (uint32_t j = 0; j < st.cp_len; j++) out[n++] = st.cp_u8[j];
  } else if (c != kRaw && is_ws(c) && c != st.cp) {
    return n;
  } else {
    for (uint32_t j = 0; j < l; j++) out[n++] = x.t[p + j];
  }
  if (!pre) {
    *bg = first;
    if (!first) {
      const uint32_t pc = cp_at(x, unit_lead(x, p - 1), &lp);
      *bg = pc != kRaw && is_ws(pc) && pc != ' ' && pc != st.cp;
    }
  }
  return n;
}

}  // namespace pretok
