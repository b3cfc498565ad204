// The primitive steps of the Normalizer (the reference's src/normalizers.rs:43-202), shared by the
// kernels (normalize.hip) and the CPU check (tools/normalize_check.cpp): plain integer code, no HIP
// include, no intrinsics.
//
// A step maps a packed batch (text bytes, 64-bit text offsets) to a new one.  Its work is cut into
// units: a unit starts at an input byte, emits some output bytes and never leaves its text.  A thread
// owns the units that start in a span of kSpan input bytes (span_run): once to count their output
// bytes, and, after a scan over the spans, once more to write them.  A text's new offset comes out
// of the same sums (off_run).  Nothing assumes a fixed expansion.
//
//   P_DECOMP_D/K   unit = code point: its full canonical / compatibility decomposition (Hangul
//                  algorithmic, the rest from gen/normalize_data.h)
//   P_REORDER      unit = a starter, or a whole run of non-starters: the run in canonical order,
//                  a stable sort by combining class done as one pass per class present (at most 55
//                  classes exist), so linear in the run, never quadratic
//   P_COMPOSE_C/KC unit = the code points from one stable code point (class 0, never the second of
//                  a composition), or from the text's start, up to the next: canonical composition
//   P_FILTER       unit = code point: the five ranges of is_combining_mark are dropped
//   P_CLEAN        unit = code point: bert_clean_text      P_CHINESE: bert_handle_chinese_chars
//   P_STRIP        unit = byte: kept inside the text's trim bounds (trim_bounds, one thread per text)
//   P_REPLACE      unit = an applied match or a byte outside one; the applied matches come from
//                  cand_run (candidates at every byte) and chain_run (one walker per chain)
//   P_INSERT       Replace with an empty pattern: the replacement before every code point, and
//                  once more behind every text
//   P_PREPEND / P_APPEND  a constant before / behind every text
// Every loop is bounded by its text's length (or by the pattern's), and no function reads a byte
// outside [lo, hi) of the text it is given.  Bytes that are not well-formed UTF-8 (overlong forms,
// surrogates and values past U+10FFFF included) are single raw units that every step copies.
#pragma once
#include <cstdint>

#include "lowercase_hd.h"
#include "ws_split_hd.h"

#if defined(__HIPCC__)
#define NZ_HD __host__ __device__ __forceinline__
#else
#define NZ_HD inline
#endif

// the CPU check counts inner-loop steps (tools/normalize_check.cpp --steps)
#if defined(NZ_COUNT_STEPS)
extern uint64_t nz_steps;
#define NZ_STEP() (++nz_steps)
#else
#define NZ_STEP() ((void)0)
#endif

namespace normalize {

constexpr uint32_t kSpan = 64;
constexpr uint32_t kRaw = 0xFFFFFFFFu;

// bits of a property word above the combining class (tools/gen_normalize_tables.py)
constexpr uint32_t kHasD = 1u << 8, kHasK = 1u << 9, kSecond = 1u << 10, kStableC = 1u << 11, kStableKC = 1u << 13;
constexpr uint32_t kKIsD = 1u << 15;  // the compatibility decomposition is the canonical one (only that table has it)

constexpr uint32_t kSBase = 0xAC00u, kLBase = 0x1100u, kVBase = 0x1161u, kTBase = 0x11A7u;
constexpr uint32_t kLCount = 19, kVCount = 21, kTCount = 28, kSCount = kLCount * kVCount * kTCount;

enum Prim : uint32_t {
  P_DECOMP_D, P_DECOMP_K, P_REORDER, P_COMPOSE_C, P_COMPOSE_KC, P_FILTER, P_CLEAN, P_CHINESE, P_STRIP, P_REPLACE,
  P_INSERT, P_PREPEND, P_APPEND, P_LOWER /* (lowercase.hip's kernels, not a step of this header) */
};

struct Tables {  // gen/normalize_data.h (the device's copy in normalize.hip)
  const uint16_t* run_index;  // per block of 1 << run_shift code points, the run its first one lies in
  const uint32_t* run_start;  // run r covers [run_start[r], run_start[r + 1])
  const uint16_t* run_val;
  uint32_t n_runs, n_indexed, run_shift;  // (blocks from n_indexed on share the index's last two entries)
  const uint32_t* d_cp;
  const uint32_t* d_loc;
  uint32_t n_d;
  const uint32_t* k_cp;
  const uint32_t* k_loc;
  uint32_t n_k;
  const uint32_t* kr_first;  // compatibility singles in ranges: kr_first[r] + j -> kr_to[r] + j, j < kr_count[r]
  const uint16_t* kr_count;
  const uint32_t* kr_to;
  uint32_t n_kr;
  const uint32_t* pool;
  const uint64_t* comp_key;
  const uint32_t* comp_to;
  uint32_t n_comp;
};

struct Step {  // a primitive step as its threads see it
  uint32_t kind;
  uint32_t a_len, b_len;
  const uint8_t* a;      // Replace: the pattern; Prepend / Append: the string
  const uint8_t* b;      // Replace / Insert: the replacement
  const uint8_t* cand;   // Replace: cand[p] = 1: the pattern matches at byte p, inside p's text
  const uint8_t* taken;  // Replace: taken[p] = 1: the match at p is applied
  const uint64_t* trim;  // Strip: text d keeps the bytes [trim[2d], trim[2d + 1])
};

// bytes a step puts before and behind every text, whatever the text is
NZ_HD uint64_t pre_len(const Step& st) { return st.kind == P_PREPEND ? st.a_len : 0; }
NZ_HD uint64_t post_len(const Step& st) { return st.kind == P_APPEND ? st.a_len : st.kind == P_INSERT ? st.b_len : 0; }

// where a unit's output goes: out + shift + n (nothing is written when out is null)
struct Sink {
  uint8_t* out;
  uint64_t shift;
  uint64_t n;
};

NZ_HD void put_cp(Sink& s, uint32_t c) {
  if (s.out) (void)lowercase::put(s.out + s.shift + s.n, c);
  s.n += lowercase::utf8_len(c);
}

NZ_HD void put_bytes(Sink& s, const uint8_t* src, uint64_t len) {
  if (s.out)
    for (uint64_t j = 0; j < len; j++) s.out[s.shift + s.n + j] = src[j];
  s.n += len;
}

// the scalar value that starts at byte p (p < hi) and its length; kRaw / 1 when none does
NZ_HD uint32_t dec(const uint8_t* t, uint64_t hi, uint64_t p, uint32_t* len) {
  const uint32_t c = lowercase::decode(t, hi, p, len);
  if (c != kRaw && c >= 0x80u &&
      (*len != lowercase::utf8_len(c) || c > 0x10FFFFu || (c >= 0xD800u && c < 0xE000u))) {
    *len = 1;
    return kRaw;
  }
  return c;
}

// where the unit of dec() that ends at byte p (lo < p) starts: looks back at most 4 bytes
NZ_HD uint64_t prev_start(const uint8_t* t, uint64_t lo, uint64_t p) {
  uint64_t r = p - 1;
  for (int back = 1; back < 4 && r > lo && lowercase::is_cont(t[r]); back++) r--;
  uint32_t l;
  (void)dec(t, p, r, &l);
  return r + l == p ? r : p - 1;
}

// byte p of the text [lo, hi) starts a unit of dec()
NZ_HD bool is_start(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t p) {
  if (!lowercase::is_cont(t[p])) return true;
  uint64_t r = p;
  for (int back = 0; back < 3 && r > lo; back++) {
    r--;
    if (!lowercase::is_cont(t[r])) {
      uint32_t l;
      (void)dec(t, hi, r, &l);
      return r + l <= p;
    }
  }
  return true;
}

// a raw byte has class 0, composes with nothing and is stable under every form
NZ_HD uint32_t props(const Tables& T, uint32_t c) {
  if (c == kRaw) return kStableC | kStableKC;
  const uint32_t b = c >> T.run_shift < T.n_indexed ? c >> T.run_shift : T.n_indexed;
  uint32_t lo = T.run_index[b], hi = T.run_index[b + 1];  // the last run among them that starts at or before c
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (T.run_start[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return T.run_val[lo];
}
NZ_HD uint32_t ccc(const Tables& T, uint32_t c) { return props(T, c) & 0xFFu; }

// the full decomposition of c into s; false (nothing emitted) when c is its own
NZ_HD bool decompose(const Tables& T, uint32_t c, bool compat, Sink& s) {
  if (c == kRaw || c < 0xA0u) return false;
  if (c - kSBase < kSCount) {
    const uint32_t i = c - kSBase;
    put_cp(s, kLBase + i / (kVCount * kTCount));
    put_cp(s, kVBase + i % (kVCount * kTCount) / kTCount);
    if (i % kTCount) put_cp(s, kTBase + i % kTCount);
    return true;
  }
  const uint32_t pr = props(T, c);
  if (!(pr & (compat ? kHasK : kHasD))) return false;
  if (pr & kKIsD) compat = false;
  if (compat) {
    uint32_t lo = 0, hi = T.n_kr;  // the first range that starts past c
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (T.kr_first[mid] <= c) lo = mid + 1;
      else hi = mid;
    }
    if (lo && c - T.kr_first[lo - 1] < T.kr_count[lo - 1]) {
      put_cp(s, T.kr_to[lo - 1] + (c - T.kr_first[lo - 1]));
      return true;
    }
  }
  const uint32_t* cp = compat ? T.k_cp : T.d_cp;
  uint32_t lo = 0, hi = compat ? T.n_k : T.n_d;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cp[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t loc = (compat ? T.k_loc : T.d_loc)[lo];  // (the property bit says c is there)
  for (uint32_t j = 0; j < (loc & 31u); j++) put_cp(s, T.pool[(loc >> 5) + j]);
  return true;
}

// the primary composite of (a, b), or 0
NZ_HD uint32_t compose(const Tables& T, uint32_t a, uint32_t b) {
  if (a == kRaw || b == kRaw) return 0;
  if (a - kLBase < kLCount && b - kVBase < kVCount) return kSBase + ((a - kLBase) * kVCount + (b - kVBase)) * kTCount;
  if (a - kSBase < kSCount && (a - kSBase) % kTCount == 0 && b - (kTBase + 1) < kTCount - 1) return a + (b - kTBase);
  if (!(props(T, b) & kSecond)) return 0;
  const uint64_t key = (uint64_t)a << 21 | b;
  uint32_t lo = 0, hi = T.n_comp;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (T.comp_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < T.n_comp && T.comp_key[lo] == key ? T.comp_to[lo] : 0;
}

NZ_HD bool is_accent(uint32_t c) {  // is_combining_mark, src/normalizers.rs:188-202: not category M
  return (c >= 0x300u && c <= 0x36Fu) || (c >= 0x1AB0u && c <= 0x1AFFu) || (c >= 0x1DC0u && c <= 0x1DFFu) ||
         (c >= 0x20D0u && c <= 0x20FFu) || (c >= 0xFE20u && c <= 0xFE2Fu);
}

NZ_HD bool is_control(uint32_t c) {  // is_control_char, :138-146
  if (c == 9u || c == 10u || c == 13u) return false;
  return c <= 0x1Fu || (c >= 0x7Fu && c <= 0x9Fu);
}

NZ_HD bool is_chinese(uint32_t c) {  // is_chinese_char_bert, :164-176
  return (c >= 0x4E00u && c <= 0x9FFFu) || (c >= 0x3400u && c <= 0x4DBFu) || (c >= 0x20000u && c <= 0x2A6DFu) ||
         (c >= 0x2A700u && c <= 0x2B73Fu) || (c >= 0x2B740u && c <= 0x2B81Fu) || (c >= 0x2B820u && c <= 0x2CEAFu) ||
         (c >= 0xF900u && c <= 0xFAFFu) || (c >= 0x2F800u && c <= 0x2FA1Fu);
}

// ---- canonical ordering ------------------------------------------------------------------------------

// The run of non-starters that starts at p (the code point at p has class first != 0) of the text
// [.., hi), in canonical order; returns the run's end.  One pass finds the end and whether the run is
// in order already; if not, one pass per class present emits that class's code points in their input
// order (a stable counting sort without the counters) and finds the next class.
NZ_HD uint64_t reorder_run(const Tables& T, const uint8_t* t, uint64_t hi, uint64_t p, Sink& s, bool* changed) {
  uint64_t e = p;
  uint32_t last = 0, lowest = 255;
  bool sorted = true;
  while (e < hi) {
    uint32_t l;
    const uint32_t cc = ccc(T, dec(t, hi, e, &l));
    if (!cc) break;
    NZ_STEP();
    if (cc < last) sorted = false;
    if (cc < lowest) lowest = cc;
    last = cc;
    e += l;
  }
  if (sorted) {
    put_bytes(s, t + p, e - p);
    return e;
  }
  *changed = true;
  for (uint32_t cls = lowest; cls < 256;) {
    uint32_t next = 256;
    for (uint64_t q = p; q < e;) {
      uint32_t l;
      const uint32_t cc = ccc(T, dec(t, hi, q, &l));
      NZ_STEP();
      if (cc == cls) put_bytes(s, t + q, l);
      else if (cc > cls && cc < next) next = cc;
      q += l;
    }
    cls = next;
  }
  return e;
}

// ---- canonical composition ---------------------------------------------------------------------------

// One starter at p (of text [.., hi)) with what follows it up to the next starter that does not
// compose: the composed starter, then the code points left over, in order.  Pass 1 finds the final
// starter, pass 2 emits the others (emit = false: pass 1 alone, its result in *k_out).  A code
// point c composes with the starter k when compose(k, c) exists and no code point left over since
// the starter has a class >= c's (UAX #15: c is not blocked).  Returns where the next one starts.
NZ_HD uint64_t compose_walk(const Tables& T, const uint8_t* t, uint64_t hi, uint64_t p, uint32_t first, uint32_t len,
                            Sink* s, uint32_t* k_out, bool* changed) {
  uint32_t k = first, last = 0;  // last: the class of the last code point left over, 0 when none is
  uint64_t q = p + len;
  while (q < hi) {
    uint32_t l;
    const uint32_t c = dec(t, hi, q, &l);
    const uint32_t cc = ccc(T, c);
    NZ_STEP();
    uint32_t r = 0;
    if (last == 0 || last < cc) r = compose(T, k, c);
    if (r) {
      k = r;
      *changed = true;
    } else {
      if (cc == 0) break;  // the next starter
      last = cc;
      if (s) put_bytes(*s, t + q, l);
    }
    q += l;
  }
  *k_out = k;
  return q;
}

// the unit of P_COMPOSE that starts at p: up to the next stable code point or the text's end
NZ_HD uint64_t compose_unit(const Tables& T, uint32_t stable_bit, const uint8_t* t, uint64_t hi, uint64_t p, Sink& s,
                            bool* changed) {
  uint64_t q = p;
  while (q < hi) {
    uint32_t l;
    const uint32_t c = dec(t, hi, q, &l);
    const uint32_t pr = props(T, c);
    if (q != p && (pr & stable_bit)) break;
    NZ_STEP();
    if (pr & 0xFFu) {  // a non-starter with no starter before it
      put_bytes(s, t + q, l);
      q += l;
      continue;
    }
    uint32_t k;
    bool ch = false;
    const uint64_t e = compose_walk(T, t, hi, q, c, l, nullptr, &k, &ch);
    if (!ch) {
      put_bytes(s, t + q, e - q);  // (nothing composed: the input's own bytes)
    } else {
      *changed = true;
      put_cp(s, k);
      (void)compose_walk(T, t, hi, q, c, l, &s, &k, &ch);
    }
    q = e;
  }
  return q;
}

// ---- Strip and Replace: what their units read ------------------------------------------------------

// str::trim of the text [lo, hi): the bytes kept are [*a, *b)
NZ_HD void trim_bounds(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t* a, uint64_t* b) {
  uint64_t p = lo;
  while (p < hi) {
    uint32_t l;
    const uint32_t c = dec(t, hi, p, &l);
    if (c == kRaw || !wsplit::ws_at(t, hi, p)) break;
    NZ_STEP();
    p += l;
  }
  uint64_t q = hi;
  while (q > p) {
    const uint64_t r = prev_start(t, p, q);
    uint32_t l;
    const uint32_t c = dec(t, q, r, &l);
    if (c == kRaw || !wsplit::ws_at(t, q, r)) break;
    NZ_STEP();
    q = r;
  }
  *a = p;
  *b = q;
}

// the text of byte p < doc_off[n_docs]: the d with doc_off[d] <= p < doc_off[d + 1]
NZ_HD uint64_t doc_of(const uint64_t* doc_off, uint64_t n_docs, uint64_t p) {
  uint64_t lo = 0, hi = n_docs;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (doc_off[mid + 1] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// cand[p] for the bytes of [b0, b1): the pattern (a_len >= 1) matches at p and ends inside p's text
NZ_HD void cand_run(const Step& st, const uint8_t* t, const uint64_t* doc_off, uint64_t n_docs, uint64_t b0, uint64_t b1,
                    uint8_t* cand) {
  uint64_t d = doc_of(doc_off, n_docs, b0);
  for (uint64_t p = b0; p < b1; p++) {
    while (d + 1 < n_docs && p >= doc_off[d + 1]) d++;
    const uint64_t hi = doc_off[d + 1];
    bool m = st.a_len <= hi - p;
    for (uint32_t j = 0; m && j < st.a_len; j++) m = t[p + j] == st.a[j];
    cand[p] = m ? 1 : 0;
  }
}

// str::replace applies the matches leftmost first, none overlapping one before it.  Candidates
// closer than the pattern's length to the candidate before them form a chain; a chain's first
// candidate is applied whatever lies before it, and the chain is walked from there by the thread
// that owns the first candidate's byte.  A chain lies inside one text (cand_run), so does the walk.
NZ_HD void chain_run(const Step& st, const uint64_t* doc_off, uint64_t n_docs, uint64_t b0, uint64_t b1, uint8_t* taken) {
  const uint64_t L = st.a_len;
  uint64_t d = doc_of(doc_off, n_docs, b0);
  for (uint64_t p = b0; p < b1; p++) {
    if (!st.cand[p]) continue;
    while (d + 1 < n_docs && p >= doc_off[d + 1]) d++;
    const uint64_t lo = doc_off[d], hi = doc_off[d + 1];
    bool head = true;
    for (uint64_t q = p; head && q > lo && p - (q - 1) < L; q--) head = !st.cand[q - 1];
    if (!head) continue;
    uint64_t cur = p, last = p;  // cur: the last applied match; last: the last candidate seen
    taken[p] = 1;
    for (uint64_t r = p + 1; r < hi && r - last < L; r++) {
      NZ_STEP();
      if (!st.cand[r]) continue;
      last = r;
      if (r - cur >= L) {
        taken[r] = 1;
        cur = r;
      }
    }
  }
}

// the first byte at or after b0 that no applied match that starts before b0 covers
NZ_HD uint64_t replace_resume(const Step& st, uint64_t b0) {
  for (uint64_t q = b0; q > 0 && b0 - (q - 1) < st.a_len; q--)
    if (st.taken[q - 1]) return q - 1 + st.a_len;
  return b0;
}

// ---- the units ---------------------------------------------------------------------------------------

// The unit that starts at byte p of text d = [lo, hi), into s; returns how many input bytes to go
// on by (>= 1; the bytes skipped start no unit).  A byte that starts no unit emits nothing.
NZ_HD uint64_t unit(const Tables& T, const Step& st, const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t d, uint64_t p,
                    Sink& s, bool* changed) {
  switch (st.kind) {
    case P_STRIP:
      if (p >= st.trim[2 * d] && p < st.trim[2 * d + 1]) put_bytes(s, t + p, 1);
      else *changed = true;
      return 1;
    case P_REPLACE:
      if (st.taken[p]) {
        put_bytes(s, st.b, st.b_len);
        *changed = true;
        return st.a_len;
      }
      put_bytes(s, t + p, 1);
      return 1;
    case P_PREPEND:
    case P_APPEND:
      *changed = true;
      put_bytes(s, t + p, 1);
      return 1;
    default:
      break;
  }
  if (!is_start(t, lo, hi, p)) return 1;
  uint32_t l;
  const uint32_t c = dec(t, hi, p, &l);
  switch (st.kind) {
    case P_DECOMP_D:
    case P_DECOMP_K:
      if (decompose(T, c, st.kind == P_DECOMP_K, s)) *changed = true;
      else put_bytes(s, t + p, l);
      return l;
    case P_REORDER: {
      if (!ccc(T, c)) {
        put_bytes(s, t + p, l);
        return l;
      }
      if (p > lo) {  // inside a run: the run's first code point owns it
        const uint64_t r = prev_start(t, lo, p);
        uint32_t l2;
        if (ccc(T, dec(t, p, r, &l2))) return l;
      }
      return reorder_run(T, t, hi, p, s, changed) - p;
    }
    case P_COMPOSE_C:
    case P_COMPOSE_KC: {
      const uint32_t bit = st.kind == P_COMPOSE_C ? kStableC : kStableKC;
      if (p > lo && !(props(T, c) & bit)) return l;
      return compose_unit(T, bit, t, hi, p, s, changed) - p;
    }
    case P_FILTER:
      if (c != kRaw && is_accent(c)) *changed = true;
      else put_bytes(s, t + p, l);
      return l;
    case P_CLEAN:
      if (c != kRaw && is_control(c)) {
        *changed = true;
      } else if (c != kRaw && wsplit::ws_at(t, hi, p)) {
        if (c != 0x20u) *changed = true;
        put_cp(s, 0x20u);
      } else {
        put_bytes(s, t + p, l);
      }
      return l;
    case P_CHINESE:
      if (c != kRaw && is_chinese(c)) {
        *changed = true;
        put_cp(s, 0x20u);
        put_bytes(s, t + p, l);
        put_cp(s, 0x20u);
      } else {
        put_bytes(s, t + p, l);
      }
      return l;
    case P_INSERT:
      *changed = true;
      put_bytes(s, st.b, st.b_len);
      put_bytes(s, t + p, l);
      return l;
    default:
      return l;
  }
}

// The output bytes of the units that start in [b0, b1) (b1 <= the batch's bytes), written behind
// out (the place of the span's first byte, before the texts' constants) when out is non-null.
NZ_HD uint64_t span_run(const Tables& T, const Step& st, const uint8_t* t, const uint64_t* doc_off, uint64_t n_docs,
                        uint64_t b0, uint64_t b1, uint8_t* out, bool* changed) {
  const uint64_t pre = pre_len(st), both = pre + post_len(st);
  uint64_t d = doc_of(doc_off, n_docs, b0);
  Sink s{out, d * both + pre, 0};
  uint64_t p = st.kind == P_REPLACE ? replace_resume(st, b0) : b0;
  while (p < b1) {
    while (d + 1 < n_docs && p >= doc_off[d + 1]) {
      d++;
      s.shift = d * both + pre;
    }
    p += unit(T, st, t, doc_off[d], doc_off[d + 1], d, p, s, changed);
  }
  return s.n;
}

// Text d's new offset (d <= n_docs) from pos, the exclusive scan of the spans' counts with the
// total at pos[n_spans]; with out non-null also writes the constants around the text's edge.
NZ_HD uint64_t off_run(const Tables& T, const Step& st, const uint8_t* t, uint64_t n_bytes, const uint64_t* doc_off,
                       uint64_t n_docs, uint64_t n_spans, const uint64_t* pos, uint64_t d, uint8_t* out) {
  const uint64_t pre = pre_len(st), post = post_len(st), o = doc_off[d];
  uint64_t at;
  if (o >= n_bytes) {
    at = pos[n_spans];
  } else {
    bool ch = false;
    at = pos[o / kSpan] + span_run(T, st, t, doc_off, n_docs, o / kSpan * kSpan, o, nullptr, &ch);
  }
  at += d * (pre + post);
  if (out) {
    const uint8_t* src = st.kind == P_INSERT ? st.b : st.a;
    if (d < n_docs)
      for (uint64_t j = 0; j < pre; j++) out[at + j] = src[j];
    if (d > 0)
      for (uint64_t j = 0; j < post; j++) out[at - post + j] = src[j];
  }
  return at;
}

}  // namespace normalize
