// A PreTokenizer's program: the steps of include/ctok_pretokenizer.h as the rules of pretok_hd.h take
// them, and the gates a `split` pattern goes through.  Shared by the host runtime (pretok_host.cpp)
// and the CPU check (tools/pretok_check.cpp).  Host-only; not part of the C ABI.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ctok_pretokenizer.h"
#include "pretok_hd.h"
#include "regex_dfa.h"

namespace pretok {

struct HostStep {
  uint32_t kind = 0, flags = 0, cp = 0;
  uint32_t mode = M_IDENTITY, plus = 0, neg = 0;
  std::vector<uint32_t> items;  // M_CLASS: type, lo, hi
  std::string lit;              // M_LITERAL
  regex_dfa::Dfa dfa;           // M_DFA
  std::string cp_u8;            // Metaspace: the replacement
};

inline const char* kind_name(uint32_t kind) {
  static const char* names[] = {"whitespace", "whitespace_split", "byte_level",           "metaspace",       "punctuation", "digits",
                                "gpt2",       "bert",             "char_delimiter_split", "unicode_scripts", "split"};
  return kind < sizeof(names) / sizeof(names[0]) ? names[kind] : "?";
}
inline bool rewrites(uint32_t kind) { return kind == K_BYTE_LEVEL || kind == K_METASPACE; }

enum PatternClass { PC_REJECTED = 0, PC_LITERAL = 1, PC_CLASS = 2, PC_UNSUPPORTED = 3, PC_DFA = 4 };

// Gates 2 and 3 of a pattern the Rust crate compiles: a literal, or one class atom with an optional
// '+'.  Everything else is PC_UNSUPPORTED: never split differently in silence.
inline PatternClass classify_split(const std::string& p, HostStep* out) {
  std::vector<uint32_t> cps;
  for (uint64_t i = 0; i < p.size();) {
    uint32_t l;
    const uint32_t c = normalize::dec((const uint8_t*)p.data(), p.size(), i, &l);
    if (c == kRaw) return PC_UNSUPPORTED;
    cps.push_back(c);
    i += l;
  }
  const size_t n = cps.size();
  if (!n) return PC_UNSUPPORTED;
  auto is_meta = [](uint32_t c) { return c < 0x80u && strchr("\\.+*?()|[]{}^$", (int)c) != nullptr && c != 0; };
  // at cps[i] == '\\': a one-character escape (ASCII punctuation, \n \t \r); 0xFFFFFFFF when it is none
  auto char_escape = [&](size_t i) -> uint32_t {
    if (i + 1 >= n) return kRaw;
    const uint32_t e = cps[i + 1];
    if (e == 'n') return '\n';
    if (e == 't') return '\t';
    if (e == 'r') return '\r';
    if (e == '<' || e == '>') return kRaw;  // (word-boundary assertions of regex 1.10)
    if (e < 0x80u && ((e >= 0x21u && e <= 0x2Fu) || (e >= 0x3Au && e <= 0x40u) || (e >= 0x5Bu && e <= 0x60u) ||
                      (e >= 0x7Bu && e <= 0x7Eu)))
      return e;
    return kRaw;
  };
  // at cps[i] == '\\': a class escape; its item type and length, or 0 length
  auto class_escape = [&](size_t i, uint32_t* type) -> size_t {
    if (i + 1 >= n) return 0;
    const uint32_t e = cps[i + 1];
    if (e == 's' || e == 'S') return *type = I_SPACE | (e == 'S' ? I_NEG : 0), 2;
    if (e == 'd' || e == 'D') return *type = I_DIGIT | (e == 'D' ? I_NEG : 0), 2;
    if ((e == 'p' || e == 'P') && i + 4 < n && cps[i + 2] == '{' && (cps[i + 3] == 'L' || cps[i + 3] == 'N') && cps[i + 4] == '}')
      return *type = (cps[i + 3] == 'L' ? I_LETTER : I_NUMBER) | (e == 'P' ? I_NEG : 0), 5;
    return 0;
  };
  // a literal
  {
    std::string lit;
    size_t i = 0;
    while (i < n) {
      uint32_t c = cps[i];
      if (c == '\\') {
        c = char_escape(i);
        if (c == kRaw) break;
        i += 2;
      } else if (is_meta(c)) {
        break;
      } else {
        i++;
      }
      uint8_t b[4];
      lit.append((const char*)b, lowercase::put(b, c));
    }
    if (i == n) {
      if (out) {
        out->mode = M_LITERAL;
        out->lit = lit;
      }
      return PC_LITERAL;
    }
  }
  // one class atom
  HostStep st;
  size_t i = 0;
  uint32_t type = 0;
  if (cps[0] == '\\') {
    const size_t l = class_escape(0, &type);
    if (!l) return PC_UNSUPPORTED;
    st.items = {type, 0, 0};
    i = l;
  } else if (cps[0] == '[') {
    i = 1;
    if (i < n && cps[i] == '^') {
      st.neg = 1;
      i++;
    }
    bool closed = false;
    while (i < n) {
      uint32_t c = cps[i];
      if (c == ']') {
        closed = true;
        i++;
        break;
      }
      if (c == '\\') {
        const size_t l = class_escape(i, &type);
        if (l) {
          st.items.insert(st.items.end(), {type, 0, 0});
          i += l;
          if (i < n && cps[i] == '-') return PC_UNSUPPORTED;
          continue;
        }
        c = char_escape(i);
        if (c == kRaw) return PC_UNSUPPORTED;
        i += 2;
      } else if (c < 0x80u && strchr("[^-&~", (int)c)) {
        return PC_UNSUPPORTED;
      } else {
        i++;
      }
      uint32_t hi = c;
      if (i + 1 < n && cps[i] == '-' && cps[i + 1] != ']') {
        hi = cps[i + 1];
        i += 2;
        if (hi == '\\') {
          hi = char_escape(i - 1);
          if (hi == kRaw) return PC_UNSUPPORTED;
          i++;
        } else if (hi < 0x80u && strchr("[^-&~", (int)hi)) {
          return PC_UNSUPPORTED;
        }
        if (hi < c) return PC_UNSUPPORTED;
      }
      st.items.insert(st.items.end(), {(uint32_t)I_RANGE, c, hi});
    }
    if (!closed || st.items.empty() || st.items.size() > 3 * 32) return PC_UNSUPPORTED;
  } else {
    return PC_UNSUPPORTED;
  }
  if (i < n && cps[i] == '+') {
    st.plus = 1;
    i++;
  }
  if (i != n) return PC_UNSUPPORTED;
  if (out) {
    out->mode = M_CLASS;
    out->plus = st.plus;
    out->neg = st.neg;
    out->items = st.items;
  }
  return PC_CLASS;
}

// Gate 4, for a step that carries kRegex: a pattern no earlier gate takes, compiled to a DFA
// (regex_dfa.h).  PC_DFA, or PC_UNSUPPORTED with *why naming the construct that is refused.
inline PatternClass plan_split(const std::string& p, HostStep* out, std::string* why) {
  const PatternClass c = classify_split(p, out);
  if (c != PC_UNSUPPORTED) return c;
  regex_dfa::Dfa d;
  *why = regex_dfa::compile(p, &d);
  if (!why->empty()) return PC_UNSUPPORTED;
  if (out) {
    out->mode = M_DFA;
    out->dfa = d;
  }
  return PC_DFA;
}

// The step's class items, literal and DFA tables as one block the rules read (4-byte aligned), and
// where the literal and the DFA's four arrays start in it.
struct StepBlob {
  std::string bytes;
  size_t lit = 0, trans = 0, ascii = 0, bounds = 0, symmap = 0;
};
inline StepBlob step_blob(const HostStep& h) {
  StepBlob b;
  auto pad = [&] {
    while (b.bytes.size() % 4) b.bytes.push_back('\0');
  };
  b.bytes.append((const char*)h.items.data(), h.items.size() * 4);
  b.lit = b.bytes.size();
  b.bytes += h.lit;
  if (h.mode == M_DFA) {
    pad();
    b.bounds = b.bytes.size();
    b.bytes.append((const char*)h.dfa.bounds.data(), h.dfa.bounds.size() * 4);
    b.trans = b.bytes.size();
    b.bytes.append((const char*)h.dfa.trans.data(), h.dfa.trans.size() * 2);
    b.ascii = b.bytes.size();
    b.bytes.append((const char*)h.dfa.ascii, 128);
    b.symmap = b.bytes.size();
    b.bytes.append((const char*)h.dfa.symmap.data(), h.dfa.symmap.size());
  }
  pad();
  return b;
}
// the Step the rules take, its pointers into the block at `base`; cap: the work bound of a cyclic DFA
inline Step step_view(const HostStep& h, const StepBlob& b, const uint8_t* base, uint32_t cap) {
  Step st{};
  st.kind = h.kind;
  st.flags = h.flags;
  st.cp = h.cp;
  st.mode = h.mode;
  st.plus = h.plus;
  st.neg = h.neg;
  st.n_items = (uint32_t)(h.items.size() / 3);
  st.items = (const uint32_t*)base;
  st.lit = base + b.lit;
  st.lit_len = (uint32_t)h.lit.size();
  st.cp_len = (uint32_t)h.cp_u8.size();
  memcpy(st.cp_u8, h.cp_u8.data(), h.cp_u8.size());
  if (h.mode == M_DFA) {
    st.dfa.trans = (const uint16_t*)(base + b.trans);
    st.dfa.ascii = base + b.ascii;
    st.dfa.bounds = (const uint32_t*)(base + b.bounds);
    st.dfa.symmap = base + b.symmap;
    st.dfa.n_bounds = (uint32_t)h.dfa.bounds.size();
    st.dfa.n_symbols = h.dfa.n_symbols;
    st.dfa.n_states = h.dfa.n_states;
    st.dfa.raw_sym = h.dfa.raw_sym;
    st.dfa.use = h.dfa.use;
    st.dfa.start = h.dfa.start;
    st.dfa.cap = h.dfa.cyclic ? cap : 0xFFFFFFFFu;
  }
  return st;
}

// One step of the ABI as a HostStep (a split's pattern already classified by the caller's gate 1:
// rejected = the Rust crate refuses it, the step is the identity).  An error text, or "";
// *unsupported is set when the text names a pattern no gate takes.
inline std::string make_step(uint32_t kind, uint32_t flags, const std::string& a, uint32_t cp, bool rejected, HostStep* out,
                             bool* unsupported) {
  *unsupported = false;
  if (kind > K_SPLIT) return "unknown kind";
  out->kind = kind;
  out->flags = flags;
  out->cp = cp;
  if (kind == K_METASPACE || kind == K_CHAR_DELIM) {
    if (cp > 0x10FFFFu || (cp >= 0xD800u && cp < 0xE000u)) return "cp is no Unicode scalar value";
    uint8_t b[4];
    out->cp_u8.assign((const char*)b, lowercase::put(b, cp));
  }
  if (kind == K_SPLIT) {
    if ((flags & 7u) > B_CONTIGUOUS) return "unknown behavior";
    if (a.size() >= (1ull << 32)) return "the pattern reaches 4 GiB";
    if (rejected) {
      out->mode = M_IDENTITY;
    } else if (!(flags & kRegex)) {
      if (classify_split(a, out) == PC_UNSUPPORTED) {
        *unsupported = true;
        return "the pattern is neither a literal nor one class atom with an optional '+'";
      }
    } else {
      std::string why;
      if (plan_split(a, out, &why) == PC_UNSUPPORTED) {
        *unsupported = true;
        return "the regex engine refuses " + why;
      }
    }
  }
  return "";
}

// What becomes of the empty word (an empty text) under steps [from, ..): `split` passes it on, Metaspace
// with a prefix makes it the replacement (*at = that step), every other step maps it to nothing.
enum EmptyFate { E_NOTHING, E_EMPTY_WORD, E_METASPACE };
inline EmptyFate empty_fate(const std::vector<HostStep>& prog, size_t* at) {
  for (size_t i = 0; i < prog.size(); i++) {
    if (prog[i].kind == K_SPLIT) continue;
    if (prog[i].kind == K_METASPACE && (prog[i].flags & 1u)) {
      *at = i;
      return E_METASPACE;
    }
    return E_NOTHING;
  }
  return E_EMPTY_WORD;
}

}  // namespace pretok
