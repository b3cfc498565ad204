// A `split` pattern outside the literal and class-atom gates (pretok_prog.h classify_split) compiled
// to a DFA that the kernels of pretok.hip step (pretok_hd.h dfa_len): parser, priority-ordered
// Thompson NFA, determinisation into ordered thread lists cut after the match state (leftmost-first,
// as the Rust regex crate matches), over an alphabet of code-point classes.  Host-only and HIP-free;
// shared by the runtime (pretok_host.cpp) and the CPU checks (tools/regex_dfa_check.cpp,
// tools/pretok_check.cpp).  Not part of the C ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace regex_dfa {

// The caps: a pattern over any of them is refused.
constexpr uint32_t kMaxSymbols = 64;      // code-point classes, the ill-formed byte's included
constexpr uint32_t kMaxStates = 4096;     // DFA states, the dead state not counted
constexpr uint32_t kMaxNfa = 1u << 14;    // NFA instructions after counted repetitions are expanded
constexpr uint32_t kMaxPrims = 64;        // distinct primitive sets (ranges and class escapes) of a pattern
constexpr uint64_t kMaxThreads = 1u << 22;  // NFA threads over all DFA states: the determinisation's memory and time

// A transition entry: kDead, or the next state with kAccept set when that state holds a match.
constexpr uint16_t kDead = 0xFFFF, kAccept = 0x8000, kStateMask = 0x0FFF;

struct Dfa {
  uint32_t n_symbols = 0, n_states = 0, n_nfa = 0, start = 0;
  bool cyclic = false;    // a match can be unbounded
  uint64_t longest = 0;   // acyclic: the longest match in code points
  std::vector<uint16_t> trans;  // [state][symbol]
  // code point -> symbol: ASCII directly; otherwise symmap[interval * 8 + key], interval = the last
  // bounds[] entry <= c, key = cls * 2 + nd (cls: 0 \s, 1 \p{L}, 2 \p{N}, 3 other, read when use & 1;
  // nd: \d, read when use & 2 and cls == 2).  An ill-formed byte is raw_sym.
  uint8_t ascii[128] = {};
  std::vector<uint32_t> bounds;
  std::vector<uint8_t> symmap;
  uint32_t raw_sym = 0, use = 0;
};

// "" and *out, or why the pattern is refused (the construct named).  The pattern is one the Rust
// crate compiles (gate 1 is the caller's).
std::string compile(const std::string& pattern, Dfa* out);

}  // namespace regex_dfa
