// regex_dfa.h: pattern -> AST -> priority-ordered Thompson NFA -> DFA over code-point classes.
//
// Matching is the Rust crate's: leftmost-first.  The NFA's splits are ordered (greedy: the body
// first, lazy: the exit first; an alternation: its branches left to right), a DFA state is the list
// of NFA threads in priority order, and a list ends at its first match instruction: whatever stands
// behind it has lower priority than a match already found and can never win.  Running the DFA from
// a start, the last accepting state seen gives the match's end (pretok_hd.h dfa_len), so `a|ab` and
// `ab|a`, `a+` and `a+?` differ as they do in the crate.
#include "regex_dfa.h"

#include <algorithm>
#include <cstring>
#include <map>

#include "gen/pretok_data.h"
#include "gen/unicode_data.h"
#include "pretok_hd.h"

namespace regex_dfa {
namespace {

using pretok::I_DIGIT;
using pretok::I_LETTER;
using pretok::I_NUMBER;
using pretok::I_RANGE;
using pretok::I_SPACE;
using pretok::kRaw;

constexpr uint32_t kInf = 0xFFFFFFFFu;

struct Refuse {
  std::string why;
};

struct Prim {
  uint32_t type, lo, hi;
  bool operator==(const Prim& o) const { return type == o.type && lo == o.lo && hi == o.hi; }
};
struct SetItem {
  uint32_t prim;
  bool neg;
};
struct Set {
  std::vector<SetItem> items;
  bool neg = false;
};
enum NodeKind { N_SET, N_EMPTY, N_CAT, N_ALT, N_REP };
struct Node {
  NodeKind kind = N_EMPTY;
  uint32_t set = 0;            // N_SET
  std::vector<uint32_t> kids;  // N_CAT, N_ALT; N_REP: one
  uint32_t min = 0, max = 0;   // N_REP
  bool lazy = false;
};

std::string show_cp(uint32_t c) {
  uint8_t b[4];
  return std::string((const char*)b, lowercase::put(b, c));
}

struct Parser {
  std::vector<uint32_t> cps;
  size_t i = 0;
  std::vector<Prim> prims;
  std::vector<Set> sets;
  std::vector<Node> nodes;

  uint32_t prim(uint32_t type, uint32_t lo, uint32_t hi) {
    const Prim p{type, lo, hi};
    for (uint32_t k = 0; k < prims.size(); k++)
      if (prims[k] == p) return k;
    if (prims.size() >= kMaxPrims) throw Refuse{"more than " + std::to_string(kMaxPrims) + " distinct ranges and class escapes"};
    prims.push_back(p);
    return (uint32_t)prims.size() - 1;
  }
  uint32_t node(const Node& n) {
    nodes.push_back(n);
    return (uint32_t)nodes.size() - 1;
  }
  uint32_t set_node(const Set& s) {
    sets.push_back(s);
    Node n;
    n.kind = N_SET;
    n.set = (uint32_t)sets.size() - 1;
    return node(n);
  }
  bool more() const { return i < cps.size(); }

  // at cps[at] == '\\' (pretok_prog.h classify_split's two escape rules)
  uint32_t char_escape(size_t at) const {
    if (at + 1 >= cps.size()) return kRaw;
    const uint32_t e = cps[at + 1];
    if (e == 'n') return '\n';
    if (e == 't') return '\t';
    if (e == 'r') return '\r';
    if (e == '<' || e == '>') return kRaw;
    if (e < 0x80u && ((e >= 0x21u && e <= 0x2Fu) || (e >= 0x3Au && e <= 0x40u) || (e >= 0x5Bu && e <= 0x60u) || (e >= 0x7Bu && e <= 0x7Eu)))
      return e;
    return kRaw;
  }
  size_t class_escape(size_t at, SetItem* it) {
    if (at + 1 >= cps.size()) return 0;
    const uint32_t e = cps[at + 1];
    if (e == 's' || e == 'S') return *it = SetItem{prim(I_SPACE, 0, 0), e == 'S'}, 2;
    if (e == 'd' || e == 'D') return *it = SetItem{prim(I_DIGIT, 0, 0), e == 'D'}, 2;
    if ((e == 'p' || e == 'P') && at + 4 < cps.size() && cps[at + 2] == '{' && (cps[at + 3] == 'L' || cps[at + 3] == 'N') && cps[at + 4] == '}')
      return *it = SetItem{prim(cps[at + 3] == 'L' ? I_LETTER : I_NUMBER, 0, 0), e == 'P'}, 5;
    return 0;
  }
  [[noreturn]] void refuse_escape(size_t at) const {
    const uint32_t e = at + 1 < cps.size() ? cps[at + 1] : 0;
    if (e == 'A' || e == 'z') throw Refuse{std::string("the anchor \\") + (char)e};
    if (e == 'b' || e == 'B' || e == '<' || e == '>') throw Refuse{std::string("the word boundary \\") + (char)e};
    if (e == 'w' || e == 'W') throw Refuse{std::string("the class \\") + (char)e};
    if (e == 'p' || e == 'P') throw Refuse{std::string("a \\") + (char)e + " class other than {L} and {N}"};
    throw Refuse{"the escape \\" + show_cp(e)};
  }

  uint32_t parse_class() {  // at '['
    Set s;
    i++;
    if (more() && cps[i] == '^') {
      s.neg = true;
      i++;
    }
    bool closed = false;
    while (more()) {
      uint32_t c = cps[i];
      if (c == ']') {
        closed = true;
        i++;
        break;
      }
      if (c == '\\') {
        SetItem it;
        const size_t l = class_escape(i, &it);
        if (l) {
          s.items.push_back(it);
          i += l;
          if (more() && cps[i] == '-') throw Refuse{"a range from a class escape"};
          continue;
        }
        c = char_escape(i);
        if (c == kRaw) refuse_escape(i);
        i += 2;
      } else if (c == '[') {
        throw Refuse{"a nested or POSIX class"};
      } else if (c == '&' || c == '~') {
        throw Refuse{"a class set operation"};
      } else if (c == '^' || c == '-') {
        throw Refuse{std::string("an unescaped '") + (char)c + "' inside a class"};
      } else {
        i++;
      }
      uint32_t hi = c;
      if (i + 1 < cps.size() && cps[i] == '-' && cps[i + 1] != ']') {
        hi = cps[i + 1];
        i += 2;
        if (hi == '\\') {
          hi = char_escape(i - 1);
          if (hi == kRaw) refuse_escape(i - 1);
          i++;
        } else if (hi < 0x80u && strchr("[^-&~", (int)hi)) {
          throw Refuse{"a class range that ends at an unescaped '" + show_cp(hi) + "'"};
        }
        if (hi < c) throw Refuse{"a class range that runs backwards"};
      }
      s.items.push_back(SetItem{prim(I_RANGE, c, hi), false});
    }
    if (!closed) throw Refuse{"an unclosed class"};
    if (s.items.empty()) throw Refuse{"an empty class"};
    return set_node(s);
  }

  uint32_t parse_atom() {
    const uint32_t c = cps[i];
    if (c == '(') {
      i++;
      if (more() && cps[i] == '?') {
        if (i + 1 < cps.size() && cps[i + 1] == ':') i += 2;
        else throw Refuse{"a flag or named group (?...)"};
      }
      const uint32_t n = parse_alt();
      if (!more() || cps[i] != ')') throw Refuse{"an unclosed group"};
      i++;
      return n;
    }
    if (c == '[') return parse_class();
    if (c == '.') {
      i++;
      Set s;
      s.neg = true;
      s.items.push_back(SetItem{prim(I_RANGE, '\n', '\n'), false});
      return set_node(s);
    }
    if (c == '^' || c == '$') throw Refuse{std::string("the anchor ") + (char)c};
    if (c == '*' || c == '+' || c == '?' || c == '{') throw Refuse{std::string("a repetition '") + (char)c + "' of nothing"};
    if (c == ']' || c == '}') throw Refuse{std::string("an unescaped '") + (char)c + "'"};
    Set s;
    if (c == '\\') {
      SetItem it;
      const size_t l = class_escape(i, &it);
      if (l) {
        i += l;
        s.items.push_back(it);
        return set_node(s);
      }
      const uint32_t e = char_escape(i);
      if (e == kRaw) refuse_escape(i);
      i += 2;
      s.items.push_back(SetItem{prim(I_RANGE, e, e), false});
      return set_node(s);
    }
    i++;
    s.items.push_back(SetItem{prim(I_RANGE, c, c), false});
    return set_node(s);
  }

  bool parse_count(uint32_t* out) {
    uint64_t v = 0;
    const size_t from = i;
    while (more() && cps[i] >= '0' && cps[i] <= '9') {
      v = v * 10 + (cps[i] - '0');
      if (v > kMaxNfa) throw Refuse{"a repetition count over " + std::to_string(kMaxNfa)};
      i++;
    }
    *out = (uint32_t)v;
    return i > from;
  }

  uint32_t parse_repeat() {
    uint32_t n = parse_atom();
    while (more()) {
      const uint32_t c = cps[i];
      Node r;
      r.kind = N_REP;
      if (c == '?') r.min = 0, r.max = 1, i++;
      else if (c == '*') r.min = 0, r.max = kInf, i++;
      else if (c == '+') r.min = 1, r.max = kInf, i++;
      else if (c == '{') {
        i++;
        if (!parse_count(&r.min)) throw Refuse{"a malformed counted repetition"};
        r.max = r.min;
        if (more() && cps[i] == ',') {
          i++;
          if (!parse_count(&r.max)) r.max = kInf;
        }
        if (!more() || cps[i] != '}') throw Refuse{"a malformed counted repetition"};
        i++;
        if (r.max < r.min) throw Refuse{"a counted repetition that runs backwards"};
      } else {
        break;
      }
      if (more() && cps[i] == '?') {
        r.lazy = true;
        i++;
      }
      r.kids = {n};
      n = node(r);
    }
    return n;
  }

  uint32_t parse_cat() {
    Node cat;
    cat.kind = N_CAT;
    while (more() && cps[i] != '|' && cps[i] != ')') cat.kids.push_back(parse_repeat());
    if (cat.kids.empty()) return node(Node{});
    if (cat.kids.size() == 1) return cat.kids[0];
    return node(cat);
  }

  uint32_t parse_alt() {
    Node alt;
    alt.kind = N_ALT;
    alt.kids.push_back(parse_cat());
    while (more() && cps[i] == '|') {
      i++;
      alt.kids.push_back(parse_cat());
    }
    if (alt.kids.size() == 1) return alt.kids[0];
    return node(alt);
  }

  bool nullable(uint32_t n) const {
    const Node& x = nodes[n];
    switch (x.kind) {
      case N_SET: return false;
      case N_EMPTY: return true;
      case N_CAT:
        for (uint32_t k : x.kids)
          if (!nullable(k)) return false;
        return true;
      case N_ALT:
        for (uint32_t k : x.kids)
          if (nullable(k)) return true;
        return false;
      default: return x.min == 0 || nullable(x.kids[0]);
    }
  }
};

enum Op : uint32_t { OP_CHAR, OP_SPLIT, OP_MATCH };
struct Inst {
  Op op;
  uint32_t x, y;  // OP_CHAR: set, next; OP_SPLIT: preferred, other
};

struct Emitter {
  const Parser& P;
  std::vector<Inst> prog;
  uint64_t work = 0;

  uint32_t add(Op op, uint32_t x, uint32_t y) {
    if (prog.size() >= kMaxNfa) throw Refuse{"more than " + std::to_string(kMaxNfa) + " NFA states"};
    prog.push_back(Inst{op, x, y});
    return (uint32_t)prog.size() - 1;
  }
  // the entry of node n's fragment, which goes on to `next`
  uint32_t emit(uint32_t n, uint32_t next) {
    if (++work > (1u << 20)) throw Refuse{"more than " + std::to_string(kMaxNfa) + " NFA states"};
    const Node& x = P.nodes[n];
    switch (x.kind) {
      case N_SET: return add(OP_CHAR, x.set, next);
      case N_EMPTY: return next;
      case N_CAT:
        for (size_t k = x.kids.size(); k-- > 0;) next = emit(x.kids[k], next);
        return next;
      case N_ALT: {
        std::vector<uint32_t> e;
        for (uint32_t k : x.kids) e.push_back(emit(k, next));
        uint32_t cur = e.back();
        for (size_t k = e.size() - 1; k-- > 0;) cur = add(OP_SPLIT, e[k], cur);
        return cur;
      }
      default: break;
    }
    const uint32_t kid = x.kids[0];
    uint32_t cur = next, need = x.min;
    if (x.max == kInf) {
      // x{n,}: n - 1 copies and x+ (n = 0: x*)
      const uint32_t loop = add(OP_SPLIT, 0, 0);
      const uint32_t body = emit(kid, loop);
      prog[loop].x = x.lazy ? next : body;
      prog[loop].y = x.lazy ? body : next;
      if (need) {
        cur = body;
        need--;
      } else {
        cur = loop;
      }
    } else {
      // x{n,m}: n copies, then m - n nested options (x(x(x)?)?)? whose exits all go to `next`
      for (uint32_t k = x.min; k < x.max; k++) {
        const uint32_t body = emit(kid, cur);
        cur = x.lazy ? add(OP_SPLIT, next, body) : add(OP_SPLIT, body, next);
      }
    }
    for (uint32_t k = 0; k < need; k++) cur = emit(kid, cur);
    return cur;
  }
};

}  // namespace

std::string compile(const std::string& pattern, Dfa* out) {
  try {
    Parser P;
    for (uint64_t i = 0; i < pattern.size();) {
      uint32_t l;
      const uint32_t c = normalize::dec((const uint8_t*)pattern.data(), pattern.size(), i, &l);
      if (c == kRaw) throw Refuse{"a pattern that is not UTF-8"};
      P.cps.push_back(c);
      i += l;
    }
    const uint32_t root = P.parse_alt();
    if (P.more()) throw Refuse{"an unopened ')'"};
    if (P.nullable(root)) throw Refuse{"a pattern that can match the empty string"};

    Emitter E{P, {}, 0};
    const uint32_t match = E.add(OP_MATCH, 0, 0);
    const uint32_t entry = E.emit(root, match);
    const std::vector<Inst>& prog = E.prog;
    Dfa d;
    d.n_nfa = (uint32_t)prog.size();

    // ---- the alphabet: the scalars partitioned by the primitive sets -----------------------------------
    for (const Prim& p : P.prims) {
      if (p.type == I_SPACE || p.type == I_LETTER || p.type == I_NUMBER) d.use |= 1u;
      if (p.type == I_DIGIT) d.use |= 3u;
    }
    d.bounds.push_back(0);
    for (const Prim& p : P.prims)
      if (p.type == I_RANGE) {
        d.bounds.push_back(p.lo);
        if (p.hi < 0x10FFFFu) d.bounds.push_back(p.hi + 1);
      }
    std::sort(d.bounds.begin(), d.bounds.end());
    d.bounds.erase(std::unique(d.bounds.begin(), d.bounds.end()), d.bounds.end());
    while (d.bounds.back() > 0x10FFFFu) d.bounds.pop_back();
    const pretok::Tables T{ct_cls_stage1, ct_cls_stage2, pt_nd_lo, pt_nd_hi, PT_N_ND};
    auto sig_of = [&](uint32_t at, uint32_t key) {  // which primitives hold the scalars of interval `at` with `key`
      uint64_t sig = 0;
      for (size_t k = 0; k < P.prims.size(); k++) {
        const Prim& p = P.prims[k];
        bool m;
        switch (p.type) {
          case I_RANGE: m = p.lo <= d.bounds[at] && d.bounds[at] <= p.hi; break;
          case I_SPACE: m = (key >> 1) == 0; break;
          case I_LETTER: m = (key >> 1) == 1; break;
          case I_NUMBER: m = (key >> 1) == 2; break;
          default: m = (key & 1u) != 0; break;
        }
        if (m) sig |= 1ull << k;
      }
      return sig;
    };
    std::map<uint64_t, uint32_t> sym_of_sig;
    std::vector<uint64_t> sig_of_sym;
    d.symmap.assign(d.bounds.size() * 8, 0xFF);
    auto sym_at = [&](uint32_t at, uint32_t key) {
      uint8_t& s = d.symmap[at * 8 + key];
      if (s == 0xFF) {
        const uint64_t sig = sig_of(at, key);
        auto it = sym_of_sig.find(sig);
        if (it == sym_of_sig.end()) {
          if (sig_of_sym.size() >= kMaxSymbols) throw Refuse{"more than " + std::to_string(kMaxSymbols) + " symbols"};
          it = sym_of_sig.emplace(sig, (uint32_t)sig_of_sym.size()).first;
          sig_of_sym.push_back(sig);
        }
        s = (uint8_t)it->second;
      }
      return s;
    };
    if (d.use) {
      uint32_t at = 0;
      for (uint32_t c = 0; c < 0x110000u; c++) {
        if (c == 0xD800u) c = 0xE000u;
        while (at + 1 < d.bounds.size() && d.bounds[at + 1] <= c) at++;
        const uint32_t cl = pretok::cls(T, c);
        const uint32_t key = cl * 2 + ((d.use & 2u) && cl == 2 && pretok::is_nd(T, c) ? 1 : 0);
        const uint8_t s = sym_at(at, key);
        if (c < 0x80u) d.ascii[c] = s;
      }
    } else {
      for (uint32_t at = 0; at < d.bounds.size(); at++) (void)sym_at(at, 0);
      for (uint32_t c = 0, at = 0; c < 0x80u; c++) {
        while (at + 1 < d.bounds.size() && d.bounds[at + 1] <= c) at++;
        d.ascii[c] = d.symmap[at * 8];
      }
    }
    for (uint8_t& s : d.symmap)
      if (s == 0xFF) s = 0;  // (no scalar has this interval and key)
    // the ill-formed byte: no primitive holds it (class_match's convention), and it is its own symbol
    if (sig_of_sym.size() >= kMaxSymbols) throw Refuse{"more than " + std::to_string(kMaxSymbols) + " symbols"};
    d.raw_sym = (uint32_t)sig_of_sym.size();
    sig_of_sym.push_back(0);
    d.n_symbols = (uint32_t)sig_of_sym.size();
    // every set as a mask over the symbols
    std::vector<uint64_t> set_mask(P.sets.size(), 0);
    for (size_t k = 0; k < P.sets.size(); k++)
      for (uint32_t s = 0; s < d.n_symbols; s++) {
        bool any = false;
        for (const SetItem& it : P.sets[k].items) any = any || (((sig_of_sym[s] >> it.prim) & 1u) != 0) != it.neg;
        if (any != P.sets[k].neg) set_mask[k] |= 1ull << s;
      }

    // ---- determinisation --------------------------------------------------------------------------------
    std::vector<uint32_t> seen(prog.size(), 0), stack;
    uint32_t stamp = 0;
    // the threads reached from pc without consuming, in priority order, appended to list
    auto follow = [&](uint32_t pc, std::vector<uint32_t>& list) {
      stack.push_back(pc);
      while (!stack.empty()) {
        const uint32_t q = stack.back();
        stack.pop_back();
        if (seen[q] == stamp) continue;
        seen[q] = stamp;
        if (prog[q].op == OP_SPLIT) {
          stack.push_back(prog[q].y);
          stack.push_back(prog[q].x);
        } else {
          list.push_back(q);
        }
      }
    };
    auto cut = [&](std::vector<uint32_t>& list) {
      for (size_t k = 0; k < list.size(); k++)
        if (prog[list[k]].op == OP_MATCH) {
          list.resize(k + 1);
          return true;
        }
      return false;
    };
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> states;
    std::vector<uint8_t> accepts;
    uint64_t threads = 0;
    auto state_of = [&](std::vector<uint32_t>& list) -> uint16_t {
      const bool acc = cut(list);
      if (list.empty()) return kDead;
      auto it = ids.find(list);
      if (it == ids.end()) {
        if (states.size() >= kMaxStates) throw Refuse{"more than " + std::to_string(kMaxStates) + " DFA states"};
        threads += list.size();
        if (threads > kMaxThreads) throw Refuse{"a DFA of more than " + std::to_string(kMaxThreads) + " NFA threads"};
        it = ids.emplace(list, (uint32_t)states.size()).first;
        states.push_back(list);
        accepts.push_back(acc ? 1 : 0);
      }
      return (uint16_t)(it->second | (acc ? kAccept : 0));
    };
    std::vector<uint32_t> list;
    stamp++;
    follow(entry, list);
    d.start = state_of(list) & kStateMask;
    for (size_t s = 0; s < states.size(); s++) {
      d.trans.resize((s + 1) * d.n_symbols, kDead);
      for (uint32_t a = 0; a < d.n_symbols; a++) {
        list.clear();
        stamp++;
        const std::vector<uint32_t> from = states[s];  // (a copy: state_of grows states)
        for (uint32_t pc : from)
          if (prog[pc].op == OP_CHAR && ((set_mask[prog[pc].x] >> a) & 1u)) follow(prog[pc].y, list);
        d.trans[s * d.n_symbols + a] = state_of(list);
      }
    }
    d.n_states = (uint32_t)states.size();

    // ---- a cycle, or the longest path (every live state reaches a match, so every path counts) ---------
    std::vector<uint8_t> colour(d.n_states, 0);
    std::vector<uint64_t> depth(d.n_states, 0);  // the longest path from the state, in transitions
    std::vector<std::pair<uint32_t, uint32_t>> dfs{{d.start, 0}};
    colour[d.start] = 1;
    while (!dfs.empty() && !d.cyclic) {
      auto& top = dfs.back();
      const uint32_t s = top.first;
      if (top.second == d.n_symbols) {
        colour[s] = 2;
        dfs.pop_back();
        if (!dfs.empty()) depth[dfs.back().first] = std::max(depth[dfs.back().first], depth[s] + 1);
        continue;
      }
      const uint16_t e = d.trans[s * d.n_symbols + top.second++];
      if (e == kDead) continue;
      const uint32_t to = e & kStateMask;
      if (colour[to] == 1) d.cyclic = true;
      else if (colour[to] == 2) depth[s] = std::max(depth[s], depth[to] + 1);
      else {
        colour[to] = 1;
        dfs.push_back({to, 0});
      }
    }
    d.longest = d.cyclic ? 0 : depth[d.start];
    *out = d;
    return "";
  } catch (const Refuse& r) {
    return r.why;
  }
}

}  // namespace regex_dfa
