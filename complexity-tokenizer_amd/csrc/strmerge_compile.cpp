// The model compiler of the string-keyed merge engine: see strmerge_compile.h.  Host-only.
#include "strmerge_compile.h"

#include <unordered_map>

namespace strmerge {

std::string byte_char(uint32_t b) {
  auto keep = [](uint32_t x) { return (x >= 0x21 && x <= 0x7E) || (x >= 0xA1 && x <= 0xAC) || (x >= 0xAE && x <= 0xFF); };
  uint32_t c = b;
  if (!keep(b)) {
    c = 256;
    for (uint32_t x = 0; x < b; x++)
      if (!keep(x)) c++;
  }
  std::string s;
  if (c < 0x80) s += (char)c;
  else {
    s += (char)(0xC0 | (c >> 6));  // (c < 0x800)
    s += (char)(0x80 | (c & 63));
  }
  return s;
}

// bytes of the well-formed UTF-8 char at s[i], 0 if there is none
static uint32_t char_at(const std::string& s, size_t i) {
  const uint8_t* t = (const uint8_t*)s.data();
  const size_t n = s.size();
  const uint8_t b0 = t[i];
  if (b0 < 0x80) return 1;
  uint32_t len, cp;
  if (b0 >= 0xC2 && b0 < 0xE0) len = 2, cp = b0 & 0x1F;
  else if (b0 >= 0xE0 && b0 < 0xF0) len = 3, cp = b0 & 0x0F;
  else if (b0 >= 0xF0 && b0 < 0xF5) len = 4, cp = b0 & 0x07;
  else return 0;
  if (i + len > n) return 0;
  for (uint32_t j = 1; j < len; j++) {
    if ((t[i + j] & 0xC0) != 0x80) return 0;
    cp = (cp << 6) | (t[i + j] & 0x3F);
  }
  if (len == 3 && (cp < 0x800 || (cp >= 0xD800 && cp < 0xE000))) return 0;
  if (len == 4 && (cp < 0x10000 || cp > 0x10FFFF)) return 0;
  return len;
}

bool valid_utf8(const std::string& s) {
  for (size_t i = 0; i < s.size();) {
    const uint32_t l = char_at(s, i);
    if (!l) return false;
    i += l;
  }
  return true;
}

uint32_t one_char(const std::string& s) {
  if (s.empty()) return 0;
  const uint32_t l = char_at(s, 0);
  return l == s.size() ? l : 0;
}

int compile(Kind kind, const std::vector<std::pair<std::string, uint32_t>>& vocab,
            const std::vector<std::pair<std::string, std::string>>& merges, const std::string& suffix,
            const std::string& unk_token, Compiled* out, std::string* err) {
  auto fail = [&](int code, const std::string& msg) {
    if (err) *err = msg;
    return code;
  };
  if (merges.size() > kMaxMerges)
    return fail(kErrUnsupported, "a model of " + std::to_string(merges.size()) + " merges: at most " +
                                     std::to_string(kMaxMerges) + " are supported");
  if (vocab.size() + 3 * (uint64_t)merges.size() + 256 >= kMaxSymbols)
    return fail(kErrUnsupported, "a model of 2^31 or more distinct token strings is not supported");
  if (!valid_utf8(suffix) || !valid_utf8(unk_token)) return fail(kErrArg, "a string argument is not valid UTF-8");

  Compiled& c = *out;
  c = Compiled();
  std::unordered_map<std::string, uint32_t> sym;
  auto intern = [&](const std::string& s) {
    const auto it = sym.emplace(s, (uint32_t)c.sym_str.size());
    if (it.second) c.sym_str.push_back(s);
    return it.first->second;
  };
  std::unordered_map<std::string, uint32_t> ids;
  for (const auto& kv : vocab) {
    if (!valid_utf8(kv.first)) return fail(kErrArg, "a vocab string is not valid UTF-8");
    if (!ids.emplace(kv.first, kv.second).second) return fail(kErrArg, "a vocab string is given twice");
    intern(kv.first);
  }
  {
    const auto it = ids.find(unk_token);
    c.unk_id = it == ids.end() ? 0u : it->second;
  }
  if (kind == kByteLevel)
    for (uint32_t b = 0; b < 256; b++) c.byte2sym[b] = intern(byte_char(b));
  else
    for (uint32_t b = 0; b < 256; b++) c.byte2sym[b] = 0;

  // the pairs in rank order: a later duplicate overwrites the rank (HashMap::insert, :439, :630)
  struct P {
    uint32_t a, b, rank, sym;
  };
  std::vector<P> pairs;
  if (kind != kWordLevel) {
    std::unordered_map<uint64_t, size_t> at;
    for (size_t r = 0; r < merges.size(); r++) {
      if (!valid_utf8(merges[r].first) || !valid_utf8(merges[r].second)) return fail(kErrArg, "a merge string is not valid UTF-8");
      const uint32_t a = intern(merges[r].first), b = intern(merges[r].second);
      const uint32_t ab = intern(merges[r].first + merges[r].second);
      const auto it = at.emplace((uint64_t)a << 32 | b, pairs.size());
      if (it.second) pairs.push_back(P{a, b, (uint32_t)r, ab});
      else pairs[it.first->second].rank = (uint32_t)r;
    }
    c.n_merges = merges.size();
  }
  const uint32_t S = (uint32_t)c.sym_str.size();
  c.foreign = S;
  c.sym_id.assign((size_t)S + 1, c.unk_id);
  for (uint32_t s = 0; s < S; s++) {
    const auto it = ids.find(c.sym_str[s]);
    if (it != ids.end()) c.sym_id[s] = it->second;
  }

  // the pair table
  uint64_t cap = 16;
  while (cap < 2 * (uint64_t)pairs.size()) cap <<= 1;
  for (;; cap <<= 1) {
    if (cap > (1ull << 28)) return fail(kErrCapacity, "the pair table cannot be built");
    c.pairs.assign(cap, PairSlot{kNoRank, 0, 0, 0});
    const uint32_t mask = (uint32_t)cap - 1;
    bool full = false;
    for (const P& p : pairs) {
      uint32_t s = pair_slot(p.a, p.b, mask), i = 0;
      for (; i < kPairProbe; i++) {
        if (c.pairs[s].a == kNoRank) {
          c.pairs[s] = PairSlot{p.a, p.b, p.rank, p.sym};
          break;
        }
        s = (s + 1) & mask;
      }
      if (i == kPairProbe) {
        full = true;
        break;
      }
    }
    if (!full) break;
  }

  // the strings of the initial tokens (the patterns' bytes are copied by wptab::build)
  std::vector<wptab::Pattern> pats;
  if (kind == kWordLevel) {
    for (uint32_t s = 0; s < S; s++)
      if (!c.sym_str[s].empty())
        pats.push_back(wptab::Pattern{(const uint8_t*)c.sym_str[s].data(), (uint32_t)c.sym_str[s].size(), 0, s});
  } else if (kind == kCharBpe) {
    for (uint32_t s = 0; s < S; s++) {
      const std::string& t = c.sym_str[s];
      if (const uint32_t l = one_char(t)) pats.push_back(wptab::Pattern{(const uint8_t*)t.data(), l, 0, s});
      if (t.size() > suffix.size() && !t.compare(t.size() - suffix.size(), suffix.size(), suffix)) {
        const uint32_t l = one_char(t.substr(0, t.size() - suffix.size()));
        if (l) pats.push_back(wptab::Pattern{(const uint8_t*)t.data(), l, 1, s});
      }
    }
  }
  const int rc = wptab::build(pats, &c.strings);
  if (rc != wptab::kOk) return fail(kErrCapacity, "the model's string table cannot be built");
  return kOk;
}

}  // namespace strmerge
