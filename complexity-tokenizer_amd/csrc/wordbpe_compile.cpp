// The table compiler of the id-keyed word BPE: see wordbpe_compile.h.  Host-only.
#include "wordbpe_compile.h"

#include <algorithm>
#include <unordered_map>

namespace wordbpe {

namespace {

// the code point of a string that is exactly one well-formed char, kNoId otherwise
uint32_t one_char(const std::string& s) {
  uint32_t cp = 0;
  const uint32_t l = dec_char((const uint8_t*)s.data(), 0, s.size(), &cp);
  return l && l == s.size() ? cp : kNoId;
}

bool valid_utf8(const std::string& s) {
  for (size_t i = 0; i < s.size();) {
    uint32_t cp = 0;
    const uint32_t l = dec_char((const uint8_t*)s.data(), i, s.size(), &cp);
    if (!l) return false;
    i += l;
  }
  return true;
}

}  // namespace

int compile(const std::vector<std::pair<std::string, uint32_t>>& vocab, const std::vector<std::pair<std::string, std::string>>& merges,
            const std::vector<AddedToken>& added, Compiled* out, std::string* err) {
  auto fail = [&](int code, const std::string& msg) {
    if (err) *err = msg;
    return code;
  };
  if (merges.size() > kMaxMerges)
    return fail(kErrUnsupported, "a model of " + std::to_string(merges.size()) + " merges: at most " + std::to_string(kMaxMerges) +
                                     " are supported");
  Compiled& c = *out;
  c = Compiled();

  std::unordered_map<std::string, uint32_t> ids;
  ids.reserve(vocab.size() * 2);
  for (const auto& kv : vocab) {
    if (kv.second == kNoId) return fail(kErrUnsupported, "the vocab id 4294967295 is not supported (it marks an empty table slot)");
    ids[kv.first] = kv.second;
  }

  // the code-point table: the one-char vocab keys (a key that is not UTF-8 is no char's string)
  std::vector<CpSlot> chars;
  for (const auto& kv : ids) {
    const uint32_t cp = one_char(kv.first);
    if (cp != kNoId) chars.push_back(CpSlot{cp, kv.second});
  }
  uint64_t cap = 16;
  while (cap < 2 * (uint64_t)chars.size()) cap <<= 1;
  for (;; cap <<= 1) {
    if (cap > (1ull << 24)) return fail(kErrCapacity, "the code-point table cannot be built");
    c.cps.assign(cap, CpSlot{kNoId, 0});
    const uint32_t mask = (uint32_t)cap - 1;
    bool full = false;
    for (const CpSlot& e : chars) {
      uint32_t s = cp_slot(e.cp, mask), i = 0;
      for (; i < kCpProbe; i++) {
        if (c.cps[s].cp == kNoId) {
          c.cps[s] = e;
          break;
        }
        s = (s + 1) & mask;
      }
      if (i == kCpProbe) {
        full = true;
        break;
      }
    }
    if (!full) break;
  }

  // BpeTokenizer::new: a merge whose parts and concatenation are vocab keys enters merge_ranks with
  // its unfiltered rank (a later duplicate pair overwrites) and appends its result to the filtered list
  struct P {
    uint32_t a, b, rank;
  };
  std::vector<P> pairs;
  std::vector<uint32_t> filtered;
  {
    std::unordered_map<uint64_t, size_t> at;
    for (size_t r = 0; r < merges.size(); r++) {
      const auto ia = ids.find(merges[r].first);
      const auto ib = ids.find(merges[r].second);
      if (ia == ids.end() || ib == ids.end()) continue;
      const auto iab = ids.find(merges[r].first + merges[r].second);
      if (iab == ids.end()) continue;
      const auto it = at.emplace((uint64_t)ia->second << 32 | ib->second, pairs.size());
      if (it.second) pairs.push_back(P{ia->second, ib->second, (uint32_t)r});
      else pairs[it.first->second].rank = (uint32_t)r;
      filtered.push_back(iab->second);
    }
  }
  c.n_filtered = filtered.size();
  c.n_pairs = pairs.size();
  cap = 16;
  while (cap < 2 * (uint64_t)pairs.size()) cap <<= 1;
  for (;; cap <<= 1) {
    if (cap > (1ull << 28)) return fail(kErrCapacity, "the pair table cannot be built");
    c.pairs.assign(cap, strmerge::PairSlot{kNoRank, 0, 0, 0});
    const uint32_t mask = (uint32_t)cap - 1;
    bool full = false;
    for (const P& p : pairs) {
      uint32_t s = strmerge::pair_slot(p.a, p.b, mask), i = 0;
      for (; i < strmerge::kPairProbe; i++) {
        if (c.pairs[s].a == kNoRank) {
          // new_id of a pair is filtered[rank].new_id: another merge's result once an invalid merge
          // stands in front, and out of bounds (the panic mark) past the filtered list's end
          if (p.rank < filtered.size()) c.pairs[s] = strmerge::PairSlot{p.a, p.b, p.rank, filtered[p.rank]};
          else c.pairs[s] = strmerge::PairSlot{p.a, p.b, p.rank | kPanicBit, 0};
          break;
        }
        s = (s + 1) & mask;
      }
      if (i == strmerge::kPairProbe) {
        full = true;
        break;
      }
    }
    if (!full) break;
  }
  for (const P& p : pairs)
    if (p.rank >= filtered.size()) c.n_panic++;

  // the added tokens: the last entry of a content, ordered by first byte
  std::vector<AddedToken> toks;
  {
    std::unordered_map<std::string, size_t> at;
    for (const AddedToken& t : added) {
      if (t.content.empty())
        return fail(kErrUnsupported, "added token with empty content: the reference's word loop never terminates "
                                     "(src/huggingface/mod.rs:569-610)");
      if (!valid_utf8(t.content)) return fail(kErrArg, "an added token is not valid UTF-8");
      if (t.content.size() > kMaxAddedBytes)
        return fail(kErrUnsupported, "an added token of " + std::to_string(t.content.size()) + " bytes: at most " +
                                         std::to_string(kMaxAddedBytes) + " are supported");
      const auto it = at.emplace(t.content, toks.size());
      if (it.second) toks.push_back(t);
      else toks[it.first->second] = t;
    }
  }
  if (toks.size() > kMaxAdded)
    return fail(kErrUnsupported, std::to_string(toks.size()) + " added tokens: at most " + std::to_string(kMaxAdded) + " are supported");
  std::stable_sort(toks.begin(), toks.end(),
                   [](const AddedToken& x, const AddedToken& y) { return (uint8_t)x.content[0] < (uint8_t)y.content[0]; });
  c.a_group.assign(257, 0);
  for (const AddedToken& t : toks) {
    const uint8_t b = (uint8_t)t.content[0];
    c.a_group[b + 1]++;
    c.first_byte[b >> 5] |= 1u << (b & 31);
    c.a_bytes.insert(c.a_bytes.end(), t.content.begin(), t.content.end());
    c.a_off.push_back((uint32_t)c.a_bytes.size());
    c.a_id.push_back(t.id);
    c.a_flags.push_back(t.flags & (kSingleWord | kLstrip | kRstrip));
  }
  for (uint32_t b = 0; b < 256; b++) c.a_group[b + 1] += c.a_group[b];
  for (uint32_t b = 0; b < 256; b++)
    c.max_group_bytes = std::max(c.max_group_bytes, c.a_off[c.a_group[b + 1]] - c.a_off[c.a_group[b]]);
  if (c.max_group_bytes > kMaxGroupBytes)
    return fail(kErrUnsupported, "added tokens that share a first byte hold " + std::to_string(c.max_group_bytes) +
                                     " bytes: at most " + std::to_string(kMaxGroupBytes) + " are supported");
  return kOk;
}

}  // namespace wordbpe
