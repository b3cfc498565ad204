// The table compiler: a BpeModel (bpe_model.cpp) into the device tables every kernel trusts
// (CompiledTables), one function per phase, in the order compile_tables calls them -- later
// phases read earlier tables.  The format is pair_tables_hd.h's.  Host-only and HIP-free;
// checked on a CPU by tools/table_compile_check.cpp (tests/test_table_compile_cpu.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>

#include "table_compile.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {
namespace {

using Merge = BpeModel::Merge;

// Can the merge apply?  One whose rank lies past the valid merges panics when looked up (src/bpe.rs:141).
bool applies(const BpeModel& m, const Merge& g) { return g.rank < m.valid_new.size(); }

// The table value of the merge of rank r: the rank, or (compact) its new id -- both increasing in rank
uint64_t table_value(const BpeModel& m, const CompiledTables& t, uint32_t r) {
  if (!t.compact) return r;
  return r < m.valid_new.size() ? m.valid_new[r] : kPanicVal;
}
bool value_panics(const BpeModel& m, const CompiledTables& t, uint64_t v) {
  return t.compact ? v == kPanicVal : v >= m.valid_new.size();
}

size_t capacity(size_t entries, size_t slack) {
  size_t cap = 1024;
  while (cap < entries * slack + 16) cap <<= 1;
  return cap;
}

// open addressing: e into the first empty slot from its home slot
void insert(std::vector<uint64_t>& tab, uint32_t mask, uint32_t home, uint64_t e) {
  uint32_t h = home & mask;
  while (tab[h] != kEmpty) h = (h + 1) & mask;
  tab[h] = e;
}

// The merge table probed as the kernels probe it: the value of pair (a, b), kNoRank without a merge
uint32_t lookup(const CompiledTables& t, uint32_t a, uint32_t b) {
  const uint64_t key = ((uint64_t)a << kIdBits) | b;
  for (uint32_t h = mhash(a, b) & t.merge_mask;; h = (h + 1) & t.merge_mask) {
    const uint64_t e = t.merge_tab[h];
    if (e == kEmpty) return kNoRank;
    if ((e & kKeyMask) == key) return (uint32_t)(e >> 42);
  }
}

void set_bit(uint32_t* bits, uint32_t i) { bits[i >> 5] |= 1u << (i & 31); }

// What a pair is in the tables of one key width: its entry, its two candidate hot-table buckets
// and its two Bloom-filter bits (pair_tables_hd.h)
struct Placement {
  uint64_t entry;
  uint32_t bucket[2], bloom[2];
};
Placement place42(uint64_t val, uint32_t a, uint32_t b) {
  const uint32_t h1 = mhash(a, b), h2 = mhash2(h1);
  return {(val << 42) | ((uint64_t)a << kIdBits) | b,
          {h1 & (kHotBuckets - 1), h2 & (kHotBuckets - 1)},
          {(h1 >> 12) & (kBloomBits - 1), (h2 >> 12) & (kBloomBits - 1)}};
}
Placement place16(uint64_t val, uint32_t a, uint32_t b) {
  const uint32_t h = hash16_h(a, b), g = hash16_g(a, b);
  return {(val << 32) | key16(a, b), {h >> 20, g >> 20}, {h & (kBloomBits - 1), g >> 14}};
}

// ---- value kind
void choose_value_kind(const BpeModel& m, const TableOptions& opt, CompiledTables& t) {
  t.narrow = m.max_id < 0xFFFFu;
  // compact table: values are the new ids themselves when new id is strictly increasing in rank
  // over the merges that can apply
  t.compact = !opt.force_wide;
  const uint32_t* prev = nullptr;
  for (const Merge& g : m.merges) {
    if (!t.compact || !applies(m, g)) continue;
    if (prev && m.valid_new[g.rank] <= *prev) t.compact = false;
    prev = &m.valid_new[g.rank];
  }
}

// ---- global merge table, and the narrow one beside it
void build_merge_tables(const BpeModel& m, const TableOptions& opt, CompiledTables& t) {
  for (const Merge& g : m.merges)
    if (g.left > kMaxId || g.right > kMaxId) throw_err(CTOK_E_UNSUPPORTED, "token ids above 2^21-2 are not supported by the device merge table");
  for (uint32_t id : m.valid_new)
    if (id > kMaxId) throw_err(CTOK_E_UNSUPPORTED, "token ids above 2^21-2 are not supported by the device merge table");
  // load factor <= 1/8: a lookup the Bloom filter lets through is often a pair with no merge,
  // whose linear probe runs to an empty slot (C2 k_bpe_short 0.54 -> 0.48 ms against 1/2)
  const size_t cap = capacity(m.merges.size(), opt.merge_slack);
  t.merge_tab.assign(cap, kEmpty);
  t.merge_mask = (uint32_t)(cap - 1);
  if (t.narrow) {
    // load <= 1/64: a lookup that reaches this table (a hot-table miss passing the Bloom filter)
    // stops at its first slot almost always, and a wavefront waits for its slowest lane's
    // probe chain -- C2 k_bpe_short 0.414 ms at 1/8, 0.391 at 1/32, 0.385 at 1/128 (A/B on one
    // box, profiles/r02/v9_ab_merge16_load.txt); 32 MB for 50k merges
    const size_t cap16 = capacity(m.merges.size(), opt.merge16_slack);
    t.merge16.assign(cap16, kEmpty);
    t.merge16_mask = (uint32_t)(cap16 - 1);
  }
  // inserted in rank order: the low-rank (frequent) pairs sit in their home slots, so their
  // lookups end at the first probe (the same reason the whole-piece table is filled in id order)
  for (const Merge& g : m.merges) {
    const uint64_t val = table_value(m, t, g.rank);
    insert(t.merge_tab, t.merge_mask, mhash(g.left, g.right), place42(val, g.left, g.right).entry);
    if (t.narrow) insert(t.merge16, t.merge16_mask, hash16_h(g.left, g.right), place16(val, g.left, g.right).entry);
  }
}

// ---- LDS images
// One image (hot table | Bloom filter of the pairs not in it, the merge passes ask the filter only
// after a hot-table miss) in the key width of `place`; returns the hot table's entries.  The hot
// table is filled greedily in rank order (a pair whose two buckets are full stays global-only),
// the filter covers every other entry (including the ones whose lookup panics).  Byte-pair
// merges are left out of both: the merge passes look a pair up in LDS only after a merge, when
// one side is a merged (multi-byte) token; initial byte pairs use pair0.  filter_all (optional):
// a second filter, over every pair.
template <class Place>
size_t fill_image(const BpeModel& m, const TableOptions& opt, const CompiledTables& t, const std::vector<uint8_t>& is_byte_tok,
                  Place place, uint64_t* hot, uint32_t* filter_all) {
  std::fill(hot, hot + kHotU64, kEmpty);
  uint32_t* filter = reinterpret_cast<uint32_t*>(hot + kHotU64);
  size_t placed = 0;
  for (const Merge& g : m.merges) {
    if (is_byte_tok[g.left] && is_byte_tok[g.right]) continue;
    const Placement p = place(table_value(m, t, g.rank), g.left, g.right);
    if (filter_all)
      for (uint32_t i : p.bloom) set_bit(filter_all, i);
    uint64_t* slot = nullptr;
    if (!opt.no_hot_table && applies(m, g)) {  // never cache an entry that panics
      for (uint32_t c : p.bucket)
        for (int k = 0; k < 2 && !slot; k++)
          if (hot[2 * c + k] == kEmpty) slot = &hot[2 * c + k];
    }
    if (slot) {
      *slot = p.entry;
      placed++;
      continue;  // a hot pair is found in the hot table before the filter is asked
    }
    for (uint32_t i : p.bloom) set_bit(filter, i);
  }
  return placed;
}

void build_lds_images(const BpeModel& m, const TableOptions& opt, CompiledTables& t) {
  std::vector<uint8_t> is_byte_tok(kMaxId + 2, 0);
  for (int b = 0; b < 256; b++)
    if (t.byte2id[b] >= 0 && (uint32_t)t.byte2id[b] <= kMaxId) is_byte_tok[t.byte2id[b]] = 1;
  // the wide image, then, outside the image, the Bloom filter of all pairs for the kernels that
  // load the filter alone (k_bpe_wave without HOT)
  t.lds_image.assign(kLdsImageBytes / 8 + kBloomWords / 2, 0);
  uint64_t* hot = t.lds_image.data();
  t.hot_entries = fill_image(m, opt, t, is_byte_tok, place42, hot, reinterpret_cast<uint32_t*>(hot + kLdsImageBytes / 8));
  // narrow vocabularies: the same tables keyed by key16, for the register merge passes
  if (t.narrow) {
    t.lds16_image.assign(kLdsImageBytes / 8, 0);
    fill_image(m, opt, t, is_byte_tok, place16, t.lds16_image.data(), nullptr);
  }
}

// ---- rank monotonicity ("proper": every merge consuming z ranks after every merge producing z)
// and the eager bits
void find_eager_merges(const BpeModel& m, CompiledTables& t) {
  // per id (ids <= kMaxId, checked by build_merge_tables): the latest rank producing it, the earliest consuming it
  constexpr uint32_t kUnset = UINT32_MAX;
  std::vector<uint32_t> maxprod(kMaxId + 2, kUnset), mincons(kMaxId + 2, kUnset);
  for (const Merge& g : m.merges) {
    if (!applies(m, g)) continue;  // panics on lookup anyway
    const uint32_t r = g.rank, z = m.valid_new[r];
    if (maxprod[z] == kUnset || maxprod[z] < r) maxprod[z] = r;
    for (uint32_t c : {g.left, g.right})
      if (mincons[c] == kUnset || mincons[c] > r) mincons[c] = r;
  }
  t.proper = true;
  for (size_t z = 0; z < maxprod.size(); z++)
    if (maxprod[z] != kUnset && mincons[z] != kUnset && mincons[z] <= maxprod[z]) { t.proper = false; break; }
  // per merge (bit at its table value: the rank, or the new id in a compact table): "eager"
  // when a merge consuming its token ranks before it.  Only an eager merge can be followed at
  // once by a merge of lower rank, so the long-piece rounds apply every occurrence of a
  // non-eager merge together even when the table as a whole is not rank-monotone (tiktoken-
  // style lists), and the leftmost one alone for an eager merge (ctok_internal.h Tables::eager).
  t.eager_bits.assign(((t.compact ? kMaxId + 2 : m.valid_new.size()) + 31) / 32 + 1, 0u);
  if (t.proper) return;
  for (const Merge& g : m.merges) {
    if (!applies(m, g)) continue;
    const uint32_t z = m.valid_new[g.rank];
    if (mincons[z] != kUnset && mincons[z] < g.rank) set_bit(t.eager_bits.data(), (uint32_t)table_value(m, t, g.rank));
  }
}

// ---- window metadata
// Window rounds of the long-piece tiers (Tables::window, long.hip bpe_wave_seg): exact when
// every token instance spans exactly its string's length -- each byte's initial token is one
// char, and every merge that can apply makes the token its two sides spell (no rank shift from
// an invalid merge before it, src/bpe.rs:60-69); on a table that is not rank-monotone the
// kernels add a check for candidates whose merge is eager.
// Per id: the longest left side of a merge whose right side it is, and the longest right side
// of a merge whose left side it is (chars = bytes; 0xFFFF when longer).
void build_window_meta(const BpeModel& m, const TableOptions& opt, CompiledTables& t) {
  auto nchars = [&](uint32_t id, bool& ok) -> uint32_t {
    auto it = m.id_to_token->find(id);
    if (it == m.id_to_token->end()) { ok = false; return 0; }
    uint32_t c = 0;
    for (unsigned char ch : it->second) c += (ch & 0xC0) != 0x80;
    return c;
  };
  bool ok = !opt.no_window;
  for (int b = 0; b < 256 && ok; b++)
    if (t.byte2id[b] >= 0 && nchars((uint32_t)t.byte2id[b], ok) != 1) ok = false;
  std::vector<uint32_t> ml, mr;
  if (ok) {
    ml.assign((size_t)m.max_id + 1, 0);
    mr.assign((size_t)m.max_id + 1, 0);
  }
  for (const Merge& g : m.merges) {
    if (!ok) break;
    if (!applies(m, g)) continue;  // panics when looked up: never merges
    const uint32_t a = g.left, b = g.right;
    const uint32_t la = nchars(a, ok), lb = nchars(b, ok), lz = nchars(m.valid_new[g.rank], ok);
    if (!ok || lz != la + lb || a > m.max_id || b > m.max_id) { ok = false; break; }
    ml[b] = std::max(ml[b], la);
    mr[a] = std::max(mr[a], lb);
  }
  t.window = ok;
  if (!ok) return;
  t.wmeta.resize((size_t)m.max_id + 1);
  for (size_t i = 0; i <= m.max_id; i++) t.wmeta[i] = std::min(ml[i], 0xFFFFu) | std::min(mr[i], 0xFFFFu) << 16;
}

// ---- byte-pair table: the merge-table value of (byte2id[a], byte2id[b]) for every byte pair a, b
// (the initial pairs of every piece are byte pairs), kNoRank where the pair has no merge
void build_pair0(CompiledTables& t) {
  t.pair0.assign(65536, kNoRank);
  for (uint32_t a = 0; a < 256; a++)
    for (uint32_t b = 0; b < 256; b++)
      if (t.byte2id[a] >= 0 && t.byte2id[b] >= 0) t.pair0[a * 256 + b] = lookup(t, (uint32_t)t.byte2id[a], (uint32_t)t.byte2id[b]);
}

// ---- the packed tier's decision
// The packed 16-slot tier of k_bpe_short (merge_packed_hd.h) keeps table values as u16 with 0xFFFF
// for "none": every value it can see -- the byte-pair table, the narrow global table, the narrow
// hot table -- must be below 0xFFFF, and none may be one whose lookup panics (the tier does not
// check for those).  Compact tables (value = new id) of a narrow vocabulary without panicking
// entries qualify; the tier is built for compact tables only.
bool fits_short_packed(const CompiledTables& t) {
  if (!t.narrow || !t.compact) return false;
  auto fits = [&](uint32_t v) { return v < 0xFFFFu; };  // (kPanicVal is above it)
  bool ok = true;
  for (uint32_t v : t.pair0) ok = ok && (v == kNoRank || fits(v));
  for (uint64_t e : t.merge16) ok = ok && (e == kEmpty || fits((uint32_t)(e >> 32)));
  for (uint32_t i = 0; i < kHotU64; i++) {
    const uint64_t e = t.lds16_image[i];
    ok = ok && (e == kEmpty || fits((uint32_t)(e >> 32)));
  }
  return ok;
}

// ---- whole-piece table: every vocab entry of <= 8 raw bytes whose own BPE is that single token
using PieceEntry = std::pair<std::string, uint32_t>;  // raw bytes, id

std::vector<PieceEntry> whole_pieces(const BpeModel& m, const CompiledTables& t) {
  const std::vector<int> inv = byte_unmap();
  std::vector<std::pair<const std::string*, uint32_t>> items;
  items.reserve(m.vocab->size());
  for (const auto& kv : *m.vocab) items.push_back({&kv.first, kv.second});
  // the reference merge loop (src/bpe.rs:88-153) on each entry's bytes, vocab split over threads
  const unsigned nth = std::min(16u, usable_cpus_once());
  std::vector<std::vector<PieceEntry>> part(nth);
  auto work = [&](unsigned w) {
    std::vector<uint32_t> cps, tk;
    std::string raw;
    for (size_t i = w; i < items.size(); i += nth) {
      if (!decode_utf8(*items[i].first, cps) || cps.empty() || cps.size() > 8 || !unmap_bytes(inv, cps, raw)) continue;
      bool ok = true;
      tk.clear();
      for (unsigned char c : raw) {
        if (t.byte2id[c] < 0) { ok = false; break; }
        tk.push_back((uint32_t)t.byte2id[c]);
      }
      if (!ok) continue;
      for (;;) {
        size_t bi = 0;
        uint32_t best = kNoRank;
        for (size_t j = 0; j + 1 < tk.size(); j++) {
          const uint32_t v = lookup(t, tk[j], tk[j + 1]);
          if (v == kNoRank) continue;
          if (value_panics(m, t, v)) { ok = false; break; }  // would panic: leave to the kernels
          if (v < best) { best = v; bi = j; }
        }
        if (!ok || best == kNoRank) break;
        tk[bi] = t.compact ? best : m.valid_new[best];
        tk.erase(tk.begin() + bi + 1);
      }
      if (ok && tk.size() == 1 && tk[0] == items[i].second) part[w].push_back({raw, items[i].second});
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned w = 1; w < nth; w++) th.emplace_back(work, w);
    work(0);
    for (auto& x : th) x.join();
  }
  std::vector<PieceEntry> ents;
  for (auto& p : part)
    for (auto& e : p) ents.push_back(std::move(e));
  return ents;
}

void build_piece_table(std::vector<PieceEntry> ents, const TableOptions& opt, CompiledTables& t) {
  // id order (BPE ids grow with merge order, roughly inverse frequency): frequent pieces are
  // inserted first and sit in their home slots -- k_segment's probes mostly end at the first
  // slot (C2 k_segment 0.42 -> 0.32 ms against the hash-map order used before)
  std::sort(ents.begin(), ents.end(), [](const auto& x, const auto& y) { return x.second < y.second; });
  const size_t pcap = capacity(ents.size(), opt.piece_slack);  // load <= 1/8: misses end early (C2 k_segment -10%)
  t.piece_tab.assign((pcap + 1) * 4, 0);  // + one slot that stays empty (k_segment's no-probe lanes)
  t.piece_mask = (uint32_t)(pcap - 1);
  if (opt.no_piece_table) return;
  for (const auto& e : ents) {
    uint64_t v = 0;
    for (size_t i = 0; i < e.first.size(); i++) v |= (uint64_t)(uint8_t)e.first[i] << (8 * i);
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32), len = (uint32_t)e.first.size();
    uint32_t h = piece_hash(lo, hi, len) & t.piece_mask;
    while (t.piece_tab[4 * h + 2] != 0) h = (h + 1) & t.piece_mask;
    t.piece_tab[4 * h] = lo;
    t.piece_tab[4 * h + 1] = hi;
    t.piece_tab[4 * h + 2] = len;
    t.piece_tab[4 * h + 3] = e.second;
  }
}

}  // namespace

void compile_tables(const BpeModel& m, const TableOptions& opt, CompiledTables& t, LoadTimer& timer) {
  if (m.n_listed >= (size_t)kNoRank - 2) throw_err(CTOK_E_UNSUPPORTED, "more than 4M merges");
  t.rank_newid = m.valid_new;
  memcpy(t.byte2id, m.byte2id, sizeof(t.byte2id));
  choose_value_kind(m, opt, t);
  build_merge_tables(m, opt, t);
  timer.lap("merge_tab");
  build_lds_images(m, opt, t);
  timer.lap("lds_image");
  find_eager_merges(m, t);
  build_window_meta(m, opt, t);
  timer.lap("window");
  build_pair0(t);
  t.short_packed = fits_short_packed(t);
  if (timer.on) fprintf(stderr, "[ctok load] narrow %d compact %d short_packed %d\n", (int)t.narrow, (int)t.compact, (int)t.short_packed);
  timer.lap("proper+pair0");
  build_piece_table(whole_pieces(m, t), opt, t);
  timer.lap("piece_tab");
}

}  // namespace ctok_rt
