// The table compiler (csrc/table_compile.cpp) on the host, with no HIP header:
//   g++ -O2 -std=c++17 -Wall -pthread table_compile_check.cpp ../csrc/table_compile.cpp ../csrc/bpe_model.cpp
//   table_compile_check [ARM[=N]:]tokenizer.json ...     ARM: a TableOptions field
// Per argument it prints "== <index>", the scalar results, the element count and the 64-bit FNV-1a
// digest of every table (tests/test_table_compile_cpu.py compares them with
// tests/golden/table_digests.json) and "consistent" once the tables answer, read as
// pair_tables_hd.h documents them, for every merge of the model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>

#include "../csrc/json.hpp"
#include "../csrc/table_compile.h"

using namespace ctok_rt;

static int g_bad = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c) && g_bad++ < 20) {                         \
      printf("FAILED %s: ", #c), printf(__VA_ARGS__), printf("\n"); \
    }                                                   \
  } while (0)

template <class T>
static void digest(const char* name, const T* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n * sizeof(T); i++) h = (h ^ b[i]) * 0x100000001b3ull;
  printf("%s %zu %016llx\n", name, n, (unsigned long long)h);
}

static void print_tables(const CompiledTables& t) {
  printf("narrow %d compact %d proper %d window %d short_packed %d\n", t.narrow, t.compact, t.proper, t.window, t.short_packed);
  printf("merge_mask %u merge16_mask %u piece_mask %u hot_entries %zu\n", t.merge_mask, t.merge16_mask, t.piece_mask, t.hot_entries);
  digest("merge_tab", t.merge_tab.data(), t.merge_tab.size());
  digest("lds_image", t.lds_image.data(), t.lds_image.size());
  digest("merge16", t.merge16.data(), t.merge16.size());
  digest("lds16_image", t.lds16_image.data(), t.lds16_image.size());
  digest("pair0", t.pair0.data(), t.pair0.size());
  digest("piece_tab", t.piece_tab.data(), t.piece_tab.size());
  digest("rank_newid", t.rank_newid.data(), t.rank_newid.size());
  digest("eager_bits", t.eager_bits.data(), t.eager_bits.size());
  digest("wmeta", t.wmeta.data(), t.wmeta.size());
  digest("byte2id", t.byte2id, 256);
}

static bool bit(const uint32_t* w, uint32_t i) { return (w[i >> 5] >> (i & 31)) & 1; }

// a hot table: kHotBuckets buckets of two entries; is `key` (under `mask`) in bucket c1 or c2?
static bool in_hot(const uint64_t* hot, uint64_t key, uint64_t mask, uint32_t c1, uint32_t c2) {
  for (uint32_t c : {c1, c2})
    for (int k = 0; k < 2; k++)
      if (hot[2 * c + k] != kEmpty && (hot[2 * c + k] & mask) == key) return true;
  return false;
}

static void check_tables(const BpeModel& m, const CompiledTables& t) {
  const size_t n_valid = m.valid_new.size();
  auto value = [&](uint32_t r) -> uint64_t { return t.compact ? (r < n_valid ? m.valid_new[r] : kPanicVal) : r; };
  auto panics = [&](uint64_t v) { return t.compact ? v == kPanicVal : v >= n_valid; };
  std::set<uint32_t> byte_tok;
  for (int b = 0; b < 256; b++)
    if (m.byte2id[b] >= 0) byte_tok.insert((uint32_t)m.byte2id[b]);
  const uint64_t* hot = t.lds_image.data();
  const uint32_t* bloom = reinterpret_cast<const uint32_t*>(hot + kHotU64);
  const uint32_t* bloom_all = reinterpret_cast<const uint32_t*>(hot + kLdsImageBytes / 8);
  const uint64_t* hot16 = t.lds16_image.data();
  const uint32_t* bloom16 = reinterpret_cast<const uint32_t*>(hot16 + kHotU64);
  CHECK(t.lds_image.size() == kLdsImageBytes / 8 + kBloomWords / 2, "%zu", t.lds_image.size());
  CHECK(t.lds16_image.size() == (t.narrow ? kLdsImageBytes / 8 : 0), "%zu", t.lds16_image.size());
  for (const auto& g : m.merges) {
    const uint32_t a = g.left, b = g.right;
    const uint64_t key = ((uint64_t)a << kIdBits) | b, want = value(g.rank);
    uint32_t h = mhash(a, b) & t.merge_mask;
    while (t.merge_tab[h] != kEmpty && (t.merge_tab[h] & kKeyMask) != key) h = (h + 1) & t.merge_mask;
    CHECK(t.merge_tab[h] == ((want << 42) | key), "merge_tab rank %u", g.rank);
    if (t.narrow) {
      uint32_t s = hash16_h(a, b) & t.merge16_mask;
      while (t.merge16[s] != kEmpty && (uint32_t)t.merge16[s] != key16(a, b)) s = (s + 1) & t.merge16_mask;
      CHECK(t.merge16[s] == ((want << 32) | key16(a, b)), "merge16 rank %u", g.rank);
    }
    if (byte_tok.count(a) && byte_tok.count(b)) continue;  // byte pairs: pair0 only
    const uint32_t h1 = mhash(a, b), h2 = mhash2(h1);
    const uint32_t b1 = (h1 >> 12) & (kBloomBits - 1), b2 = (h2 >> 12) & (kBloomBits - 1);
    CHECK(in_hot(hot, key, kKeyMask, h1 & (kHotBuckets - 1), h2 & (kHotBuckets - 1)) || (bit(bloom, b1) && bit(bloom, b2)),
          "rank %u in neither the hot table nor its filter", g.rank);
    CHECK(bit(bloom_all, b1) && bit(bloom_all, b2), "rank %u not in the all-pairs filter", g.rank);
    if (t.narrow) {
      const uint32_t hh = hash16_h(a, b), gg = hash16_g(a, b);
      CHECK(in_hot(hot16, key16(a, b), 0xFFFFFFFFull, hh >> 20, gg >> 20) ||
                (bit(bloom16, hh & (kBloomBits - 1)) && bit(bloom16, gg >> 14)),
            "rank %u in neither the narrow hot table nor its filter", g.rank);
    }
  }
  for (uint32_t i = 0; i < kHotU64; i++) {
    CHECK(hot[i] == kEmpty || !panics(hot[i] >> 42), "hot slot %u panics", i);
    if (t.narrow) CHECK(hot16[i] == kEmpty || !panics(hot16[i] >> 32), "narrow hot slot %u panics", i);
  }
  // whole-piece table: {lo, hi, len, id} per slot, len == 0 empty; piece_mask + 2 slots
  const uint32_t* p = t.piece_tab.data();
  CHECK(t.piece_tab.size() == 4 * ((size_t)t.piece_mask + 2), "%zu", t.piece_tab.size());
  std::set<uint32_t> ids;
  for (uint32_t s = 0; s <= t.piece_mask; s++) {
    if (p[4 * s + 2] == 0) continue;
    uint32_t h = piece_hash(p[4 * s], p[4 * s + 1], p[4 * s + 2]) & t.piece_mask;
    while (h != s && p[4 * h + 2] != 0) h = (h + 1) & t.piece_mask;
    CHECK(h == s, "piece slot %u is not reachable from its hash", s);
    // the table's order is by id with an unstable sort: a digest is a witness only without ties
    CHECK(ids.insert(p[4 * s + 3]).second, "two whole-piece entries share id %u: the table's order is a tie", p[4 * s + 3]);
  }
  CHECK(p[4 * ((size_t)t.piece_mask + 1) + 2] == 0, "the slot past the table is not empty");
}

static void set_arm(TableOptions& o, const std::string& arm) {
  const size_t eq = arm.find('=');
  const std::string k = arm.substr(0, eq);
  const size_t n = eq == std::string::npos ? 0 : (size_t)atoi(arm.c_str() + eq + 1);
  if (k == "force_wide") o.force_wide = true;
  else if (k == "no_hot_table") o.no_hot_table = true;
  else if (k == "no_window") o.no_window = true;
  else if (k == "no_piece_table") o.no_piece_table = true;
  else if (k == "merge_slack") o.merge_slack = n;
  else if (k == "merge16_slack") o.merge16_slack = n;
  else if (k == "piece_slack") o.piece_slack = n;
  else fprintf(stderr, "unknown arm %s\n", arm.c_str()), exit(2);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    std::string path = argv[i];
    TableOptions opt;
    const size_t colon = path.find(':');
    if (colon != std::string::npos && path.find('/') > colon) {
      set_arm(opt, path.substr(0, colon));
      path.erase(0, colon + 1);
    }
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    printf("== %d\n", i - 1);
    try {
      const ctj::Value root = ctj::parse(text.data(), text.size());
      const ctj::Value* model = root.get("model");
      if (!model) throw CtokError{CTOK_E_PARSE, "missing field `model`"};
      std::unordered_map<std::string, uint32_t> vocab;
      std::unordered_map<uint32_t, std::string> id_to_token;
      LoadTimer timer;
      const BpeModel m = parse_model(*model, vocab, id_to_token, timer);
      CompiledTables t;
      compile_tables(m, opt, t, timer);
      print_tables(t);
      check_tables(m, t);
      if (!g_bad) printf("consistent\n");
    } catch (const CtokError& e) {
      printf("error %d %s\n", e.code, e.msg.c_str());
      g_bad++;
    } catch (const ctj::ParseError& e) {
      printf("error json %s\n", e.what());
      g_bad++;
    }
  }
  return g_bad ? 1 : 0;
}
