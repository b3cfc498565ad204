// The table compiler's interface: the BPE model the loader's parse phase hands over (BpeModel,
// bpe_model.cpp), the device tables compiled from it (CompiledTables, table_compile.cpp) and the
// load-time A/B arms (TableOptions).  Host-only and HIP-free: builds with plain g++, so the
// compiler is checked on a CPU (tools/table_compile_check.cpp).
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ctok.h"
#include "pair_tables_hd.h"

namespace ctj {
struct Value;
}

namespace ctok_rt __attribute__((visibility("hidden"))) {
using namespace ctok_dev;

struct CtokError {
  int code;
  std::string msg;
};

[[noreturn]] inline void throw_err(int code, const std::string& msg) { throw CtokError{code, msg}; }

// CTOK_LOAD_TIMING=1: per-phase load times on stderr, one "[ctok load] <phase> <ms> ms" line per lap
struct LoadTimer {
  bool on = false;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(const char* what);
};

// What BpeTokenizer::new (src/bpe.rs:52-79) keeps of model.vocab and model.merges.
struct BpeModel {
  struct Merge {
    uint32_t rank, left, right;  // rank: the merge's index in the file's list (a later duplicate pair wins)
  };
  std::vector<Merge> merges;        // sorted by rank
  size_t n_listed = 0;              // merges the file lists as two tokens: ranks run below it
  std::vector<uint32_t> valid_new;  // new id of the k-th merge whose three tokens exist: a rank
                                    // past its end panics when looked up (src/bpe.rs:141)
  const std::unordered_map<std::string, uint32_t>* vocab = nullptr;        // model.vocab
  const std::unordered_map<uint32_t, std::string>* id_to_token = nullptr;  // Vocab::id_to_token
  uint32_t max_id = 0;    // the vocabulary's largest id
  int32_t byte2id[256];   // vocab[bytes_to_unicode[b]] (src/bpe.rs:94-97), -1 = dropped
};

// Load-time A/B arms of the compiler (knobs.h fills them from the environment)
struct TableOptions {
  bool force_wide = false;
  bool no_hot_table = false;
  bool no_window = false;
  bool no_piece_table = false;
  size_t merge_slack = 8, merge16_slack = 64, piece_slack = 8;
};

struct CompiledTables {
  std::vector<uint64_t> merge_tab;
  uint32_t merge_mask = 0;
  std::vector<uint64_t> lds_image;  // kLdsImageBytes: hot table + Bloom filter; then the filter of all pairs
  std::vector<uint64_t> lds16_image, merge16;  // narrow vocabularies: the 32-bit-key tables (key16)
  uint32_t merge16_mask = 0;
  std::vector<uint32_t> pair0;      // 256 x 256 byte-pair merge values
  size_t hot_entries = 0;
  std::vector<uint32_t> piece_tab;  // 4 u32 per slot (see pair_tables_hd.h piece_hash)
  uint32_t piece_mask = 0;
  std::vector<uint32_t> rank_newid;
  std::vector<uint32_t> eager_bits;  // bit v: the merge of table value v is eager (see Tables::eager)
  std::vector<uint32_t> wmeta;       // window rounds (Tables::wmeta): per id, max left | max right << 16
  bool window = false;               // window rounds exact for this table (see Tables::window)
  int32_t byte2id[256];
  bool proper = true;
  bool compact = false;
  bool narrow = false;  // every vocab id < 2^16
  bool short_packed = false;  // narrow, and every narrow-table value fits the packed 16-slot tier (Tables::short_packed)
  // added tokens that can occur inside a piece, as raw-byte patterns (compile_added_patterns, ctok_load.cpp)
  std::string at_bytes;
  std::vector<uint32_t> at_off{0}, at_id;
  std::vector<uint8_t> at_flags;
  bool ids16 = false;   // every id encode can emit (vocab and added tokens) < 2^16: 16-bit ids on PCIe
};

// ---- bpe_model.cpp
unsigned usable_cpus_once();
std::vector<uint32_t> byte_map();  // GPT-2 bytes_to_unicode: byte -> code point
std::vector<int> byte_unmap();     // its inverse: mapped code point (< U+0144) -> byte, -1 for any other
// the raw bytes of a string of mapped code points; false when one of them is no byte's
bool unmap_bytes(const std::vector<int>& inv, const std::vector<uint32_t>& cps, std::string& raw);
std::string utf8(uint32_t cp);
bool decode_utf8(const std::string& s, std::vector<uint32_t>& out);
// model.vocab into vocab / id_to_token (which the model then points into), model.merges through
// BpeTokenizer::new; throws the loader's schema errors
BpeModel parse_model(const ctj::Value& model, std::unordered_map<std::string, uint32_t>& vocab,
                     std::unordered_map<uint32_t, std::string>& id_to_token, LoadTimer& timer);

// ---- table_compile.cpp
// Every table but the at_* patterns and ids16.  Throws CTOK_E_UNSUPPORTED for ids above 2^21-2
// and for more than 4M merges.
void compile_tables(const BpeModel& m, const TableOptions& opt, CompiledTables& t, LoadTimer& timer);

}  // namespace ctok_rt
