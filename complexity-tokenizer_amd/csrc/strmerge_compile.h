// The model compiler of the three stand-alone models behind include/ctok_models.h (WordLevelModel,
// CharBpeModel, ByteLevelBpeModel; reference src/models.rs:300-741): vocab and merges as strings in,
// the tables of the string-keyed merge engine (strmerge.hip) out.  Host-only: no HIP include, so
// tools/strmerge_check.cpp builds and checks it with a plain C++ compiler.
//
// Interning.  Every distinct string among the vocab keys, the merge parts a, b and the results
// a + b (and, for the byte-level model, the 256 chars of the GPT-2 byte map) is a symbol 0 .. S - 1.
// A token's identity is its string, however it was produced: a merge's parts and result need not
// be vocab entries.  Symbol S is the foreign symbol: an initial token whose string is not interned.
// It is in no pair, so it takes part in no merge (two adjacent foreign tokens never merge), and
// sym_id[S] = unk_id.
//
// Tables.
//   pairs     (symA, symB) -> (rank, sym(A + B)), strmerge_hd.h; a pair given twice keeps its last rank
//   sym_id    [S + 1] the vocab id of the symbol's string, or unk_id
//   byte2sym  [256] byte-level model: the symbol of the byte's map char
//   strings   char model: wp_table_hd.h patterns of the initial tokens -- form 0: a one-char string,
//             keyed by the char; form 1: a one-char string + suffix, keyed by the char (a word's last
//             char).  Word-level model: form 0, every non-empty vocab string (a match counts only
//             when it is as long as the word).
//
// Limits (compile refuses with CTOK_E_UNSUPPORTED): symbols below 2^31 and at most kMaxMerges merges.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "strmerge_hd.h"
#include "wp_table_hd.h"

namespace strmerge {

constexpr uint64_t kMaxMerges = 1ull << 24;
constexpr uint64_t kMaxSymbols = 1ull << 31;

enum Kind { kWordLevel = 0, kCharBpe = 1, kByteLevel = 2 };

// the error codes of include/ctok.h that compile returns (kept equal by models_host.cpp)
constexpr int kOk = 0, kErrUnsupported = -3, kErrArg = -4, kErrCapacity = -5;

struct Compiled {
  std::vector<std::string> sym_str;  // S
  std::vector<uint32_t> sym_id;      // S + 1
  std::vector<PairSlot> pairs;       // a power of two
  uint32_t byte2sym[256];
  wptab::Built strings;
  uint32_t unk_id = 0;
  uint32_t foreign = 0;  // S
  uint64_t n_merges = 0;
  PairView pair_view() const { return PairView{pairs.data(), (uint32_t)pairs.size() - 1}; }
};

// UTF-8 of the GPT-2 byte map's char for byte b (src/models.rs:369-390)
std::string byte_char(uint32_t b);
// bytes of s when it is exactly one well-formed UTF-8 char, else 0
uint32_t one_char(const std::string& s);
bool valid_utf8(const std::string& s);

// vocab: distinct strings with their ids; merges: (a, b) in rank order.  0, or an error code with
// *err set.
int compile(Kind kind, const std::vector<std::pair<std::string, uint32_t>>& vocab,
            const std::vector<std::pair<std::string, std::string>>& merges, const std::string& suffix,
            const std::string& unk_token, Compiled* out, std::string* err);

}  // namespace strmerge
