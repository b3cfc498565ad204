// The table compiler of the id-keyed word BPE (wordbpe_hd.h, wordbpe.hip): vocab, merges and added
// tokens, as the reference's loader holds them, into the code-point table, the pair table with the
// rank / new-id quirk of BpeTokenizer::new (src/bpe.rs:52-79) and the added-token pool.  Host-only:
// no HIP include; tools/wordbpe_check.cpp builds it with plain g++.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "wordbpe_hd.h"

namespace wordbpe {

constexpr int kOk = 0, kErrUnsupported = -3, kErrArg = -4, kErrCapacity = -5;  // CTOK_E_* of include/ctok.h

struct AddedToken {
  std::string content;
  uint32_t id;
  uint32_t flags;  // kSingleWord | kLstrip | kRstrip
};

struct Compiled {
  std::vector<CpSlot> cps;
  std::vector<strmerge::PairSlot> pairs;
  uint64_t n_filtered = 0;  // the length of the filtered merge list: what a marked pair's rank is out of
  uint64_t n_pairs = 0;
  uint64_t n_panic = 0;     // pairs that carry the panic mark
  // the added tokens, ordered by first byte (then as given)
  std::vector<uint8_t> a_bytes;
  std::vector<uint32_t> a_off{0}, a_id, a_flags, a_group;
  uint32_t first_byte[8] = {};  // the set of their first bytes
  uint32_t max_group_bytes = 0;  // the most bytes of the tokens that share a first byte

  CpView cp_view() const { return CpView{cps.data(), (uint32_t)cps.size() - 1}; }
  PairView pair_view() const { return PairView{pairs.data(), (uint32_t)pairs.size() - 1}; }
  // alnum_lo / alnum_hi are the caller's (csrc/gen/alnum_data.h)
  AddedView added_view(const uint32_t* alnum_lo, const uint32_t* alnum_hi, uint32_t n_alnum) const {
    return AddedView{a_bytes.data(), a_off.data(), a_id.data(), a_flags.data(), a_group.data(), alnum_lo, alnum_hi, n_alnum,
                     (uint32_t)a_id.size()};
  }
};

// vocab: (string, id) in the file's order, a string given twice keeps its last id (a JSON object read
// into a map).  merges: the (left, right) pairs that survived the split at ' ', in rank order.  added:
// in the file's order, a content given twice keeps its last entry (HashMap::insert, mod.rs:275-283).
int compile(const std::vector<std::pair<std::string, uint32_t>>& vocab, const std::vector<std::pair<std::string, std::string>>& merges,
            const std::vector<AddedToken>& added, Compiled* out, std::string* err);

}  // namespace wordbpe
