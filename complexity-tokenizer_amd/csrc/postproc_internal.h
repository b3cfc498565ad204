// What the PostProcessor's host runtime (postproc_host.cpp) calls: the template compiler
// (postproc_compile.cpp, host-only, also tools/postproc_check.cpp's) and the launches of postproc.hip.
// Not part of the C ABI.  Every pointer of the launch functions is a device pointer.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "postproc_hd.h"

namespace postproc {

enum Kind : uint32_t { K_TEMPLATE, K_BERT, K_ROBERTA, K_N };  // ctok_postprocessor.h

struct HostStep {
  uint32_t kind = K_TEMPLATE;
  bool has_pair_template = false;
  std::string single, pair;                                 // UTF-8
  std::vector<std::pair<std::string, uint32_t>> specials;  // a template's, in the caller's order
  uint32_t id_a = 0, id_b = 0;                              // Bert: cls, sep; Roberta: bos, eos
};

struct HostItem {
  uint32_t kind;   // ItemKind
  uint32_t value;  // IT_SPECIAL: the id
};

struct HostList {
  std::vector<HostItem> items;
  std::vector<uint16_t> pa, pb, ps;  // items.size() + 1 each
  std::vector<uint32_t> val;         // items.size()
  List view() const { return List{pa.data(), pb.data(), ps.data(), val.data(), (uint32_t)items.size()}; }
};

struct Program {
  HostList single, pair;  // for rows without a pair, with a pair
};

enum CompileError : int { C_OK = 0, C_ARG = 1, C_CAPACITY = 2 };

// The items one step gives, the walk of postprocessors.rs:88-187: an unknown token gives nothing, a
// $B without a pair gives nothing.
std::vector<HostItem> step_items(const HostStep& st, bool has_pair);
// Both flat lists of a Sequence with their prefix tables.  Composition is substitution: a step after
// the first sees no pair and takes the list so far for its $A.  C_CAPACITY when a list would have
// more than kMaxItems items (err holds the count), C_ARG for a step that is none.
CompileError compile(const std::vector<HostStep>& steps, Program* out, std::string* err);
bool is_utf8(const std::string& s);

}  // namespace postproc

#if defined(__HIP_PLATFORM_AMD__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace ctok_pp {

constexpr uint32_t kThreads = 256;  // a workgroup, and the cells of its tile
constexpr uint32_t kMetaBad = 0, kMetaLongest = 1, kMetaN = 2;

struct DevProgram {
  postproc::List single, pair;
};

struct Matrix {
  uint32_t* ids;
  uint32_t* attention_mask;
  uint32_t* token_type_ids;
  uint32_t* special_tokens_mask;
  uint32_t* row_len;  // n_rows
  uint64_t width;
};

// rows[r] = row r's lengths after truncation, off[r] = its processed length (n_rows + 1 entries, for
// scan_u64); meta[kMetaBad] != 0 when the offsets are not in order, meta[kMetaLongest] = the longest row
hipError_t launch_count(const postproc::In& in, const postproc::Opts& o, const DevProgram& p, postproc::Row* rows, uint64_t* off,
                        uint64_t* meta, hipStream_t s);
// after the scan: out[off[r] + j] = cell j of row r; total = off[n_rows] < 2^32
hipError_t launch_write_ragged(const postproc::In& in, const DevProgram& p, const postproc::Row* rows, const uint64_t* off,
                               uint64_t total, uint32_t* out, hipStream_t s);
// after the scan: the n_rows * m.width < 2^32 cells of the four matrices, and row_len
hipError_t launch_write_matrix(const postproc::In& in, const postproc::Opts& o, const DevProgram& p, const postproc::Row* rows,
                               const uint64_t* off, const Matrix& m, hipStream_t s);

}  // namespace ctok_pp
#endif
