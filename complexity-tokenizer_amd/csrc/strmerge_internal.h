// Internal interface between the host runtime of the stand-alone models (models_host.cpp) and the
// kernels of the string-keyed merge engine (strmerge.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "strmerge_hd.h"
#include "wp_table_hd.h"

namespace ctok_sm {

constexpr uint32_t kTier1 = 32;    // symbols of a word one thread merges in LDS columns
constexpr uint32_t kTier2 = 2048;  // symbols of a word one wavefront merges in LDS (4 u32 arrays: 32 KiB)
// The most symbols of one word.  The literal loop is quadratic in a word's length, so a longer word
// is refused before any merge kernel runs (DESIGN.md 4.6f has the measured basis).
constexpr uint32_t kMaxWordSymbols = 1u << 15;

enum { kCtrList2 = 0, kCtrList3 = 1, kCtrMaxSym = 2, kCtrState = 4 /* u64: positions reserved for list 3 */, kNumCtr = 8 };

struct Model {  // device pointers, owned by the host runtime
  uint32_t kind;  // strmerge::Kind
  strmerge::PairView pairs;
  const uint32_t* sym_id;    // [foreign + 1]
  const uint32_t* byte2sym;  // [256]
  wptab::View strings;
  uint32_t foreign;
  uint32_t prefix_space;  // byte-level: add_prefix_space
};

// One call's text and word list.  A run is the text between two set start bits; runs[r] is run r's
// first byte and runs[n_runs] = n_bytes.  For the char and word-level models a run is a word or a
// stretch of whitespace (ws_split_hd.h; whitespace has nsym 0), for the byte-level model a word.
struct Batch {
  const uint8_t* text;
  uint32_t n_bytes;
  uint32_t n_w;  // 32-byte words of the bitmaps
  const uint64_t* doc_off;
  uint64_t n_docs;
  uint32_t* bits;    // [n_w] start bits
  uint32_t* dbits;   // [n_w] byte-level: the start bits of non-empty texts
  uint32_t* wrank;   // [n_w + 1] set start bits before each bitmap word; [n_w] = n_runs
  uint32_t* crank;   // [n_w + 1] char model: code-point starts before each bitmap word
  uint32_t* runs;    // [n_runs + 1]
  uint32_t* nsym;    // [n_runs] initial symbols of the run
  uint32_t* soff;    // [n_runs + 1] exclusive scan of nsym
  uint32_t* fcnt;    // [n_runs] final tokens of the run
  uint32_t* wpos;    // [n_runs + 1] exclusive scan of fcnt
  uint32_t* tok;     // [soff[n_runs]] run r's final symbols at tok[soff[r] ..]
  uint32_t* list2;   // runs of kTier1 < nsym <= kTier2
  uint32_t* list3;   // runs of nsym > kTier2
  uint64_t* state3;  // list 3: the run's place in `state` (4 u32 arrays of nsym each from there)
  uint32_t* state;
  uint32_t* ctr;     // [kNumCtr]
  const uint32_t* empty_before;  // [n_docs + 1] byte-level with prefix_space: empty texts before each text; else null
};

// byte-level start bits: every 0x20 byte and every non-empty text's first byte (also into dbits)
hipError_t launch_byte_starts(const Batch& b, hipStream_t s);
// pc[w] = set bits of bits[w]; cpc[w] (non-null: char model) = code-point starts among the word's bytes
hipError_t launch_popc(const Batch& b, uint32_t* pc, uint32_t* cpc, hipStream_t s);
hipError_t launch_runs(const Batch& b, hipStream_t s);                      // runs from bits and wrank
hipError_t launch_word_info(const Model& m, const Batch& b, uint32_t n_runs, hipStream_t s);  // nsym, lists, ctr
// the three merge tiers: tok and fcnt of every run
hipError_t launch_merge(const Model& m, const Batch& b, uint32_t n_runs, uint32_t n2, uint32_t n3, hipStream_t s);
hipError_t launch_empty_flags(const Batch& b, uint32_t* flag, hipStream_t s);  // flag[d] = text d is empty
// ids[...] = sym_id of every run's final symbols, and tok_off[d] for d <= n_docs
hipError_t launch_emit(const Model& m, const Batch& b, uint32_t n_runs, uint32_t* ids, uint64_t* tok_off, hipStream_t s);

}  // namespace ctok_sm
