// Internal interface between the host runtime of the pipeline tokenizer (pipeline_host.cpp) and the
// kernels of its Encoding path (pipeline_enc.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pipeline_enc_hd.h"

namespace ctok_pe {

// The most work of one sequence's word search (DESIGN.md 4.6l has the definition and the measured
// basis): one wavefront walks a sequence, and a word that is not found scans to the text's end.
constexpr uint64_t kMaxFindWork = 1ull << 28;  // measured: 1.38 s all-miss (2^29: 2.83 s)
// `work` does not see what a partial match costs: a lane that finds the needle's first byte compares on,
// and a window lasts as long as its longest compare, about 126 ns a byte.  So the bytes one lane compares
// after first bytes are bounded too, by the work limit / kFindCompareShare: 2^24 of them take about 2.1 s.
constexpr uint64_t kFindCompareShare = 16;
constexpr uint32_t kMaxSpecial = 1024;  // special added tokens (wordbpe::kMaxAdded added tokens at most)
constexpr uint64_t kNoPanic = ~0ull;
constexpr uint32_t kNoSeq = 0xFFFFFFFFu;

enum {
  kRepPanic = 0,    // u64: sequence << 32 | byte index of the lowest sequence whose search start is inside a char; atomicMin
  kRepMaxWork = 1,  // u64: the most work of a sequence; atomicMax
  kRepOver = 2,     // u64: the lowest sequence whose work is above the limit (low half; kNoSeq: none); atomicMin
  kRepShort = 3,    // u64: the lowest row whose processed ids are fewer than its ids (low half; kNoSeq: none); atomicMin
  kRepCompares = 4, // u64: the lowest sequence in which one lane compared more than the limit's bytes of partial matches; atomicMin
  kNumRep = 5
};

// Sequence q is text[off[q] .. off[q + 1]) and owns words text_word[q] .. text_word[q + 1) of the packed
// words (word j = words[word_off[j] .. word_off[j + 1])).
struct Find {
  const uint8_t* text;
  const uint64_t* off;
  uint64_t n_seqs;
  const uint8_t* words;
  const uint64_t* word_off;
  const uint64_t* text_word;
  uint64_t n_words;
  uint64_t* wstart;  // [n_words] relative to the sequence's text
  uint64_t* wend;
  uint64_t* work;    // [n_seqs]
  unsigned long long* rep;  // [kNumRep]
  uint64_t limit;      // of a sequence's work
  uint64_t cmp_limit;  // of the bytes one lane compares after first bytes
};

struct Spans {
  const uint32_t* ids;
  uint64_t n_ids;
  uint64_t* scan;  // [n_ids + 1]: token byte lengths, then their exclusive scan in place
  const uint32_t* len_id;   // the id -> length table: sorted ids, their lengths
  const uint32_t* len_val;
  uint32_t n_len;
  const uint32_t* wpos;  // [n_words + 1] every word's first id
  uint32_t n_words;
  const uint64_t* text_word;  // [n_seqs + 1]
  uint64_t n_seqs;
  const uint64_t* wstart;
  const uint64_t* wend;
  uint64_t* offsets;   // [2 * n_ids]
  uint32_t* word_ids;  // [n_ids]
};

// Row r holds the ids of sequences r * per_row .. (r + 1) * per_row - 1 (per_row: 1, or 2 for pairs).
struct Rows {
  const uint64_t* tok_off;  // [n_rows * per_row + 1] ids before every sequence
  uint32_t per_row;
  uint64_t n_rows;
  uint64_t* seq_off;        // [n_rows + 1] out: ids before every row
  uint64_t* n_a;            // [n_rows] out
  const uint32_t* out_ids;  // the processed ids
  const uint64_t* row_off;  // [n_rows + 1] of the processed rows
  uint64_t n_cells;
  const uint32_t* special;  // sorted ids of the special added tokens
  uint32_t n_special;
  uint32_t* type_ids;       // [n_cells]
  uint32_t* special_mask;
  unsigned long long* rep;
};

hipError_t launch_word_find(const Find& f, hipStream_t s);  // wstart, wend, work, rep (set by the caller)
hipError_t launch_tok_len(const Spans& p, hipStream_t s);   // scan[k] = the bytes of ids[k]'s string, scan[n_ids] = 0
hipError_t launch_tok_spans(const Spans& p, hipStream_t s);
hipError_t launch_row_heads(const Rows& r, hipStream_t s);  // seq_off, n_a
hipError_t launch_enc_rows(const Rows& r, hipStream_t s);   // type_ids, special_mask, rep[kRepShort]

}  // namespace ctok_pe
