// Internal interface between the host runtime of the pipeline tokenizer (pipeline_host.cpp) and the
// kernels of its padded batches and stride windows (pipeline_win.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pipeline_win_hd.h"

namespace ctok_pw {

constexpr uint64_t kNoRow = ~0ull;
constexpr uint32_t kNoneCell = 0xFFFFFFFFu;  // word_ids / sequence_ids past a list's end, and None inside sequence_ids

enum {
  kRepPanic = 0,  // u64: the lowest row the reference panics on (kNoRow: none); atomicMin
  kRepMain = 1,   // u64: the longest main window; atomicMax
  kNumRep = 2
};

// What the Encoding call (or the id call, without special tokens) left on the device, and the call's options.
// Row r: processed ids[row_off[r] .. row_off[r + 1]) (P of them), lists of n = seq_off[r + 1] - seq_off[r].
struct Win {
  const uint32_t* ids;
  const uint32_t* type_ids;      // null: 0 for the first n_a ids of a row, 1 for the rest
  const uint32_t* special_mask;  // null: 0
  const uint64_t* row_off;
  const uint64_t* offsets;       // null: the rows have no offsets and no word ids
  const uint32_t* word_ids;
  const uint64_t* seq_off;
  const uint64_t* n_a;
  const uint32_t* tokenless;     // null, or [n_rows]: ids of the row that have no vocab string
  uint64_t n_rows;
  uint32_t mode;                 // pwin::Mode
  uint32_t pad_left;
  uint32_t pad_id;
  uint64_t m, stride;
  uint64_t target;               // of window 0's padding (0: none); set after the plan
  uint64_t n_windows, width;     // set after the plan
  uint64_t* row_win;             // [n_rows + 1]: counts, then their exclusive scan
  unsigned long long* rep;       // [kNumRep]
  // the records, [n_windows]
  uint64_t* win_len;
  uint32_t* win_row;
  uint64_t* win_start;    // null: not wanted
  uint64_t* win_off_len;  // null: not wanted
  uint64_t* win_seq_len;  // null: not wanted
  // the arrays, [n_windows, width]
  uint32_t* out_ids;
  uint32_t* out_attn;     // null: not wanted, as all below
  uint32_t* out_type;
  uint32_t* out_special;
  uint64_t* out_offsets;  // two per cell
  uint32_t* out_word;
  uint32_t* out_seq;
};

// tokenless[r] += 1 per id of row r (ids[seq_off[r] ..]) that is not in the sorted table; tokenless is zeroed by the caller
hipError_t launch_tokenless(const uint32_t* ids, uint64_t n_ids, const uint64_t* seq_off, uint64_t n_rows, const uint32_t* table,
                            uint32_t n_table, uint32_t* tokenless, hipStream_t s);
hipError_t launch_plan(const Win& w, hipStream_t s);     // row_win (counts), rep (set by the caller)
hipError_t launch_records(const Win& w, hipStream_t s);  // after the scan of row_win
hipError_t launch_write(const Win& w, hipStream_t s);    // after the records

}  // namespace ctok_pw
