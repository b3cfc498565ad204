// Internal interface between the classic BPE trainer's host (bpe_train_host.cpp) and its kernels
// (bpe_train.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trainer_internal.h"  // ctok_train::Words: the device CSR of the training words

namespace ctok_bpe {

using ctok_train::Words;

constexpr uint64_t kEmptyKey = ~0ull;  // no pair (a, b) has a = b = 0xFFFFFFFF
constexpr uint32_t kMaxProbe = 8192;   // slots one add looks at before it gives up
constexpr uint32_t kBestBlocks = 1024; // partials of the first k_pair_best launch, at most

constexpr int kCtrTaken = 0;     // slots that hold a key (keys are never removed between rebuilds)
constexpr int kCtrOverflow = 1;  // != 0: an add found no slot; the counts are not complete
constexpr int kNumCtr = 2;

// The resident pair table: open addressing with linear probing, key a << 32 | b, i64 count.  It is
// kept across merges: a merge subtracts and adds in place, a pair whose count fell to 0 keeps its
// slot until the next rebuild.  Any capacity >= 1 (not only powers of two).
struct Table {
  uint64_t* keys;
  int64_t* vals;
  uint32_t cap;
  uint32_t* ctr;  // [kNumCtr]
};

struct Best {       // what one search for the best pair reports (32 bytes)
  int64_t count;    // 0: no pair with a count > 0
  uint64_t key;
  uint64_t taken;
  uint64_t overflow;
};

// pbits = the run starts of the whitespace split (ws_split_hd.h) of text[0 .. n_bytes), plus the
// first byte of every non-empty text (doc_off: n_docs + 1 offsets); n_bytes > 0
hipError_t launch_ws_bits(const uint8_t* text, uint32_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                          uint32_t* pbits, hipStream_t s);
// every adjacent pair of every word += the word's frequency (words of frequency 0 add nothing)
hipError_t launch_pair_count(const Words& W, const Table& T, hipStream_t s);
// the best pair of the table (pair_best_hd.h) and the table's counters -> *out (device memory);
// partial: [2 * kBestBlocks] u64 scratch
hipError_t launch_pair_best(const Table& T, uint64_t* partial, Best* out, hipStream_t s);
// every word rewritten with (a, b) -> nid, left to right; the table follows exactly
hipError_t launch_merge(const Words& W, const Table& T, uint32_t a, uint32_t b, uint32_t nid, hipStream_t s);

}  // namespace ctok_bpe
