// Internal interface between the trainer host (trainer_host.cpp) and the word-counting kernels
// (wordcount.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ctok_wc {

// counters of one chunk (device words, zeroed by the host before the count)
constexpr int kCtrUsed = 0;      // slots taken (the used list's length = unique words)
constexpr int kCtrOverflow = 1;  // != 0: a probe sequence ran out; the chunk's table is not complete
constexpr int kCtrPieces = 2;    // pieces seen
constexpr int kCtrWords = 3;     // words counted (pieces of >= min_len bytes)
constexpr int kNumCtr = 4;

struct Text {             // what a pretok-only encode call leaves on the device
  const uint8_t* text;    // 4-byte aligned, >= 16 readable bytes past n_bytes
  const uint32_t* pbits;  // bit g = a piece starts at byte g; bits >= n_bytes are clear
  uint32_t n_bytes;
  uint32_t n_words;       // (n_bytes + 31) / 32
};

struct Table {            // open addressing over wordcount_hd.h descriptors; capacity mask + 1
  uint64_t* keys;         // wc::kEmpty or a descriptor
  uint32_t* vals;         // the word's count
  uint32_t mask;
  uint32_t* used;         // [capacity] slots taken, in the order they were taken
  uint32_t* ctr;          // [kNumCtr]
};

// ctr[kCtrPieces] += the pieces of the text (the table's capacity is sized from it)
hipError_t launch_pieces(const Text& x, uint32_t* ctr, hipStream_t s);
// every word of >= min_len bytes added to the table (keys all kEmpty, vals and ctr zero before)
hipError_t launch_count(const Text& x, const Table& t, uint32_t min_len, hipStream_t s);
// the n_used slots of the used list as (bytes, offsets, counts): word i = out_bytes[out_off[i] ..
// out_off[i + 1]) with count out_cnt[i]; out_off has n_used + 1 entries, out_bytes <= n_bytes bytes.
// pos: [n_used] scratch; tmp: scan scratch of >= scan_tmp_elems(n_used + 1) u64
uint64_t drain_tmp_elems(uint64_t n_used);
hipError_t launch_drain(const Text& x, const Table& t, uint32_t n_used, uint8_t* out_bytes, uint64_t* out_off,
                        uint32_t* out_cnt, uint32_t* pos, uint64_t* tmp, uint64_t tmp_cap, hipStream_t s);

}  // namespace ctok_wc
