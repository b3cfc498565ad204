// What the PreTokenizer's host runtime (pretok_host.cpp) calls in pretok.hip.  Not part of the C ABI.
// Every pointer is a device pointer (a Step's too).  A batch is n bytes with two bitmaps of
// (n + 63) / 64 words (pretok_hd.h); doc_off[0] = 0 and doc_off[n_docs] = n.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pretok_hd.h"

namespace ctok_pt {

constexpr uint32_t kThreads = 256;                      // a workgroup: 4 wavefronts, one bitmap word each
constexpr uint32_t kWaveWords = 16;                     // bitmap words a wavefront walks in the script carry
constexpr uint32_t kWaveTile = kWaveWords * 64;         // ... in bytes
constexpr uint32_t kTile = kWaveTile * (kThreads / 64);  // a workgroup's tile there

struct Bits {
  uint64_t* inw;
  uint64_t* beg;
};

inline uint64_t words64(uint64_t n) { return (n + 63) / 64; }
inline uint64_t wave_tiles(uint64_t n) { return (n + kWaveTile - 1) / kWaveTile; }

// every text one word: in_word everywhere, begin at the first byte of every non-empty text
hipError_t launch_init(uint64_t n, const uint64_t* doc_off, uint64_t n_docs, Bits out, hipStream_t s);
// A pure splitter: out = the step over x.  UnicodeScripts: tail and carry have wave_tiles(n) entries.
// A literal `split`: cand and mark have n bytes.  A DFA `split` (M_DFA): mark has n bytes, len n entries,
// tmax and tcarry wave_tiles(n) entries (the prefix max of the matches' ends, tile by tile), *over is
// 0xFFFFFFFF and receives the lowest start whose run passes the step's cap.  Removed without invert: wpos has words64(n) + 1
// entries, tmp is scan_u64's, whit has room for every word (one per begin bit) + 1.
struct Scratch {
  uint8_t* tail;
  uint8_t* carry;
  uint8_t* cand;
  uint8_t* mark;
  uint64_t* wpos;
  uint64_t* tmp;
  uint64_t tmp_cap;
  uint8_t* whit;
  uint32_t* len;
  uint32_t* tmax;
  uint32_t* tcarry;
  uint32_t* over;
};
// A DFA's transition table is copied into LDS when it has at most this many bytes: five workgroups of
// kThreads then still fit the 160 KiB of a CU.  A larger table is read from global memory.
constexpr uint32_t kDfaLdsBytes = 32u << 10;
hipError_t launch_split(const pretok::Tables& T, pretok::Step st, const pretok::Ctx& x, const Scratch& sc, Bits out,
                        hipStream_t s);
// words that begin in the batch (a host value; the stream is waited for)
hipError_t count_begins(const pretok::Ctx& x, uint64_t* wpos, uint64_t* tmp, uint64_t tmp_cap, uint64_t* n_words,
                        hipStream_t s);
// A rewriter: len[j] = output bytes of bitmap word j's input bytes (words64(n) + 1 entries) ...
hipError_t launch_rw_count(const pretok::Tables& T, const pretok::Step& st, const pretok::Ctx& x, uint64_t* len, hipStream_t s);
// ... and after scan_u64 over len: the bytes, one begin flag per output byte, the texts' new offsets
hipError_t launch_rw_write(const pretok::Tables& T, const pretok::Step& st, const pretok::Ctx& x, const uint64_t* pos,
                           const uint64_t* doc_off, uint64_t n_docs, uint8_t* out, uint8_t* out_beg, uint64_t* out_off,
                           hipStream_t s);
// the bitmaps of a rewriter's output: in_word everywhere, begin from the flags
hipError_t launch_pack(const uint8_t* flags, uint64_t n, Bits out, hipStream_t s);

// The final gather.  cb / cw: words64(n) + 1 entries each, the in_word / begin bits per bitmap word.
hipError_t launch_gather_count(const pretok::Ctx& x, uint64_t* cb, uint64_t* cw, hipStream_t s);
// e[d] = 1 when text d is empty (n_docs + 1 entries, for scan_u64); the host asks this of the input's
// offsets, before any step: a text whose words all get dropped on the way is not the empty word
hipError_t launch_empty(const uint64_t* doc_off, uint64_t n_docs, uint64_t* e, hipStream_t s);
struct Gather {
  const uint64_t* posb;  // cb, cw after scan_u64 (the totals at [words64(n)])
  const uint64_t* posw;
  const uint64_t* doc_off;
  uint64_t n_docs;
  const uint64_t* ex;  // texts empty in the input before text d (n_docs + 1 entries), or null: they own no word
  uint64_t ew, eb;     // the words every empty text owns, and their bytes
  const uint64_t* ew_off;
  const uint8_t* ew_bytes;
  uint64_t n_words, n_bytes;  // the totals, the empty texts' included
  uint8_t* words;
  uint64_t* word_off;   // n_words + 1
  uint64_t* text_word;  // n_docs + 1
};
hipError_t launch_gather(const pretok::Ctx& x, const Gather& g, hipStream_t s);

}  // namespace ctok_pt
