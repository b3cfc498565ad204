// Internal interface between the host runtime of the pipeline tokenizer (pipeline_host.cpp) and the
// kernels of the id-keyed word BPE (wordbpe.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wordbpe_hd.h"

namespace ctok_wb {

constexpr uint32_t kTier1 = 32;    // symbols of a segment one thread merges in LDS columns
constexpr uint32_t kTier2 = 2048;  // symbols of a segment one wavefront merges in LDS (4 u32 arrays: 32 KiB)
// The most symbols of one segment.  The literal loop is quadratic in a segment's length, so a longer
// one is refused before any merge kernel runs (DESIGN.md 4.6k has the measured basis).
constexpr uint32_t kMaxWordSymbols = 1u << 15;
// The most bytes of a word in which an added token's bytes occur: one thread walks such a word, and a
// byte position can cost it a compare of every token that shares the position's first byte.  So the
// bound of a handle is kFlaggedWork / (the most bytes of such a group), at most kMaxFlaggedWordBytes.
// The filter pass spends up to the same compares at every byte of a batch, the whole grid at work: a
// batch of more than kMatchWork / (group bytes) bytes is refused before it runs.  DESIGN.md 4.6k has
// the measured basis of both.
constexpr uint32_t kMaxFlaggedWordBytes = 1u << 20;
constexpr uint64_t kFlaggedWork = 1ull << 23;  // one thread: about 1e7 byte compares a second, two passes
constexpr uint64_t kMatchWork = 1ull << 40;    // the grid: about 5.5e11 a second

enum {
  kCtrList2 = 0,
  kCtrList3 = 1,
  kCtrMaxSym = 2,
  kCtrPanic = 3,  // the lowest segment that saw a marked pair (wordbpe::kNoPanic: none); atomicMin
  kCtrState = 4,  // u64: positions reserved for list 3
  kCtrMaxFlagged = 6,
  kNumCtr = 8
};

struct Tables {  // device pointers, owned by the host runtime
  wordbpe::PairView pairs;
  wordbpe::CpView cps;
  wordbpe::AddedView added;
  uint32_t first_byte[8];
};

// One call's words and segments.  The words are packed as ctok_pretokenizer_run_device leaves them:
// word j = text[word_off[j] .. word_off[j + 1]), text i owns words text_word[i] .. text_word[i + 1].
// A bitmap has a bit per byte (bit g of word g / 32) and n_w + 1 words, the last one clear.
struct Batch {
  const uint8_t* text;
  uint32_t n_bytes;
  uint32_t n_w;  // ceil(n_bytes / 32)
  const uint64_t* word_off;  // [n_words + 1]
  uint32_t n_words;
  const uint64_t* text_word;  // [n_texts + 1]
  uint64_t n_texts;
  uint32_t* wbits;   // the first byte of every non-empty word
  uint32_t* mbits;   // where some added token's bytes stand inside one word (null: no added tokens)
  uint32_t* kbits;   // the first byte of every char that has a vocab id
  uint32_t* kpc;     // [n_w + 1] popcount of kbits
  uint32_t* krank;   // [n_w + 2] exclusive scan of kpc
  uint32_t* wseg;    // [n_words] segments of the word
  uint32_t* segoff;  // [n_words + 1] exclusive scan of wseg (null: every word is one segment)
  wordbpe::Seg* segs;  // [n_segs]
  uint32_t n_segs;
  uint32_t flag_cap;  // bytes of a word that may run the added-token loop (the handle's bound)
  uint32_t* nsym;    // [n_segs] initial symbols
  uint32_t* soff;    // [n_segs] the segment's place in sym: the kept chars before its first byte
  uint32_t* fcnt;    // [n_segs] final ids (an added token: 1)
  uint32_t* wpos;    // [n_segs + 1] exclusive scan of fcnt
  uint32_t* sym;     // [kept chars] initial ids, then the final ids of segment s at sym[soff[s] ..]
  uint32_t* list2;   // segments of kTier1 < nsym <= kTier2
  uint32_t* list3;   // segments of nsym > kTier2
  uint64_t* state3;  // list 3: the segment's place in `state` (4 u32 arrays of nsym each from there)
  uint32_t* state;
  uint32_t* ctr;     // [kNumCtr]
};

hipError_t launch_word_bits(const Batch& b, hipStream_t s);                      // wbits (cleared by the caller)
hipError_t launch_match_bits(const Tables& t, const Batch& b, hipStream_t s);    // mbits
hipError_t launch_seg_count(const Tables& t, const Batch& b, hipStream_t s);     // wseg, ctr[kCtrMaxFlagged]
hipError_t launch_seg_write(const Tables& t, const Batch& b, hipStream_t s);     // segs
hipError_t launch_keep_bits(const Tables& t, const Batch& b, hipStream_t s);     // kbits, kpc
hipError_t launch_symbols(const Tables& t, const Batch& b, hipStream_t s);       // sym
hipError_t launch_seg_info(const Batch& b, hipStream_t s);                       // nsym, soff, fcnt of added tokens, lists, ctr
// the three merge tiers: the final ids and fcnt of every segment, ctr[kCtrPanic]
hipError_t launch_merge(const Tables& t, const Batch& b, uint32_t n2, uint32_t n3, hipStream_t s);
// ids[...] = every segment's final ids, tok_off[i] for i <= n_texts
hipError_t launch_emit(const Batch& b, uint32_t* ids, uint64_t* tok_off, hipStream_t s);
hipError_t launch_iota(uint64_t* p, uint64_t n, hipStream_t s);  // p[i] = i for i < n

}  // namespace ctok_wb
