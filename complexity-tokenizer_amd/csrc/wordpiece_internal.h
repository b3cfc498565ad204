// Internal interface between the WordPiece host runtime (wordpiece_host.cpp) and its kernels
// (wordpiece.hip, lowercase.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bpe_train_internal.h"  // ctok_bpe::Table, Words, launch_pair_count, launch_pair_best, launch_ws_bits
#include "wp_table_hd.h"

namespace ctok_wp {

using ctok_bpe::Table;
using ctok_train::Words;

// A text whose words are marked by their first bytes: starts has a bit per byte (bit g of word
// g / 32), set where a word begins (and, in a text with whitespace, where a whitespace run
// begins: ws_split_hd.h).  text has >= 16 readable bytes past n_bytes.
struct Text {
  const uint8_t* text;
  const uint32_t* starts;
  uint32_t n_bytes;
};

// The longest match at every byte: msym[p] / mlen[p] = symbol and byte length of the longest
// pattern of p's form (0 at a set start bit, else 1) that starts at p inside p's word, or
// (wptab::kNone, 0) where p is no code-point start, nothing matches, or (skip_ws) p is whitespace.
struct Matches {
  uint32_t* msym;
  uint32_t* mlen;
};

// k_wp_match: all of the above from the table
hipError_t launch_match(const Text& x, const wptab::View& v, bool skip_ws, const Matches& m, hipStream_t s);

// k_wp_add: one new string's patterns (pat0 in form 0, pat1 in form 1; a length of 0: none; device
// pointers) with symbol sym.  Where a pattern matches inside the word and is longer than the match
// stored, or as long and the stored symbol is `relabel` (the fallback symbol of prefix + char when
// the new string is that very string; else wptab::kNone), it replaces it and the word is marked: dirty[w] = 1 for word w = text[woff[w] .. woff[w + 1]).
hipError_t launch_add(const Text& x, const uint8_t* pat0, uint32_t len0, const uint8_t* pat1, uint32_t len1,
                      uint32_t sym, uint32_t relabel, const Matches& m, const uint32_t* woff, uint32_t n_words,
                      uint32_t* dirty, hipStream_t s);

// k_wp_walk, the trainer's: every word with dirty[w] != 0 (every word when `all`) is tokenised
// again by following the matches from its first byte; its tokens replace the old ones in W (word
// w has room for W.wstart[w + 1] - W.wstart[w] tokens) and, when T is non-null, the old adjacent
// pairs leave the pair table and the new ones enter it, weighted by the word's frequency.
// dirty[w] is cleared.  stat[0] |= 1 where a chain does not end at its word's end; stat[1] += the
// words walked.
hipError_t launch_walk_train(const uint32_t* woff, const Matches& m, const Words& W, const Table* T, uint32_t* dirty,
                             bool all, unsigned long long* stat, hipStream_t s);

// k_wp_walk, the model's, in two launches around a scan.  A word of more than max_chars chars gives
// unk; elsewhere a byte without a match gives unk and the walk moves on one char (has_unk == 0:
// nothing instead of unk).
//   count: cnt[p] = ids of the word that starts at p (0 where none does), p < n_bytes
//   emit:  the same walk, ids written from pos[p] on (pos = exclusive scan of cnt)
//   tok_off[d] = pos[doc_off[d]] for d <= n_docs (pos[n_bytes] = the total)
hipError_t launch_model_count(const Text& x, const Matches& m, uint64_t max_chars, uint32_t has_unk, uint32_t* cnt,
                              hipStream_t s);
hipError_t launch_model_emit(const Text& x, const Matches& m, uint64_t max_chars, uint32_t has_unk, uint32_t unk_id,
                             const uint32_t* pos, uint32_t* ids, const uint64_t* doc_off, uint64_t n_docs,
                             uint64_t* tok_off, hipStream_t s);

// lowercase.hip: str::to_lowercase of every text (lowercase_hd.h).  Phase 1 writes len[i] = output
// bytes of input span i (kLowerSpan bytes) and ORs *changed when a span's output differs from its
// input; the caller scans len (n_spans + 1 entries) and, when *changed, phase 2 writes the bytes
// and out_off[d] (n_docs + 1) = the position of in_off[d].
constexpr uint32_t kLowerSpan = 64;
hipError_t launch_lower_count(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                              uint64_t* len, uint32_t* changed, hipStream_t s);
hipError_t launch_lower_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                              const uint64_t* pos, uint8_t* out, uint64_t* out_off, hipStream_t s);

}  // namespace ctok_wp
