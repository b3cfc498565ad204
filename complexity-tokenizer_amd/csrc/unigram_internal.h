// Internal interface between the Unigram host runtime (unigram_host.cpp) and its kernels
// (unigram.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wordcount_internal.h"  // ctok_wc::Table and its counters
#include "wp_table_hd.h"

namespace ctok_uni {

// ---- Metaspace: the NFC text of n_docs documents -> sentence bytes behind each other ---------------
// Span i owns the input positions [64 i, 64 i + 64) up to and including n_bytes (a document that
// starts at n_bytes is empty and still gives its prefix): n_spans = n_bytes / 64 + 1.
//   measure: len[i] = output bytes, nsent[i] = sentences that start in span i; the caller scans
//            both (n_spans + 1 entries each, the totals last)
//   write:   the bytes to out[len[i] ..] and the sentences' first bytes to sent_off[nsent[i] ..]
//            (the caller sets sent_off[total sentences] = total bytes)
inline uint64_t meta_spans(uint64_t n_bytes) { return n_bytes / 64 + 1; }
hipError_t launch_meta_measure(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                               uint64_t* len, uint64_t* nsent, hipStream_t s);
hipError_t launch_meta_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                             const uint64_t* len, const uint64_t* nsent, uint8_t* out, uint64_t* sent_off, hipStream_t s);

// ---- sentences on the device -----------------------------------------------------------------------
// text: n_bytes sentence bytes and >= 16 readable bytes behind them; sentence k = text[sent_off[k] ..
// sent_off[k + 1]), k < n_sent (an empty one is allowed: it has no chars).
struct Sents {
  const uint8_t* text;
  uint32_t n_bytes;
  const uint64_t* sent_off;
  uint64_t n_sent;
};

// bits (zeroed by the caller, a bit per byte): set at every non-empty sentence's first byte
hipError_t launch_sent_bits(const Sents& x, uint32_t* bits, hipStream_t s);
// lead[p] = 1 where byte p starts a char, p < n_bytes; the caller's exclusive scan is cidx
hipError_t launch_lead_flags(const Sents& x, uint32_t* lead, hipStream_t s);
// sent_c[k] = cidx[sent_off[k]], k <= n_sent: sentence k holds the chars [sent_c[k], sent_c[k + 1])
hipError_t launch_sent_chars(const Sents& x, const uint32_t* cidx, uint32_t* sent_c, hipStream_t s);

// ---- substring counts ------------------------------------------------------------------------------
// Every substring of 1 .. max_chars chars inside a sentence is added to the table with count 1 per
// occurrence (wordcount_hd.h descriptors into x.text; keys all kEmpty, vals and ctr zero before).
// ctr[kCtrOverflow] bit 0: a probe sequence ran out; bit 1: a substring of 0xFFFF bytes or more.
hipError_t launch_sub_count(const Sents& x, const uint32_t* bits, uint64_t max_chars, const ctok_wc::Table& t, hipStream_t s);
// the n_used slots taken as (first occurrence, bytes, count)
hipError_t launch_sub_drain(const ctok_wc::Table& t, uint32_t n_used, uint32_t* pos, uint32_t* len, uint32_t* cnt,
                            hipStream_t s);

// ---- lattice ---------------------------------------------------------------------------------------
// lat[j * n_chars + c] = symbol of the pattern of j + 1 chars that starts at char c inside c's
// sentence, or wptab::kNone; j < wl, c < n_chars.  Every entry is written.
hipError_t launch_lattice(const Sents& x, const uint32_t* bits, const uint32_t* cidx, const wptab::View& v, uint32_t wl,
                          uint32_t n_chars, uint32_t* lat, hipStream_t s);

// ---- Viterbi ---------------------------------------------------------------------------------------
struct Viterbi {
  const uint32_t* sent_c;  // [n_sent + 1]
  uint64_t n_sent;
  const uint32_t* lat;
  uint32_t n_chars;
  uint32_t wl;             // lengths the lattice holds
  uint32_t wv;             // lengths a step looks at: 0, or max(wl, 1) for the one-char fallback
  const double* score;     // by symbol
  const uint32_t* live;    // by symbol: 0 = pruned; null: all live
  double fb_score;         // the one-char fallback when nothing live matches the char
  uint32_t fb_sym;
  uint32_t* back_len;      // [n_chars] by the token's last char: its chars, 0 = nothing reaches here
  uint32_t* back_sym;      // [n_chars] its symbol (fb_sym for the fallback)
};
constexpr uint32_t kMaxWindow = 4094;  // the ring of the last best values is LDS: (wv + 2) f64 rounded up
hipError_t launch_viterbi(const Viterbi& a, hipStream_t s);

// the trainer's backtrack: count[sym] += 1 for every token that is a vocab string; *err |= 1 where
// a position is reached by nothing (the reference's panic), |= 2 where the back pointers are broken
hipError_t launch_back_train(const Viterbi& a, unsigned long long* count, uint32_t* err, hipStream_t s);
// the model's backtrack in two launches around the caller's scan_u32: cnt[d] = ids of text d; then
// ids written from pos[d] on and tok_off[d] = pos[d], d <= n_sent.  Where nothing reaches a position
// the reference emits id 0 and stops (src/models.rs:261-265).
hipError_t launch_back_count(const Viterbi& a, uint32_t* cnt, hipStream_t s);
hipError_t launch_back_emit(const Viterbi& a, const uint32_t* pos, uint32_t* ids, uint64_t* tok_off, hipStream_t s);

}  // namespace ctok_uni
