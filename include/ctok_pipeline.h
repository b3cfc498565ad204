/* ctok_pipeline.h -- C ABI of the pipeline tokenizer on the GPU.
 *
 * The reference's HuggingFaceTokenizer (Complexity-ML/complexity-tokenizer v0.3.3,
 * src/huggingface/mod.rs:247-334, :551-613, :1080-1101) with any normaliser and any pre-tokenizer:
 * a batch goes through a ctok_normalizer, a ctok_pretokenizer and the id-keyed word BPE
 * (src/bpe.rs:52-153: one id per char of a word, a char without a one-char vocab string dropped,
 * then lowest rank, leftmost, one merge per step) with the added-token loop inside every word
 * (mod.rs:566-675), without a trip through host memory.  The rank / new-id quirk of
 * BpeTokenizer::new is kept: a pair's new id is that of the filtered merge list at the pair's
 * unfiltered rank, and a pair whose rank is past that list fails the call with CTOK_E_PANIC and the
 * reference's message as soon as it is seen adjacent, for the lowest-numbered text that has one.
 *
 * Refusals the reference does not have: a vocab id of 2^32 - 1, more than 2^24 merges, more than
 * 1024 added tokens, one of more than 1024 bytes, or added tokens that share a first byte and hold
 * more than 32 KiB together (CTOK_E_UNSUPPORTED at create); a word segment of more symbols than
 * ctok_pipeline_limits reports (CTOK_E_UNSUPPORTED before any merge kernel runs); a batch or an
 * intermediate that reaches 4 GiB (CTOK_E_CAPACITY).  With added tokens a byte position can cost a
 * compare of every token that shares its first byte, G bytes for the largest such group, so the work
 * is bounded through G: a word that holds an added token may have min(2^20, 2^23 / G) bytes -- one
 * thread walks it -- and a call's words 2^40 / G bytes (CTOK_E_UNSUPPORTED before the pass that would do
 * the work); ctok_pipeline_limits reports both for a handle.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU path: without a HIP device create returns CTOK_E_DEVICE.  A handle keeps its grow-only device
 * buffers and is used by one thread at a time.
 */
#ifndef CTOK_PIPELINE_H
#define CTOK_PIPELINE_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"
#include "ctok_normalizer.h"
#include "ctok_postprocessor.h"
#include "ctok_pretokenizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_pipeline ctok_pipeline;

/* added_flags bits */
#define CTOK_PIPELINE_AT_SPECIAL 1u
#define CTOK_PIPELINE_AT_SINGLE_WORD 2u
#define CTOK_PIPELINE_AT_LSTRIP 4u
#define CTOK_PIPELINE_AT_RSTRIP 8u
#define CTOK_PIPELINE_AT_NORMALIZED 16u /* stored by the reference, never read by encode */

/* Strings are packed: string i = bytes[off[i] .. off[i + 1]).  The merges are the pairs that split
 * into exactly two parts at ' ', in rank order: strings 2r and 2r + 1 are merge r's left and right. */
typedef struct ctok_pipeline_tables {
  const uint8_t* vocab_bytes;
  const uint64_t* vocab_off;
  const uint32_t* vocab_id;
  uint64_t n_vocab;
  const uint8_t* merge_bytes;
  const uint64_t* merge_off;
  uint64_t n_merge_strings;
  const uint8_t* added_bytes;
  const uint64_t* added_off;
  const uint32_t* added_id;
  const uint8_t* added_flags;
  uint64_t n_added;
} ctok_pipeline_tables;

/* encode flags */
#define CTOK_PIPELINE_TOKENIZE 1u /* tokenize (mod.rs:1080-1101): the word BPE without the added-token loop */

/* nz and pt are borrowed (either may be NULL: no normaliser; the whole text is one word) and must
 * outlive the handle and belong to `device`. */
int ctok_pipeline_create(const ctok_pipeline_tables* tables, ctok_normalizer* nz, ctok_pretokenizer* pt, int device,
                         ctok_pipeline** out);
void ctok_pipeline_destroy(ctok_pipeline* p);

/* n_texts host texts.  *ids (tok_off[n_texts] of them) and *tok_off (n_texts + 1) point into the
 * handle and hold until its next call.  CTOK_E_ARG: a text is not UTF-8. */
int ctok_pipeline_encode_batch(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, uint32_t flags,
                               const uint32_t** ids, const uint64_t** tok_off);

/* Same, with every buffer resident in the device's memory and the work ordered on `stream` (a
 * hipStream_t; NULL: the default stream); n_bytes = off[n_texts].  d_ids has room for ids_cap ids,
 * d_tok_off for n_texts + 1.  d_off[0] must be 0 and d_off must not decrease (not checked: the offsets are
 * device memory; without a normaliser and a pre-tokenizer they are the words' offsets as they stand, and
 * n_bytes sizes the per-byte bitmaps).  The bytes are taken as they are: what is not well-formed UTF-8 is a
 * unit in no vocab string, so it gives no id.  *n_ids_out receives the number of ids, also on
 * CTOK_E_CAPACITY, when ids_cap is too small and nothing is written.  The call returns after the
 * stream has finished the work. */
int ctok_pipeline_encode_batch_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_texts,
                                      uint64_t n_bytes, uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_tok_off,
                                      uint64_t* n_ids_out, void* stream);

/* The HIP-event time of each stage of the last call: normalize, pre_tokenize, segments, symbols,
 * merges, emit. */
#define CTOK_PIPELINE_STAGES 6
int ctok_pipeline_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_STAGES]);
const char* ctok_pipeline_stage_name(uint64_t i); /* "" past the end */

typedef struct ctok_pipeline_limits_t {
  uint32_t tier1;                  /* symbols of a segment one thread merges */
  uint32_t tier2;                  /* symbols of a segment one wavefront merges in LDS */
  uint64_t max_word_symbols;       /* of this handle: CTOK_PIPELINE_MAX_WORD_SYMBOLS, read at create, may lower it */
  uint64_t max_flagged_word_bytes; /* of this handle: bytes of a word that holds an added token */
  uint64_t max_added_tokens;
  uint64_t max_added_token_bytes;
  uint64_t max_merges;
  uint64_t max_added_group_bytes;  /* bytes of the added tokens that share a first byte */
  uint64_t max_batch_bytes;        /* of this handle: bytes of words in one call (lower with added tokens, see above) */
} ctok_pipeline_limits_t;
/* p may be NULL: the built-in limits under the current environment */
void ctok_pipeline_limits(const ctok_pipeline* p, ctok_pipeline_limits_t* out);

/* What the last call did. */
typedef struct ctok_pipeline_info {
  uint64_t texts;
  uint64_t bytes_in;
  uint64_t bytes_normalized;
  uint64_t bytes_words;
  uint64_t words;
  uint64_t segments;
  uint64_t symbols;
  uint64_t ids;
  uint64_t tier2_segments;
  uint64_t tier3_segments;
  uint64_t max_segment_symbols;
} ctok_pipeline_info;
int ctok_pipeline_stats(const ctok_pipeline* p, ctok_pipeline_info* out);

/* ---- Encodings: ids with offsets, word ids and the row masks -------------------------------------------
 *
 * The reference's encode_to_encoding / encode_pair_to_encoding (mod.rs:340-480) before truncation and
 * padding, for a batch.  Every text (and every pair text) is a sequence: it goes through the normaliser,
 * the pre-tokenizer and the word BPE without the added-token loop (CTOK_PIPELINE_TOKENIZE).  Then, all on
 * the device:
 *   - every word, its leading 'Ġ' / '▁' chars trimmed (the whole word when nothing is left), is searched
 *     for in the sequence's original bytes from where the previous word ended; found at pos its span is
 *     (pos, pos + needle bytes), else (start, min(start + word bytes, text bytes)); a search that would
 *     start inside a UTF-8 char is CTOK_E_PANIC "byte index N is not a char boundary";
 *   - token k of a word gets (p, e), e = min(p + bytes of the id's vocab string, word end), p = the
 *     previous e or the word's start; an id without a vocab string has no bytes, of strings that share an
 *     id the last one counts; word_ids is the word's index in its sequence;
 *   - row r is the ids of its text, then of its pair; pp (borrowed, may be NULL, of the same device) runs
 *     over the merged row in the single form; type_ids are 0 for the text's ids, 1 for the pair's and 0
 *     for what the processed row has more; special_tokens_mask is 0 for the first n cells, 1 for the
 *     rest, and 1 wherever the processed id is a special added token's; a processed row shorter than its
 *     ids is CTOK_E_PANIC "attempt to subtract with overflow".
 * offsets and word_ids keep the length n of the ids before pp and are relative to their own sequence.
 *
 * A search scans to the text's end when the word is not there, and one wavefront walks a sequence.  With
 * s where a word's search starts, L the text's bytes and m the needle's: work = pos - s + m on a hit,
 * L - s on a miss; a sequence whose words' work adds up to more than ctok_pipeline_encoding_limits
 * reports is CTOK_E_UNSUPPORTED.  The walk of such a sequence stops at the word that crosses the limit
 * (inside it, once the work is above the limit whatever the search finds): the message holds the work
 * counted up to there.  The work does not count what a partial match costs (a lane that finds the needle's
 * first byte compares on): the bytes one lane compares after first bytes are bounded by max_find_compares,
 * CTOK_E_UNSUPPORTED above it.
 *
 * Which error a failing call reports: CTOK_E_CAPACITY (4 GiB) and CTOK_E_UNSUPPORTED (word symbols, then
 * find work) before any panic; of the panics that of the lowest row, its text before its pair, in a
 * sequence the char boundary before the merge rank; the subtraction last. */

typedef struct ctok_pipeline_encodings {
  const uint32_t* ids;                 /* row_off[n_rows] processed ids */
  const uint32_t* type_ids;
  const uint32_t* special_tokens_mask;
  const uint64_t* row_off;             /* n_rows + 1 */
  const uint64_t* offsets;             /* seq_off[n_rows] (start, end) pairs */
  const uint32_t* word_ids;            /* seq_off[n_rows] */
  const uint32_t* seq_ids;             /* seq_off[n_rows]: the ids before pp, whose vocab strings are the tokens */
  const uint64_t* seq_off;             /* n_rows + 1: the ids before pp */
  const uint64_t* n_a;                 /* n_rows: of them the text's */
  uint64_t n_rows;
} ctok_pipeline_encodings;

/* n_rows host texts and, when pair_off is not NULL, as many pair texts.  *out points into the handle and
 * holds until its next call.  CTOK_E_ARG: a text is not UTF-8. */
int ctok_pipeline_encode_encodings(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n_rows,
                                   const uint8_t* pair_utf8, const uint64_t* pair_off, ctok_postprocessor* pp,
                                   ctok_pipeline_encodings* out);

typedef struct ctok_pipeline_encodings_device {
  uint32_t* ids;                 /* cells_cap each */
  uint32_t* type_ids;
  uint32_t* special_tokens_mask;
  uint64_t cells_cap;
  uint64_t* row_off;             /* n_rows + 1 */
  uint64_t* offsets;             /* 2 * ids_cap */
  uint32_t* word_ids;            /* ids_cap */
  uint32_t* seq_ids;             /* ids_cap; may be NULL: not wanted */
  uint64_t ids_cap;
  uint64_t* seq_off;             /* n_rows + 1 */
  uint64_t* n_a;                 /* n_rows */
  uint64_t n_cells;              /* out: the cells and the ids before pp that the result has, also on CTOK_E_CAPACITY */
  uint64_t n_ids;
} ctok_pipeline_encodings_device;

/* Same, with every buffer resident in the device's memory and the work ordered on `stream`.  The
 * sequences stand in row order: with pairs != 0 sequence 2r is row r's text and 2r + 1 its pair, so d_off
 * has n_rows * 2 + 1 entries; n_bytes is its last.  The rules of ctok_pipeline_encode_batch_device hold:
 * the bytes are taken as they are and no byte at or past a sequence's end reaches a result; u32 arrays
 * must be 4-byte and u64 arrays 8-byte aligned (CTOK_E_ARG before any device is used); a capacity may be
 * exact, nothing past the counts is written; when cells_cap or ids_cap is too small the call is
 * CTOK_E_CAPACITY with both counts returned and nothing written to any of the caller's buffers.  The call
 * returns after the stream has finished the work. */
int ctok_pipeline_encode_encodings_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_rows, int pairs,
                                          uint64_t n_bytes, ctok_postprocessor* pp, ctok_pipeline_encodings_device* out, void* stream);

/* The HIP-event time of the Encoding stages of the last such call: find, spans, rows (the post-processor
 * inside rows); ctok_pipeline_stage_ms has the stages before them. */
#define CTOK_PIPELINE_ENCODING_STAGES 3
int ctok_pipeline_encoding_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_ENCODING_STAGES]);
const char* ctok_pipeline_encoding_stage_name(uint64_t i); /* "" past the end */

typedef struct ctok_pipeline_encoding_limits_t {
  uint64_t max_find_work;      /* of this handle: CTOK_PIPELINE_MAX_FIND_WORK, read at create, may lower it */
  uint64_t max_special_tokens;
  uint64_t max_find_compares;  /* of this handle: bytes one lane may compare after first bytes, max_find_work / 16 */
} ctok_pipeline_encoding_limits_t;
/* p may be NULL: the built-in limits under the current environment */
void ctok_pipeline_encoding_limits(const ctok_pipeline* p, ctok_pipeline_encoding_limits_t* out);

/* What the last Encoding call did. */
typedef struct ctok_pipeline_encoding_info {
  uint64_t rows;
  uint64_t sequences;
  uint64_t words;
  uint64_t ids;           /* before the post-processor */
  uint64_t cells;         /* of the processed rows */
  uint64_t max_find_work; /* the most work of one sequence */
} ctok_pipeline_encoding_info;
int ctok_pipeline_encoding_stats(const ctok_pipeline* p, ctok_pipeline_encoding_info* out);

/* ---- Padded batches and overflowing stride windows as arrays ---------------------------------------------
 *
 * Tokenizer.__call__'s truncation and padding (src/bindings/tokenizer.rs:33-201 over Encoding::truncate,
 * truncate_with_stride and pad, src/encoding.rs:87-223) applied on the device to what an Encoding call
 * leaves there: [n_windows, width] arrays, with no Encoding of lists in between.  flags are ctok.h's:
 *   - CTOK_P_ADD_SPECIAL: the rows are those of ctok_pipeline_encode_encodings with pp.  Without it they are
 *     Encoding::from_ids over the id path with the added-token loop (tokenizer.rs:64-97): pp is not used,
 *     type ids and sequence ids are 0 for the text's ids and 1 for the pair's, offsets and word ids are empty.
 *   - CTOK_P_PAIRS: the sequences are interleaved, 2r is row r's text and 2r + 1 its pair.
 *   - CTOK_P_TRUNCATE: a row of P > m = max_length ids is cut to m (Encoding::truncate; the remainder is
 *     not returned).  With CTOK_P_WINDOWS as well it becomes 1 + ceil((P - m) / (m - stride)) windows
 *     (truncate_with_stride): window k holds positions [k (m - stride), min(k (m - stride) + m, P)), window 0
 *     is the main encoding and the others are its `overflowing` list in order; stride >= m is CTOK_E_ARG
 *     before any device is used.
 *   - CTOK_P_PAD_LONGEST / CTOK_P_PAD_TO_MAX: window 0 of each row is padded to the longest main window of
 *     the call / to m, in front with CTOK_P_PAD_LEFT; the pad id is the reference's ([PAD], then <pad>, then
 *     0) unless CTOK_P_PAD_ID gives pad_id.  Overflowing windows are never padded.
 * width = max(longest window, padding target).  Cells at or past a window's length hold padding values: the
 * pad id, attention 0, type 0, special 1.
 *
 * offsets, word_ids and sequence_ids keep the reference's quirk: the lists have one entry per id before the
 * post-processor (n, not P), and neither truncation nor padding realigns them.  Window [start, end) takes
 * list[start .. min(end, n)) when n > start, else nothing; pad extends sequence_ids with None (in front on a
 * left pad) and leaves the other two alone.  The arrays hold exactly those lists from cell 0: win_off_len is
 * the length of a window's offsets and word_ids, win_seq_len that of its sequence_ids; past the length
 * offsets are (0, 0) and the other two 0xFFFFFFFF, which also stands for None inside sequence_ids.
 *
 * Panics: the reference slices `tokens` -- one entry per id before the post-processor, or without
 * CTOK_P_ADD_SPECIAL per id that has a vocab string; t of them -- at positions counted in P.  A row with
 * P > m > t panics when it is cut, a row with P > m and P > t when it is windowed: CTOK_E_PANIC with the
 * message of the lowest such row.  The errors of the encode come first, in their own order (above). */

#define CTOK_PIPELINE_WIN_OFFSETS 1u  /* ctok_pipeline_window_opts.want: the host entry's optional arrays */
#define CTOK_PIPELINE_WIN_WORD_IDS 2u
#define CTOK_PIPELINE_WIN_SEQUENCE_IDS 4u

typedef struct ctok_pipeline_window_opts {
  uint32_t flags;       /* CTOK_P_* of ctok.h, as above */
  uint32_t pad_id;      /* with CTOK_P_PAD_ID */
  uint64_t max_length;
  uint64_t stride;      /* with CTOK_P_WINDOWS */
  uint32_t want;        /* CTOK_PIPELINE_WIN_*: ctok_pipeline_encode_windows only */
} ctok_pipeline_window_opts;

typedef struct ctok_pipeline_windows {
  const uint32_t* ids;                 /* [n_windows, width] */
  const uint32_t* attention_mask;
  const uint32_t* type_ids;
  const uint32_t* special_tokens_mask;
  const uint64_t* offsets;             /* [n_windows, width, 2]; NULL unless wanted, as the next two */
  const uint32_t* word_ids;
  const uint32_t* sequence_ids;
  const uint64_t* win_len;             /* [n_windows] the window's Encoding length, padding included */
  const uint32_t* win_row;             /* its row: the overflow-to-sample mapping */
  const uint64_t* win_start;           /* its first position in the row */
  const uint64_t* win_off_len;         /* entries of its offsets and word_ids */
  const uint64_t* win_seq_len;         /* entries of its sequence_ids */
  const uint64_t* row_win;             /* [n_rows + 1]: row r's windows are row_win[r] .. row_win[r + 1] */
  uint64_t n_rows, n_windows, width;
} ctok_pipeline_windows;

/* Host texts as ctok_pipeline_encode_encodings takes them.  *out points into the handle and holds until its
 * next call. */
int ctok_pipeline_encode_windows(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n_rows,
                                 const uint8_t* pair_utf8, const uint64_t* pair_off, ctok_postprocessor* pp,
                                 const ctok_pipeline_window_opts* opts, ctok_pipeline_windows* out);

typedef struct ctok_pipeline_windows_device {
  uint32_t* ids;                 /* cap cells each */
  uint32_t* attention_mask;      /* may be NULL: not wanted, as every pointer below but win_len, win_row, row_win */
  uint32_t* type_ids;
  uint32_t* special_tokens_mask;
  uint64_t* offsets;             /* 2 * cap */
  uint32_t* word_ids;
  uint32_t* sequence_ids;
  uint64_t cap;
  uint64_t* win_len;             /* win_cap each */
  uint32_t* win_row;
  uint64_t* win_start;
  uint64_t* win_off_len;
  uint64_t* win_seq_len;
  uint64_t win_cap;
  uint64_t* row_win;             /* n_rows + 1 */
  uint64_t n_windows;            /* out, also on CTOK_E_CAPACITY */
  uint64_t width;
} ctok_pipeline_windows_device;

/* Same, with every buffer resident in the device's memory and the work ordered on `stream`; d_off and
 * n_bytes as ctok_pipeline_encode_encodings_device takes them.  Its rules hold: the bytes are taken as they
 * are and no byte at or past a sequence's end reaches a result; u32 arrays must be 4-byte and u64 arrays
 * 8-byte aligned (CTOK_E_ARG before any device is used); a capacity may be exact, nothing past
 * n_windows * width cells (twice that for offsets) and n_windows records is written; when
 * n_windows > win_cap or n_windows * width > cap the call is CTOK_E_CAPACITY with n_windows, width and
 * row_win filled and nothing else written.  A call of 2^32 windows or more is CTOK_E_ARG.  The call returns
 * after the stream has finished the work. */
int ctok_pipeline_encode_windows_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_rows,
                                        uint64_t n_bytes, ctok_postprocessor* pp, const ctok_pipeline_window_opts* opts,
                                        ctok_pipeline_windows_device* out, void* stream);

/* The HIP-event time of the window stages of the last such call: plan (counts, scan, records), write;
 * ctok_pipeline_stage_ms and ctok_pipeline_encoding_stage_ms have the stages before them. */
#define CTOK_PIPELINE_WINDOW_STAGES 2
int ctok_pipeline_window_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_WINDOW_STAGES]);
const char* ctok_pipeline_window_stage_name(uint64_t i); /* "" past the end */

/* What the last window call did. */
typedef struct ctok_pipeline_window_info {
  uint64_t rows;
  uint64_t windows;
  uint64_t width;
  uint64_t bytes_written; /* by the write kernel: every cell of every requested array */
} ctok_pipeline_window_info;
int ctok_pipeline_window_stats(const ctok_pipeline* p, ctok_pipeline_window_info* out);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_PIPELINE_H */
