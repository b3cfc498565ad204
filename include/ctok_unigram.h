/* ctok_unigram.h -- C ABI of the Unigram trainer and model on the GPU.
 *
 * Drop-ins for the reference's PyO3 classes `complexity_tokenizer.UnigramTrainer` and
 * `complexity_tokenizer.UnigramModel` (Complexity-ML/complexity-tokenizer v0.3.3,
 * src/bindings/trainers.rs:156-215 over src/trainers.rs:287-546, src/bindings/models.rs:52-87 over
 * src/models.rs:150-299).
 *
 * The trainer's normaliser is NFC and its pre-tokenizer Metaspace('▁', add_prefix_space); neither
 * can be changed.  A text becomes '▁' + its NFC form with every U+0020 rewritten to '▁' (U+2581),
 * cut at the other 24 White_Space code points; empty parts are dropped, so a "sentence" is a whole
 * line and an empty text is the sentence "▁".  NFC, Metaspace, the substring counts, the lookup of
 * every vocab string at every char (the lattice) and the Viterbi search of every EM iteration run
 * on the GPU; the host keeps the strings, sorts, truncates and evaluates the logarithms.
 *
 * The tie convention.  The reference's seed sort is a stable sort by count over HashMap iteration
 * order, which is randomly seeded: the order among equal counts -- and with it who survives
 * initial_vocab_size, every later stable sort and the final ids -- is random there.  Here: among
 * equal counts, ascending UTF-8 bytes.  Everything after the seed sort is deterministic.  In the
 * Viterbi search the reference replaces best[end] only when best[start] + score is greater, the
 * starts ascending, so among equal sums the smallest start (the longest token) wins; so here.
 *
 * The panic rule.  The trainer's backtrack (src/trainers.rs:533-536) indexes with `prev as usize`
 * unguarded: a position that nothing finite reaches (possible when initial_vocab_size drops a char
 * while "<unk>" is kept with count 0) panics.  Such a training returns CTOK_E_PANIC; the kernel sets
 * a flag and reads nothing out of bounds.  A training that fails, for this or any other reason,
 * leaves the trainer's vocab as it was before the call.
 *
 * Where ln runs.  score = ln(count / total) is evaluated on the host with libm's log (a count of 0
 * gives -inf); the device never evaluates a logarithm.  Each Viterbi candidate costs one f64 add
 * and one compare, never reassociated, so vocab order, scores and ids are a pure function of the
 * input bits.  After the first M-step most entries of a default-sized seed vocab have count 0 and
 * score -inf; they are live entries and stay in the vocab until a truncation drops them.
 *
 * The -inf quirk.  Model scores are any f64.  Where a -inf or NaN score lies on the only path to the
 * end of a text, nothing reaches it; the reference's backtrack (src/models.rs:261-265) then emits id 0
 * for that position and stops, so such a text encodes as [0].  Kept.
 * In the model a repeated vocab string keeps its last (id, score); id_to_token still answers for
 * every index; vocab_size counts distinct strings; unk_id is the unk token's id or 0;
 * min_score = min(0.0, every non-NaN score) - 10.0 scores a char that no vocab string covers.
 *
 * Bounds: a training keeps its sentences (< 4 GiB) and 4 * window bytes per char resident; the
 * window (max_piece_length, or the model's longest string in chars, capped by the strings the
 * table holds) is at most 4094 chars; more is CTOK_E_CAPACITY.  Counts are u64.
 *
 * Texts must be valid UTF-8 (kernels read no byte outside their buffers whatever the bytes are).
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU fallback: without a HIP device the calls return CTOK_E_DEVICE.  The handles are not
 * thread-safe.
 *
 * Environment: CTOK_TRAIN_CHUNK_BYTES (default here 16 MiB: a char gives up to max_piece_length
 * table entries) and CTOK_TRAIN_COUNT_SLOTS as for ctok_trainer_count.  A chunk whose count table
 * overflows is counted again with a larger one; a table that cannot be built within the cap is
 * CTOK_E_CAPACITY.
 */
#ifndef CTOK_UNIGRAM_H
#define CTOK_UNIGRAM_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"
#include "ctok_bpe_trainer.h" /* ctok_bpe_strings */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_uni_trainer ctok_uni_trainer;
typedef struct ctok_uni_model ctok_uni_model;

/* UnigramTrainerConfig (src/trainers.rs:287-326) as far as Python reaches it */
typedef struct ctok_uni_trainer_config {
  uint64_t vocab_size;         /* 8000 */
  /* special tokens: n_special UTF-8 strings, token i = special[special_off[i] .. special_off[i+1]) */
  const char* special;
  const uint64_t* special_off;
  uint64_t n_special;
  uint64_t initial_vocab_size; /* 1000000 */
  double shrinking_factor;     /* 0.75; any f64 */
  uint64_t n_iterations;       /* 16 */
  uint64_t max_piece_length;   /* 16, in chars */
  int device;                  /* HIP device */
} ctok_uni_trainer_config;

int ctok_uni_trainer_create(const ctok_uni_trainer_config* cfg, ctok_uni_trainer** out);
void ctok_uni_trainer_destroy(ctok_uni_trainer* tr);

/* train_from_texts (src/trainers.rs:374-387) of n_texts UTF-8 texts (text i = utf8[off[i] ..
 * off[i+1])): pretokenize, then train_from_sentences (:390-482) */
int ctok_uni_trainer_train(ctok_uni_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts);

/* train_from_sentences on sentences given directly (no normaliser, no split) */
int ctok_uni_trainer_train_sentences(ctok_uni_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_sentences);

uint64_t ctok_uni_trainer_vocab_size(const ctok_uni_trainer* tr); /* entries of the trainer's vocab */

/* The trainer's vocab in its order (string i has id i and score[i]).  Views are valid until the
 * trainer's next call or its destruction. */
int ctok_uni_trainer_result(ctok_uni_trainer* tr, ctok_bpe_strings* vocab, const double** score);

/* Debug (the parity tests read them), all of the last training:
 *   _sentences         the device's pretokenize output, in order
 *   _substring_counts  every substring with its count, before the specials and the truncation,
 *                      sorted by bytes
 *   _expected_counts   the last E-step: the vocab before that M-step, in its order, with the times
 *                      the Viterbi segmentations used each string (empty when no iteration ran) */
int ctok_uni_trainer_sentences(ctok_uni_trainer* tr, ctok_bpe_strings* sentences);
int ctok_uni_trainer_substring_counts(ctok_uni_trainer* tr, ctok_bpe_strings* strings, const uint64_t** count);
int ctok_uni_trainer_expected_counts(ctok_uni_trainer* tr, ctok_bpe_strings* strings, const uint64_t** count);

typedef struct ctok_uni_trainer_info {
  uint64_t sentences;
  uint64_t chars;             /* of all sentences */
  uint64_t seed_vocab;        /* entries after the seed sort and truncation */
  uint64_t iterations;        /* EM iterations run */
  const uint64_t* vocab_sizes; /* [iterations] the vocab's size after each; valid until the next call */
  uint64_t window;            /* token lengths (chars) the lattice holds */
  uint64_t table_capacity;    /* slots of the largest substring count table */
  uint64_t chunks;            /* of the counting: chunks, and chunks counted again with a larger table */
  uint64_t rerun_chunks;
  double ms_text;             /* HIP-event time of the Metaspace kernels and their scans */
  double ms_count;            /* ... of the substring counts and their drain */
  double ms_lattice;          /* ... of the char index and the lattice */
  double ms_viterbi;          /* ... of the Viterbi searches and backtracks, all iterations */
  double ms_host;             /* wall time of the whole call */
} ctok_uni_trainer_info;
int ctok_uni_trainer_stats(const ctok_uni_trainer* tr, ctok_uni_trainer_info* out);

/* UnigramModel::new (src/models.rs:201-222): n vocab strings (string i = bytes[off[i] .. off[i+1]),
 * repeats allowed) with their scores; the id of a string is its index.  unk_token: NUL-terminated. */
int ctok_uni_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const double* score, uint64_t n,
                          const char* unk_token, int device, ctok_uni_model** out);
void ctok_uni_model_destroy(ctok_uni_model* m);
uint64_t ctok_uni_model_vocab_size(const ctok_uni_model* m); /* distinct strings */

/* encode (src/models.rs:272-274) of n_texts host texts: text i gets ids[tok_off[i] .. tok_off[i+1]).
 * The arrays are valid until the model's next call or its destruction. */
int ctok_uni_model_encode_batch(ctok_uni_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                const uint32_t** ids, const uint64_t** tok_off);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_UNIGRAM_H */
