/* ctok_bpe_trainer.h -- C ABI of the classic frequency-BPE trainer on the GPU.
 *
 * Drop-in for the reference's PyO3 class `complexity_tokenizer.BpeTrainer`
 * (Complexity-ML/complexity-tokenizer v0.3.3, src/bindings/trainers.rs:218-279, registered at
 * src/lib.rs:53) over `BpeTrainer` (src/bpe_trainer.rs): the BPE of the original paper.  The
 * whitespace word split, the word counts, the pair counts, the search for the most frequent pair
 * and every merge's pass over the words run on the GPU; the pair counts stay on the device across
 * merges and are updated exactly, where the reference counts every pair again before every merge.
 * The host keeps the strings: symbols, vocabulary and merges.
 *
 * The reference leaves two orders to randomly seeded hash iteration; this library fixes them:
 *   - characters of equal total frequency enter the initial vocabulary in ascending code point
 *     order (build_initial_vocab's sort is by frequency only, src/bpe_trainer.rs:306-307);
 *   - among the pairs with the largest count, the one with the smallest (symbol id of first,
 *     symbol id of second) is merged (max_by_key over a HashMap, :152-155).
 * Symbol ids are dense: the characters in the order they are offered to the initial vocabulary
 * (total frequency descending, then code point ascending), then, when a continuing_subword_prefix
 * is set, the strings prefix + char of every char that follows another in a word, in ascending
 * code point order, then the merged strings in merge order.  Symbols are compared as strings, as
 * in the reference: a merged string that equals an existing symbol's string is that symbol.
 *
 * Pair counts are 64-bit here; the reference's are u32 (a panic in a debug build, a wrap in a
 * release build at 2^32).  No count after a merge exceeds the largest before it, so a training
 * whose first best count is >= 2^32 is refused with CTOK_E_ARG and every other one cannot overflow.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is
 * no CPU fallback: without a HIP device the counting and training calls return CTOK_E_DEVICE.
 * A ctok_bpe_trainer* is not thread-safe.
 *
 * Environment: CTOK_TRAIN_CHUNK_BYTES and CTOK_TRAIN_COUNT_SLOTS as for ctok_trainer_count;
 * CTOK_BPE_TRAIN_SLOTS caps the pair table's capacity; CTOK_BPE_TRAIN_RECOUNT=1 counts all pairs
 * again before every merge (the reference's literal algorithm, same results).
 */
#ifndef CTOK_BPE_TRAINER_H
#define CTOK_BPE_TRAINER_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_bpe_trainer ctok_bpe_trainer;

/* BpeTrainerConfig (src/bpe_trainer.rs:14-51) as far as Python reaches it
 * (src/bindings/trainers.rs:226-262: no initial_alphabet, no limit_alphabet). */
typedef struct ctok_bpe_trainer_config {
  uint64_t vocab_size;        /* 30000 */
  uint32_t min_frequency;     /* 2 */
  /* special tokens: n_special UTF-8 strings, token i = special[special_off[i] .. special_off[i+1]) */
  const char* special;
  const uint64_t* special_off;
  uint64_t n_special;
  /* NULL: none.  UTF-8, NUL-terminated. */
  const char* end_of_word_suffix;
  const char* continuing_subword_prefix;
  int show_progress;          /* accepted; nothing is printed per merge */
  int device;                 /* HIP device */
} ctok_bpe_trainer_config;

int ctok_bpe_trainer_create(const ctok_bpe_trainer_config* cfg, ctok_bpe_trainer** out);
void ctok_bpe_trainer_destroy(ctok_bpe_trainer* tr);

/* build_word_frequencies without the suffix: the words of n_texts UTF-8 texts (text i =
 * utf8[off[i] .. off[i+1])), each split on White_Space by itself, counted on the device.  The
 * counts replace those of the previous call; ctok_bpe_trainer_word_counts reads them. */
int ctok_bpe_trainer_count(ctok_bpe_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts);

/* BpeTrainer.train(texts)   src/bindings/trainers.rs:264-268 -> src/bpe_trainer.rs:100-228 */
int ctok_bpe_trainer_train(ctok_bpe_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts);

/* train on a word table given directly: word i = UTF-8 words[word_off[i] .. word_off[i+1]) with
 * frequency freqs[i] (the end_of_word_suffix is appended here too; equal words add up). */
int ctok_bpe_trainer_train_words(ctok_bpe_trainer* tr, const uint8_t* words, const uint64_t* word_off,
                                 const uint32_t* freqs, uint64_t n_words);

uint64_t ctok_bpe_trainer_vocab_size(const ctok_bpe_trainer* tr);   /* entries of the last training's vocab */
uint64_t ctok_bpe_trainer_num_merges(const ctok_bpe_trainer* tr);

/* n strings behind each other: string i = bytes[off[i] .. off[i+1]).  A view returned by the calls
 * below points into the trainer and is valid until the trainer's next call or its destruction. */
typedef struct ctok_bpe_strings {
  const uint8_t* bytes;
  const uint64_t* off;   /* n + 1 entries */
  uint64_t n;
} ctok_bpe_strings;

/* The last training's result: the vocab (string i has id vocab_id[i]; sorted by string) and the
 * merges in order (merge i = strings 2i and 2i + 1 of *merges). */
int ctok_bpe_trainer_result(ctok_bpe_trainer* tr, ctok_bpe_strings* vocab, const uint32_t** vocab_id,
                            ctok_bpe_strings* merges);

/* The current word counts (ctok_bpe_trainer_count, or the last ctok_bpe_trainer_train before the
 * suffix), sorted by word: word i has count freqs[i]. */
int ctok_bpe_trainer_word_counts(ctok_bpe_trainer* tr, ctok_bpe_strings* words, const uint32_t** freqs);

typedef struct ctok_bpe_trainer_info {
  uint64_t words;            /* sum of the word counts trained on */
  uint64_t unique_words;
  uint64_t initial_symbols;  /* symbol ids handed out before the first merge */
  uint64_t merges;
  uint64_t table_capacity;   /* slots of the pair table at the end */
  uint64_t rebuilds;         /* pair counts made again from the words, after the initial count */
  uint64_t chunks;           /* of the last counting: chunks, chunks counted by the host walk, */
  uint64_t host_chunks;      /*   chunks counted a second time with a larger table */
  uint64_t rerun_chunks;
  double ms_count;           /* HIP-event time of the split, counting and drain kernels */
  double ms_pairs;           /* ... of the pair counts (initial and rebuilds) */
  double ms_best;            /* ... of the searches for the best pair */
  double ms_merges;          /* ... of the merge passes */
  double ms_host;            /* wall time of the training, after the counting */
} ctok_bpe_trainer_info;
int ctok_bpe_trainer_stats(const ctok_bpe_trainer* tr, ctok_bpe_trainer_info* out);

/* The symbol strings by symbol id (see above). */
int ctok_bpe_trainer_symbols(ctok_bpe_trainer* tr, ctok_bpe_strings* symbols);

/* Debug: a copy of the live pair table after the last training, in no particular order: entry i is
 * the pair of symbol ids (a[i], b[i]) with count[i]; entries whose count fell to 0 are included.
 * The arrays are valid like a view. */
int ctok_bpe_trainer_pair_counts(ctok_bpe_trainer* tr, const uint32_t** a, const uint32_t** b, const int64_t** count,
                                 uint64_t* n);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_BPE_TRAINER_H */
