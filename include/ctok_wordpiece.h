/* ctok_wordpiece.h -- C ABI of the WordPiece trainer and model on the GPU.
 *
 * Drop-ins for the reference's PyO3 classes `complexity_tokenizer.WordPieceTrainer` and
 * `complexity_tokenizer.WordPieceModel` (Complexity-ML/complexity-tokenizer v0.3.3,
 * src/bindings/trainers.rs:94-153 over src/trainers.rs:64-279, src/bindings/models.rs:8-49 over
 * src/models.rs:17-142).
 *
 * The trainer's normaliser is Sequence[NFC, Lowercase] and its pre-tokenizer str::split_whitespace;
 * neither can be changed.  NFC, Lowercase (str::to_lowercase, csrc/lowercase_hd.h), the split, the
 * word counts, the greedy longest match of every word, the pair counts and the search for the most
 * frequent pair run on the GPU.  The reference tokenises every word against the whole vocab before
 * every merge; here every byte of the unique words keeps its longest match on the device, a round
 * compares the one new string against them (the vocab only grows, so a match only grows), and only
 * words whose matches changed are walked again.  The host keeps the strings.
 *
 * A vocab string V gives two patterns: V itself, valid at a word's first char, and V without the
 * continuing-subword prefix, valid at any later char, when V starts with the prefix and something
 * is left.  With an empty prefix both patterns are V.
 *
 * The reference leaves three orders to randomly seeded hash iteration; this library fixes them:
 *   - the chars of the kept words enter the vocab in ascending code point order;
 *   - among the pairs with the largest count, the one with the smallest (key(a), key(b)) is merged.
 *     key(t) is the vocab id of t when t is a key; otherwise t is prefix + char and key(t) = 2^31 +
 *     code point.  Vocab ids >= 2^31 are refused with CTOK_E_ARG.  A trainer that trains a second
 *     time keeps its vocab and hands ids out from 0 again (the reference's behaviour), so two keys
 *     can then share an id: keys are given at the start of a training to the vocab strings in
 *     (id, UTF-8 bytes) order and after that to every merged string, and a string whose id an
 *     earlier string already holds takes the next free value from 2^31 + 0x110000 up instead;
 *   - in the model, among vocab strings that share an id, id_to_token and decode use the smallest
 *     string by UTF-8 bytes.
 *
 * The merged string of a round can never be a key already (greedy matching would have taken it
 * instead of its first half); if it is, the training returns CTOK_E_ARG where the reference would
 * loop forever.  A training that fails leaves the trainer's vocab as it was before the call.
 * Pair counts are 64-bit here and u32 in the reference: a best count >= 2^32 is CTOK_E_ARG.  There is no min_frequency test on pairs, only on words.
 *
 * Texts must be valid UTF-8 (kernels read no byte outside their buffers whatever the bytes are).
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU fallback: without a HIP device the calls return CTOK_E_DEVICE.  The handles are not
 * thread-safe.
 *
 * Environment: CTOK_TRAIN_CHUNK_BYTES and CTOK_TRAIN_COUNT_SLOTS as for ctok_trainer_count;
 * CTOK_BPE_TRAIN_SLOTS caps the pair table's capacity as for the BPE trainer;
 * CTOK_WP_TRAIN_RECOUNT=1 walks every word and counts all pairs again in every round (the
 * reference's literal recount on the same kernels, same results).
 */
#ifndef CTOK_WORDPIECE_H
#define CTOK_WORDPIECE_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"
#include "ctok_bpe_trainer.h" /* ctok_bpe_strings */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_wp_trainer ctok_wp_trainer;
typedef struct ctok_wp_model ctok_wp_model;

/* WordPieceTrainerConfig (src/trainers.rs:19-61) as far as Python reaches it */
typedef struct ctok_wp_trainer_config {
  uint64_t vocab_size;               /* 30000 */
  uint32_t min_frequency;            /* 2: words counted less often are dropped */
  /* special tokens: n_special UTF-8 strings, token i = special[special_off[i] .. special_off[i+1]) */
  const char* special;
  const uint64_t* special_off;
  uint64_t n_special;
  const char* continuing_subword_prefix; /* "##"; UTF-8, NUL-terminated, may be empty, not NULL */
  uint64_t max_input_chars_per_word; /* 100: handed to the model */
  int device;                        /* HIP device */
} ctok_wp_trainer_config;

int ctok_wp_trainer_create(const ctok_wp_trainer_config* cfg, ctok_wp_trainer** out);
void ctok_wp_trainer_destroy(ctok_wp_trainer* tr);

/* The word counts of n_texts UTF-8 texts (text i = utf8[off[i] .. off[i+1])): each text through
 * NFC and Lowercase, split on White_Space by itself, counted on the device.  The counts replace
 * those of the previous call; ctok_wp_trainer_word_counts reads them. */
int ctok_wp_trainer_count(ctok_wp_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts);

/* train_from_texts (src/trainers.rs:112-127): count, then train_from_word_freqs (:130-225) */
int ctok_wp_trainer_train(ctok_wp_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts);

/* train_from_word_freqs on a word table given directly: word i = UTF-8 words[word_off[i] ..
 * word_off[i+1]) with frequency freqs[i] (equal words add up; no normaliser runs). */
int ctok_wp_trainer_train_words(ctok_wp_trainer* tr, const uint8_t* words, const uint64_t* word_off,
                                const uint32_t* freqs, uint64_t n_words);

uint64_t ctok_wp_trainer_vocab_size(const ctok_wp_trainer* tr); /* entries of the trainer's vocab */

/* The trainer's vocab (string i has id vocab_id[i]; sorted by string) and the last training's
 * merges in order (merge i = strings 2i and 2i + 1 of *merges: the tokens a and b).  Views are
 * valid until the trainer's next call or its destruction. */
int ctok_wp_trainer_result(ctok_wp_trainer* tr, ctok_bpe_strings* vocab, const uint32_t** vocab_id,
                           ctok_bpe_strings* merges);

/* The current word counts, sorted by word: word i has count freqs[i]. */
int ctok_wp_trainer_word_counts(ctok_wp_trainer* tr, ctok_bpe_strings* words, const uint32_t** freqs);

/* Debug (the parity tests read it): the last training's words (sorted) with their final tokens:
 * word i has the strings tok_off[i] .. tok_off[i+1] of *tokens, read back from the device. */
int ctok_wp_trainer_tokens(ctok_wp_trainer* tr, ctok_bpe_strings* words, ctok_bpe_strings* tokens,
                           const uint64_t** tok_off);

typedef struct ctok_wp_trainer_info {
  uint64_t words;            /* sum of the word counts trained on */
  uint64_t unique_words;
  uint64_t initial_vocab;    /* vocab entries before the first round */
  uint64_t merges;
  uint64_t table_capacity;   /* slots of the pair table at the end */
  uint64_t rebuilds;         /* pair counts made again from the words, after the initial count */
  uint64_t walked_words;     /* words walked again, all rounds */
  uint64_t chunks;           /* of the last counting: chunks, chunks counted by the host walk, */
  uint64_t host_chunks;      /*   chunks counted a second time with a larger table, */
  uint64_t rerun_chunks;
  uint64_t lowered_chunks;   /*   chunks Lowercase changed (the others are not copied) */
  double ms_count;           /* HIP-event time of lowercase, split, counting and drain */
  double ms_match;           /* ... of the initial match of every position */
  double ms_pairs;           /* ... of the pair counts (initial and rebuilds) */
  double ms_add;             /* ... of the rounds' k_wp_add */
  double ms_walk;            /* ... of the rounds' k_wp_walk */
  double ms_best;            /* ... of the searches for the best pair */
  double ms_host;            /* wall time of the training, after the counting */
} ctok_wp_trainer_info;
int ctok_wp_trainer_stats(const ctok_wp_trainer* tr, ctok_wp_trainer_info* out);

/* Debug: the live pair table after the last training, in no particular order: pair i is (string i
 * of *first, string i of *second) with count[i]; pairs whose count fell to 0 are left out. */
int ctok_wp_trainer_pair_counts(ctok_wp_trainer* tr, ctok_bpe_strings* first, ctok_bpe_strings* second,
                                const int64_t** count);

/* WordPieceModel::new (src/models.rs:32-49): n vocab strings (string i = bytes[off[i] ..
 * off[i+1]), distinct) with ids, the prefix and the unk token (NUL-terminated UTF-8). */
int ctok_wp_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id, uint64_t n,
                         const char* continuing_subword_prefix, const char* unk_token,
                         uint64_t max_input_chars_per_word, int device, ctok_wp_model** out);
void ctok_wp_model_destroy(ctok_wp_model* m);
uint64_t ctok_wp_model_vocab_size(const ctok_wp_model* m);

/* encode (src/models.rs:98-106) of n_texts host texts: text i gets ids[tok_off[i] .. tok_off[i+1]).
 * The arrays are valid until the model's next call or its destruction. */
int ctok_wp_model_encode_batch(ctok_wp_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                               const uint32_t** ids, const uint64_t** tok_off);

/* For tests: str::to_lowercase of every text on the device.  out has room for out_cap bytes (3/2
 * of the input always suffices), out_off for n_texts + 1 offsets.  CTOK_E_ARG: not UTF-8. */
int ctok_lowercase(const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, int device, uint8_t* out,
                   uint64_t out_cap, uint64_t* out_off);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_WORDPIECE_H */
