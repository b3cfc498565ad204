/* C ABI of the three stand-alone models WordLevelModel, CharBpeModel and ByteLevelBpeModel
 * (reference Complexity-ML/complexity-tokenizer v0.3.3, src/models.rs:300-741,
 * src/bindings/models.rs:89-214).  With the WordPiece model of ctok_wordpiece.h and the Unigram
 * model of ctok_unigram.h they complete the reference's `models` surface.
 *
 * Common to all three: unk_id = vocab.get(unk_token), else 0; no normaliser runs; vocab_size is the
 * number of vocab strings.
 *
 *   WordLevelModel (:316-362)     every split_whitespace word -> vocab.get(word), else unk_id
 *   CharBpeModel (:612-741)       per split_whitespace word: one token per char, the last one
 *                                 char + end_of_word_suffix (which may be empty); the merge loop;
 *                                 every final token -> vocab.get(token), else unk_id
 *   ByteLevelBpeModel (:421-589)  add_prefix_space: a text that does not start with U+0020 (the
 *                                 empty text too) gets one in front.  A word starts at byte 0 and at
 *                                 every U+0020 ("a  b" = "a", " ", " b"; tabs, newlines and NBSP stay
 *                                 inside words); one GPT-2 byte-map char per byte; the merge loop;
 *                                 the same final lookup
 *   split_whitespace              the 25 White_Space code points (csrc/ws_split_hd.h)
 *
 * The merge loop (:487-514, :662-689): rank[(a, b)] = the pair's index in `merges`, a later
 * duplicate of a pair overwrites it.  Every step scans all adjacent pairs, takes the smallest rank
 * (the leftmost of equals) and replaces that one pair by the string a + b, until no pair has a
 * rank.  Tokens are strings: a merge's parts and its result need not be vocab entries, and a
 * token outside the vocab becomes unk_id only at the very end.  The kernels (csrc/strmerge.hip) run
 * this loop as it stands, one merge per step, keyed on interned strings (csrc/strmerge_compile.h).
 *
 * Orders the reference leaves to hash iteration, fixed here: among vocab strings that share an id,
 * id_to_token and decode use the smallest string by UTF-8 bytes, as ctok_wp_model does.  (decode is
 * host string work in the Python layer.)
 *
 * The one deliberate difference from the reference: the loop is quadratic in a word's length and a
 * byte-level text without a space is one word, so a word of more than the cap of
 * ctok_models_limits symbols makes encode return CTOK_E_UNSUPPORTED, with the word's length in the
 * message, before any merge kernel is launched.  The environment variable
 * CTOK_MODELS_MAX_WORD_SYMBOLS lowers the cap; nothing raises it.
 *
 * Limits: a batch below 4 GiB (CTOK_E_CAPACITY), at most 2^24 merges and fewer than 2^31 distinct
 * token strings (CTOK_E_UNSUPPORTED).  Errors are the CTOK_E_* codes of ctok.h: CTOK_E_DEVICE
 * without a HIP device, CTOK_E_ARG for a vocab string given twice, an odd merge array or strings
 * that are not UTF-8.  There is no CPU path.  A model is used by one thread at a time. */
#ifndef CTOK_MODELS_H
#define CTOK_MODELS_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_sm_model ctok_sm_model; /* the three models share one engine */
typedef ctok_sm_model ctok_wl_model;
typedef ctok_sm_model ctok_cbpe_model;
typedef ctok_sm_model ctok_blbpe_model;

/* The vocab: n_vocab distinct strings (string i = vocab_bytes[vocab_off[i] .. vocab_off[i+1])) with
 * their ids.  The merges: n_merge_strings = 2 * merges strings, merge r = (string 2r, string 2r+1).
 * unk_token and end_of_word_suffix are NUL-terminated UTF-8.  The tables go to `device` here. */
int ctok_wl_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                         uint64_t n_vocab, const char* unk_token, int device, ctok_wl_model** out);
int ctok_cbpe_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                           uint64_t n_vocab, const uint8_t* merge_bytes, const uint64_t* merge_off,
                           uint64_t n_merge_strings, const char* end_of_word_suffix, const char* unk_token,
                           int device, ctok_cbpe_model** out);
int ctok_blbpe_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                            uint64_t n_vocab, const uint8_t* merge_bytes, const uint64_t* merge_off,
                            uint64_t n_merge_strings, const char* unk_token, int add_prefix_space, int device,
                            ctok_blbpe_model** out);

void ctok_wl_model_destroy(ctok_wl_model* m);
void ctok_cbpe_model_destroy(ctok_cbpe_model* m);
void ctok_blbpe_model_destroy(ctok_blbpe_model* m);
uint64_t ctok_wl_model_vocab_size(const ctok_wl_model* m);
uint64_t ctok_cbpe_model_vocab_size(const ctok_cbpe_model* m);
uint64_t ctok_blbpe_model_vocab_size(const ctok_blbpe_model* m);

/* encode of n_texts host texts: text i gets ids[tok_off[i] .. tok_off[i+1]).  The arrays are valid
 * until the model's next call or its destruction. */
int ctok_wl_model_encode_batch(ctok_wl_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                               const uint32_t** ids, const uint64_t** tok_off);
int ctok_cbpe_model_encode_batch(ctok_cbpe_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                 const uint32_t** ids, const uint64_t** tok_off);
int ctok_blbpe_model_encode_batch(ctok_blbpe_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                  const uint32_t** ids, const uint64_t** tok_off);

/* The engine's tiers: a word of up to *tier1 symbols is merged by one thread, of up to *tier2 by
 * one wavefront in LDS, a longer one by a wavefront in global memory; *max_word_symbols is the cap
 * above (after the environment variable). */
void ctok_models_limits(uint32_t* tier1, uint32_t* tier2, uint64_t* max_word_symbols);

/* Diagnostic: HIP-event times of the model's last encode call in ms -- out[0] start bits, [1] the
 * word list, [2] initial symbols and merges, [3] emit. */
#define CTOK_MODELS_STAGES 4
int ctok_models_stage_ms(const ctok_sm_model* m, double out[CTOK_MODELS_STAGES]);

#ifdef __cplusplus
}
#endif
#endif
