/* ctok_normalizer.h -- C ABI of the text normalisers on the GPU.
 *
 * A drop-in for the reference's `complexity_tokenizer.Normalizer` (Complexity-ML/complexity-tokenizer
 * v0.3.3, src/bindings/components.rs:15-87 over src/normalizers.rs:43-202): NFC, NFD, NFKC, NFKD
 * (UAX #15 with the Unicode 13.0 data of csrc/gen/normalize_data.h; no stream-safe cut-off),
 * Lowercase (str::to_lowercase), Strip (str::trim), StripAccents (NFD, then the five ranges of
 * is_combining_mark dropped), Replace (str::replace with a literal pattern), Prepend, Append,
 * BertNormalizer and Precompiled, and sequences of them.  A normaliser is a program of steps; a run
 * takes a packed batch (text i = utf8[off[i] .. off[i+1])) through all of them on the device.  Only a
 * text's own bytes decide its result.
 *
 * Every step counts its output before it writes it, so no expansion is assumed.  Two refusals the
 * reference does not have: a batch whose input, or the output of any step, reaches 4 GiB is
 * CTOK_E_CAPACITY (decided after the count, before any write), and a program of more than
 * CTOK_NORM_MAX_STEPS primitive steps is CTOK_E_UNSUPPORTED.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU path: without a HIP device the calls return CTOK_E_DEVICE.  A handle keeps its grow-only device
 * buffers and is used by one thread at a time.
 */
#ifndef CTOK_NORMALIZER_H
#define CTOK_NORMALIZER_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_normalizer ctok_normalizer;

enum {
  CTOK_NORM_NFC = 0,
  CTOK_NORM_NFD = 1,
  CTOK_NORM_NFKC = 2,
  CTOK_NORM_NFKD = 3,
  CTOK_NORM_LOWERCASE = 4,
  CTOK_NORM_STRIP = 5,
  CTOK_NORM_STRIP_ACCENTS = 6,
  CTOK_NORM_REPLACE = 7,     /* a: the pattern (may be empty), b: the replacement */
  CTOK_NORM_PREPEND = 8,     /* a: the string */
  CTOK_NORM_APPEND = 9,      /* a: the string */
  CTOK_NORM_BERT = 10,       /* flags: CTOK_NORM_BERT_* */
  CTOK_NORM_PRECOMPILED = 11 /* a: the charsmap, per entry u32 from_len, u32 to_len (little endian), from, to */
};

/* BertNormalizer{clean_text, handle_chinese_chars, strip_accents: Option<bool>, lowercase} */
#define CTOK_NORM_BERT_CLEAN_TEXT 1u
#define CTOK_NORM_BERT_CHINESE 2u
#define CTOK_NORM_BERT_LOWERCASE 4u
#define CTOK_NORM_BERT_STRIP_ACCENTS_FALSE 8u /* neither bit: None, i.e. what lowercase is */
#define CTOK_NORM_BERT_STRIP_ACCENTS_TRUE 16u

/* primitive steps (a decomposition, the canonical ordering, a Replace, ...) a program may have
 * after Bert, Precompiled and the normal forms are expanded */
#define CTOK_NORM_MAX_STEPS 1024

typedef struct ctok_norm_step {
  uint32_t kind;
  uint32_t flags;
  const uint8_t* a; /* UTF-8, a_len bytes, may be NULL when a_len is 0 */
  uint64_t a_len;
  const uint8_t* b;
  uint64_t b_len;
} ctok_norm_step;

/* A Sequence of n_steps steps (the strings are copied) for HIP device `device`. */
int ctok_normalizer_create(const ctok_norm_step* steps, uint64_t n_steps, int device, ctok_normalizer** out);
void ctok_normalizer_destroy(ctok_normalizer* nz);

/* n_texts host texts through the program.  out has room for out_cap bytes, out_off for n_texts + 1
 * offsets.  out_cap too small -> CTOK_E_CAPACITY with out_off filled (out_off[n_texts] = bytes
 * needed) and out untouched.  CTOK_E_ARG: a text is not UTF-8. */
int ctok_normalizer_run(ctok_normalizer* nz, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_off);

/* Same, with utf8 / off / out / out_off resident in the device's memory and the work ordered on
 * `stream` (a hipStream_t; NULL: the default stream); n_bytes = off[n_texts].  The bytes are taken
 * as they are: what is not well-formed UTF-8 passes through as raw bytes, and no byte outside the
 * buffers is read.  *n_bytes_out receives the output size, also on CTOK_E_CAPACITY, when out_cap is
 * too small and nothing is written.  The call returns after the stream has finished the work. */
int ctok_normalizer_run_device(ctok_normalizer* nz, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_texts,
                               uint64_t n_bytes, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                               uint64_t* n_bytes_out, void* stream);

/* The primitive steps of the program, and the HIP-event time of each in the last run (0 for a step
 * that did not run: an empty batch).  ms has room for cap values; *n receives the number of steps. */
int ctok_normalizer_stage_ms(const ctok_normalizer* nz, double* ms, uint64_t cap, uint64_t* n);
/* the name of primitive step i ("decompose", "reorder", "compose", "lowercase", "replace", ...); "" past the end */
const char* ctok_normalizer_stage_name(const ctok_normalizer* nz, uint64_t i);

/* What the last run did: primitive steps that changed the text (the others are not copied), and
 * the largest byte count any step produced. */
typedef struct ctok_normalizer_info {
  uint64_t steps;
  uint64_t steps_changed;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t bytes_peak;
} ctok_normalizer_info;
int ctok_normalizer_stats(const ctok_normalizer* nz, ctok_normalizer_info* out);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_NORMALIZER_H */
