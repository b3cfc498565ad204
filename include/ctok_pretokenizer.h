/* ctok_pretokenizer.h -- C ABI of the pre-tokenizers on the GPU.
 *
 * A drop-in for the reference's `complexity_tokenizer.PreTokenizer` (Complexity-ML/complexity-tokenizer
 * v0.3.3, src/bindings/components.rs:89-173 over src/pretokenizers.rs:69-594): Whitespace,
 * WhitespaceSplit, ByteLevel, Metaspace, Punctuation, Digits, GPT2, BertPreTokenizer,
 * CharDelimiterSplit, UnicodeScripts, SplitWithBehavior and sequences of them.  A pre-tokenizer is a
 * program of steps; a run takes a packed batch (text i = utf8[off[i] .. off[i+1])) through all of
 * them on the device, every step over every word of the step before, and returns the words packed:
 * word j = words[word_off[j] .. word_off[j+1]), text i owns words text_word[i] .. text_word[i+1].
 *
 * A `split` pattern the Rust regex crate rejects is the identity, as in the reference; one it
 * compiles runs when it is a literal or one class atom with an optional '+' (csrc/pretok_prog.h),
 * and is CTOK_E_UNSUPPORTED otherwise, unless the step carries CTOK_PRETOK_REGEX: then a pattern of
 * literals, '.', those class atoms, concatenation, '|', groups and ? * + {n} {n,} {n,m} (greedy or
 * lazy) that cannot match the empty string runs as a DFA (csrc/regex_dfa.h), leftmost-first as the
 * crate matches.  Such a pattern with unbounded matches has a work bound: a word in which a match may
 * run past ctok_pretok_limits().max_regex_run code points makes the run CTOK_E_UNSUPPORTED, naming the
 * lowest-numbered such text, with nothing written.  A batch whose input, or the output of any step, reaches
 * 4 GiB is CTOK_E_CAPACITY, decided after the count and before any write.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU path: without a HIP device the calls return CTOK_E_DEVICE.  A handle keeps its grow-only device
 * buffers and is used by one thread at a time.
 */
#ifndef CTOK_PRETOKENIZER_H
#define CTOK_PRETOKENIZER_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_pretokenizer ctok_pretokenizer;

enum {
  CTOK_PRETOK_WHITESPACE = 0,
  CTOK_PRETOK_WHITESPACE_SPLIT = 1,
  CTOK_PRETOK_BYTE_LEVEL = 2,      /* flags & 1: add_prefix_space */
  CTOK_PRETOK_METASPACE = 3,       /* cp: the replacement; flags & 1: add_prefix_space */
  CTOK_PRETOK_PUNCTUATION = 4,
  CTOK_PRETOK_DIGITS = 5,          /* flags & 1: individual_digits */
  CTOK_PRETOK_GPT2 = 6,
  CTOK_PRETOK_BERT = 7,
  CTOK_PRETOK_CHAR_DELIMITER = 8,  /* cp: the delimiter */
  CTOK_PRETOK_UNICODE_SCRIPTS = 9,
  CTOK_PRETOK_SPLIT = 10           /* a: the pattern; flags & 7: CTOK_PRETOK_*; flags & 8: invert; flags & 16: regex */
};

/* SplitBehavior */
#define CTOK_PRETOK_REMOVED 0u
#define CTOK_PRETOK_ISOLATED 1u
#define CTOK_PRETOK_MERGED_WITH_PREVIOUS 2u
#define CTOK_PRETOK_MERGED_WITH_NEXT 3u
#define CTOK_PRETOK_CONTIGUOUS 4u
#define CTOK_PRETOK_INVERT 8u
/* On CTOK_PRETOK_SPLIT: a pattern that is neither a literal nor a class atom may run as a DFA.  A
 * literal or class atom keeps its path, and without the flag nothing changes. */
#define CTOK_PRETOK_REGEX 16u

#define CTOK_PRETOK_MAX_STEPS 1024

typedef struct ctok_pretok_step {
  uint32_t kind;
  uint32_t flags;
  const uint8_t* a; /* UTF-8, a_len bytes, may be NULL when a_len is 0 */
  uint64_t a_len;
  uint32_t cp;
} ctok_pretok_step;

/* A Sequence of n_steps steps (the strings are copied) for HIP device `device`. */
int ctok_pretokenizer_create(const ctok_pretok_step* steps, uint64_t n_steps, int device, ctok_pretokenizer** out);
void ctok_pretokenizer_destroy(ctok_pretokenizer* pt);

/* How a `split` pattern runs: 0 the Rust crate rejects it (the step is the identity), 1 a literal,
 * 2 a class atom, 3 unsupported.  Needs no device. */
int ctok_pretok_split_class(const uint8_t* pattern, uint64_t len);

/* How a `split` pattern runs under CTOK_PRETOK_REGEX: gate 0..3 as ctok_pretok_split_class says (3:
 * still refused, `reason` names the construct), 4 a DFA, with its sizes.  Needs no device. */
typedef struct ctok_pretok_split_info {
  int32_t gate;
  uint32_t n_symbols;     /* code-point classes of the DFA's alphabet */
  uint32_t n_states;      /* DFA states, the dead state not counted */
  uint32_t n_nfa;         /* NFA states after counted repetitions are expanded */
  uint32_t cyclic;        /* 1: a match can be unbounded, and max_regex_run applies */
  uint32_t table_in_lds;  /* 1: the kernels keep the transition table in LDS */
  uint64_t longest_match; /* code points, when not cyclic */
  uint64_t table_bytes;
  char reason[256];       /* gates 0 and 3: why; "" otherwise */
} ctok_pretok_split_info;
int ctok_pretok_split_plan(const uint8_t* pattern, uint64_t len, ctok_pretok_split_info* out);

/* The bounds of the DFA path.  max_regex_run: the code points one start of a cyclic DFA may step
 * through; CTOK_PRETOK_MAX_REGEX_RUN, read when a handle is created and by this call, lowers it. */
typedef struct ctok_pretok_limits_info {
  uint64_t max_regex_run;
  uint64_t max_symbols;
  uint64_t max_states;
  uint64_t max_nfa_states;
  uint64_t lds_table_bytes;  /* a transition table of at most this many bytes is kept in LDS */
  uint64_t scan_tile_bytes;  /* the bytes one wavefront covers in the prefix max of the matches' ends ... */
  uint64_t scan_round_bytes; /* ... and one round of the carry over the tiles */
} ctok_pretok_limits_info;
int ctok_pretok_limits(ctok_pretok_limits_info* out);

/* n_texts host texts through the program.  words has room for words_cap bytes, word_off for
 * word_cap + 1 offsets, text_word for n_texts + 1.  *n_bytes_out and *n_words_out receive the sizes
 * needed; when a capacity is too small the call is CTOK_E_CAPACITY and writes nothing else.
 * CTOK_E_ARG: a text is not UTF-8. */
int ctok_pretokenizer_run(ctok_pretokenizer* pt, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, uint8_t* words,
                          uint64_t words_cap, uint64_t* word_off, uint64_t word_cap, uint64_t* text_word,
                          uint64_t* n_bytes_out, uint64_t* n_words_out);

/* Same, with every buffer resident in the device's memory and the work ordered on `stream` (a
 * hipStream_t; NULL: the default stream); n_bytes = off[n_texts].  The bytes are taken as they are:
 * what is not well-formed UTF-8 passes through as units of one byte that are no whitespace,
 * punctuation, digit, letter or number and have the script Unknown; no byte outside the buffers is
 * read.  On CTOK_E_CAPACITY nothing is written to d_words, d_word_off or d_text_word.  The call
 * returns after the stream has finished the work. */
int ctok_pretokenizer_run_device(ctok_pretokenizer* pt, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_texts,
                                 uint64_t n_bytes, uint8_t* d_words, uint64_t words_cap, uint64_t* d_word_off,
                                 uint64_t word_cap, uint64_t* d_text_word, uint64_t* n_bytes_out, uint64_t* n_words_out,
                                 void* stream);

/* The stages of the program (its steps, then "gather"), and the HIP-event time of each in the last
 * run.  ms has room for cap values; *n receives the number of stages. */
int ctok_pretokenizer_stage_ms(const ctok_pretokenizer* pt, double* ms, uint64_t cap, uint64_t* n);
const char* ctok_pretokenizer_stage_name(const ctok_pretokenizer* pt, uint64_t i);

/* What the last run did: the steps that rewrote the text (ByteLevel, Metaspace; the others only
 * change the word bitmaps), the largest byte count any step produced, the words that came out. */
typedef struct ctok_pretokenizer_info {
  uint64_t steps;
  uint64_t steps_rewriting;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t bytes_peak;
  uint64_t words;
} ctok_pretokenizer_info;
int ctok_pretokenizer_stats(const ctok_pretokenizer* pt, ctok_pretokenizer_info* out);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_PRETOKENIZER_H */
