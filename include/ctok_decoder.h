/* ctok_decoder.h -- C ABI of the decoders on the GPU.
 *
 * A drop-in for the reference's `complexity_tokenizer.Decoder` (Complexity-ML/complexity-tokenizer
 * v0.3.3, src/bindings/components.rs:231-292 over src/decoders.rs:30-243): ByteLevel, Metaspace,
 * WordPiece, BPE, CTC, Fuse, Strip, and Replace and sequences of them, which the reference's enum has.
 * A decoder is a program of steps; a run takes a packed batch of tokens (token j =
 * tokens[tok_off[j] .. tok_off[j+1]), document i owns tokens doc_tok[i] .. doc_tok[i+1]) through all
 * of them on the device and returns the texts packed: text i = text[text_off[i] .. text_off[i+1]).
 * After a step every document is one token, so a step after the first sees its document's text.
 *
 * A batch whose input, or the output of any step, reaches 4 GiB, or that has 2^32 tokens, is
 * CTOK_E_CAPACITY, decided after the count and before any write.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU path: without a HIP device the calls return CTOK_E_DEVICE.  A handle keeps its grow-only device
 * buffers and is used by one thread at a time.
 */
#ifndef CTOK_DECODER_H
#define CTOK_DECODER_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_decoder ctok_decoder;

enum {
  CTOK_DEC_BYTE_LEVEL = 0,
  CTOK_DEC_METASPACE = 1, /* cp: the replacement; flags & 1: add_prefix_space */
  CTOK_DEC_WORDPIECE = 2, /* a: the prefix; flags & 1: cleanup */
  CTOK_DEC_BPE = 3,       /* a: the suffix */
  CTOK_DEC_CTC = 4,       /* a: the pad token; b: the word delimiter token when flags & 1 */
  CTOK_DEC_FUSE = 5,
  CTOK_DEC_STRIP = 6,     /* cp: the content; start, stop */
  CTOK_DEC_REPLACE = 7    /* a: the literal pattern; b: the replacement */
};

#define CTOK_DEC_MAX_STEPS 1024
/* ids of a vocabulary lie below this */
#define CTOK_DEC_MAX_ID (1u << 27)
/* the length that says "no entry" in ctok_decoder_set_vocab */
#define CTOK_DEC_NO_ENTRY 0xFFFFFFFFu

typedef struct ctok_dec_step {
  uint32_t kind;
  uint32_t flags;
  const uint8_t* a; /* UTF-8, a_len bytes, may be NULL when a_len is 0 */
  uint64_t a_len;
  const uint8_t* b;
  uint64_t b_len;
  uint32_t cp;
  uint64_t start;
  uint64_t stop;
} ctok_dec_step;

/* A Sequence of n_steps steps (the strings are copied) for HIP device `device`; the empty Sequence is
 * Fuse. */
int ctok_decoder_create(const ctok_dec_step* steps, uint64_t n_steps, int device, ctok_decoder** out);
void ctok_decoder_destroy(ctok_decoder* dc);

/* The id -> token table of the ids entry: id i is pool[ent_off[i] .. ent_off[i] + ent_len[i]), or has
 * no entry when ent_len[i] is CTOK_DEC_NO_ENTRY.  Uploaded once per call.  CTOK_E_CAPACITY: n_ent is
 * above CTOK_DEC_MAX_ID or the pool reaches 4 GiB; CTOK_E_ARG: an entry is not UTF-8. */
int ctok_decoder_set_vocab(ctok_decoder* dc, const uint8_t* pool, uint64_t pool_len, const uint32_t* ent_off,
                           const uint32_t* ent_len, uint64_t n_ent);

/* n_docs host documents through the program.  text has room for text_cap bytes, text_off for
 * n_docs + 1 offsets.  *n_bytes_out receives the size needed; when text_cap is too small the call is
 * CTOK_E_CAPACITY and writes nothing else.  CTOK_E_ARG: a token is not UTF-8, or the offsets are not
 * in order. */
int ctok_decoder_run(ctok_decoder* dc, const uint8_t* tokens, const uint64_t* tok_off, const uint64_t* doc_tok,
                     uint64_t n_docs, uint8_t* text, uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out);

/* The same from ids: document i owns ids[ids_off[i] .. ids_off[i+1]); an id without an entry is
 * skipped.  CTOK_E_ARG without a vocabulary. */
int ctok_decoder_run_ids(ctok_decoder* dc, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, uint8_t* text,
                         uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out);

/* The texts of the last ctok_decoder_run or ctok_decoder_run_ids again, which the handle keeps on the device until
 * its next run: for a caller whose text_cap was too small, without running the program a second time.  text_off has
 * room for that run's n_docs + 1 offsets.  CTOK_E_CAPACITY as there; CTOK_E_ARG: there is no such result. */
int ctok_decoder_fetch(ctok_decoder* dc, uint8_t* text, uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out);

/* ctok_decoder_run with every buffer resident in the device's memory and the work ordered on `stream`
 * (a hipStream_t; NULL: the default stream); n_tok = doc_tok[n_docs], n_bytes = tok_off[n_tok].  The
 * bytes are taken as they are: what is not well-formed UTF-8 is a unit of one byte that no rule's
 * string matches; no byte outside the buffers is read.  On CTOK_E_CAPACITY nothing is written to
 * d_text or d_text_off.  The call returns after the stream has finished the work. */
int ctok_decoder_run_device(ctok_decoder* dc, const uint8_t* d_tokens, const uint64_t* d_tok_off, const uint64_t* d_doc_tok,
                            uint64_t n_docs, uint64_t n_tok, uint64_t n_bytes, uint8_t* d_text, uint64_t text_cap,
                            uint64_t* d_text_off, uint64_t* n_bytes_out, void* stream);

/* The stages of the program ("gather", which only the ids entry runs, then its steps), and the
 * HIP-event time of each in the last run.  ms has room for cap values; *n receives the number of
 * stages. */
int ctok_decoder_stage_ms(const ctok_decoder* dc, double* ms, uint64_t cap, uint64_t* n);
const char* ctok_decoder_stage_name(const ctok_decoder* dc, uint64_t i);

/* What the last run did: the passes (count, scan, write) its steps took, the tokens that went in
 * (after the gather dropped the ids without an entry), the largest byte count any pass produced. */
typedef struct ctok_decoder_info {
  uint64_t steps;
  uint64_t passes;
  uint64_t docs;
  uint64_t tokens;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t bytes_peak;
} ctok_decoder_info;
int ctok_decoder_stats(const ctok_decoder* dc, ctok_decoder_info* out);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_DECODER_H */
