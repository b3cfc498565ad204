/* ctok_postprocessor.h -- C ABI of the post-processors on the GPU.
 *
 * A drop-in for the reference's `complexity_tokenizer.PostProcessor` (Complexity-ML/complexity-tokenizer
 * v0.3.3, src/bindings/components.rs:175-229 over src/postprocessors.rs:34-280): TemplateProcessing,
 * BertProcessing, RobertaProcessing and sequences of them, with the free functions truncate and pad.
 * A post-processor is a program of steps, compiled once at create into two flat lists of items -- one
 * for rows without a pair, one for rows with a pair -- of which each item copies the row's first
 * sequence (A), its pair (B) or inserts one id (SPECIAL).  A run takes a packed batch (row i owns
 * ids[off[i] .. off[i+1]) and, when has_pair says so, pair_ids[pair_off[i] .. pair_off[i+1])) through
 * truncate, the program and pad on the device, and returns the rows ragged (ids and offsets) or as
 * [n_rows, width] matrices with their masks.
 *
 * A batch whose input or output reaches 2^32 ids, or that has 2^32 rows, is CTOK_E_CAPACITY, decided
 * after the count and before any write.
 *
 * Errors: 0 or a negative CTOK_E_* code (ctok.h), ctok_last_error() holds the message.  There is no
 * CPU path: without a HIP device the calls return CTOK_E_DEVICE.  A handle keeps its grow-only device
 * buffers and is used by one thread at a time.
 */
#ifndef CTOK_POSTPROCESSOR_H
#define CTOK_POSTPROCESSOR_H

#include <stddef.h>
#include <stdint.h>

#include "ctok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctok_postprocessor ctok_postprocessor;

enum {
  CTOK_PP_TEMPLATE = 0, /* single, pair (when flags & 1), the special tokens */
  CTOK_PP_BERT = 1,     /* id_a: cls, id_b: sep */
  CTOK_PP_ROBERTA = 2   /* id_a: bos, id_b: eos */
};

enum { CTOK_PP_ONLY_FIRST = 0, CTOK_PP_ONLY_SECOND = 1, CTOK_PP_LONGEST_FIRST = 2 };

#define CTOK_PP_MAX_STEPS 1024
/* the items of a compiled list; a program that needs more is refused at create */
#define CTOK_PP_MAX_ITEMS 4096

typedef struct ctok_pp_step {
  uint32_t kind;
  uint32_t flags;        /* CTOK_PP_TEMPLATE: & 1: there is a pair template */
  const uint8_t* single; /* UTF-8, single_len bytes, may be NULL when single_len is 0 */
  uint64_t single_len;
  const uint8_t* pair;
  uint64_t pair_len;
  /* the special tokens of a template: token t is tok_bytes[tok_off[t] .. tok_off[t+1]) with id tok_id[t];
   * the first equal string wins */
  const uint8_t* tok_bytes;
  const uint64_t* tok_off; /* n_tok + 1, may be NULL when n_tok is 0 */
  const uint32_t* tok_id;
  uint64_t n_tok;
  uint32_t id_a;
  uint32_t id_b;
} ctok_pp_step;

/* A Sequence of n_steps steps (everything is copied) for HIP device `device`: the pair goes to the
 * first step only, every later one sees the result so far alone; the empty Sequence returns the ids
 * and drops the pair.  CTOK_E_CAPACITY: a flat list would have more than CTOK_PP_MAX_ITEMS items (the
 * message holds the count); CTOK_E_UNSUPPORTED: more than CTOK_PP_MAX_STEPS steps; CTOK_E_ARG: no
 * such kind, or a string that is not UTF-8. */
int ctok_postprocessor_create(const ctok_pp_step* steps, uint64_t n_steps, int device, ctok_postprocessor** out);
void ctok_postprocessor_destroy(ctok_postprocessor* pp);

/* A packed batch.  pair_ids / pair_off may be NULL: no row has a pair.  has_pair (a byte per row, 0
 * or not) may be NULL: every row has a pair when pair_off is given.  The pair range of a row without
 * a pair is ignored. */
typedef struct ctok_pp_batch {
  const uint32_t* ids;
  const uint64_t* off; /* n_rows + 1 */
  const uint32_t* pair_ids;
  const uint64_t* pair_off; /* n_rows + 1 */
  const uint8_t* has_pair;  /* n_rows */
  uint64_t n_rows;
} ctok_pp_batch;

/* Truncate (postprocessors.rs:209-254) before the program and pad (:266-280) after it. */
typedef struct ctok_pp_opts {
  uint32_t truncate;    /* 0: none */
  uint32_t strategy;    /* CTOK_PP_ONLY_FIRST .. CTOK_PP_LONGEST_FIRST */
  uint64_t truncate_to; /* bounds len(ids) + len(pair) of the input, not the processed row */
  uint32_t padded;      /* 0: ragged output; 1: [n_rows, width] matrices */
  uint32_t pad_left;
  uint64_t pad_to;      /* width = max(longest processed row, pad_to) */
  uint32_t pad_id;
  uint32_t reserved;
} ctok_pp_opts;

/* Where a host run's result goes.  Ragged: ids (ids_cap ids) and off (n_rows + 1).  Padded: ids,
 * attention_mask, token_type_ids and special_tokens_mask of ids_cap cells each, of which
 * n_rows * width are written, and row_len (n_rows).  A cell copied from the first sequence is
 * (1, 0, 0) in the three masks, one copied from the pair (1, 1, 0), an id the program inserted
 * (1, 0, 1), padding (0, 0, 1) with the pad id.  n_ids receives the ids (ragged) or cells (padded)
 * needed, width the matrices' width, also on CTOK_E_CAPACITY. */
typedef struct ctok_pp_out {
  uint32_t* ids;
  uint64_t ids_cap;
  uint64_t* off;
  uint32_t* attention_mask;
  uint32_t* token_type_ids;
  uint32_t* special_tokens_mask;
  uint32_t* row_len;
  uint64_t n_ids;
  uint64_t width;
} ctok_pp_out;

/* A host batch through truncate, the program and pad (opts NULL: neither, ragged).  When ids_cap is
 * too small the call is CTOK_E_CAPACITY and writes nothing but out->n_ids and out->width; the handle
 * keeps the result (ctok_postprocessor_fetch).  CTOK_E_ARG: the offsets are not in order. */
int ctok_postprocessor_run(ctok_postprocessor* pp, const ctok_pp_batch* in, const ctok_pp_opts* opts, ctok_pp_out* out);

/* The result of the last ctok_postprocessor_run, or of a ctok_postprocessor_run_device that was
 * CTOK_E_CAPACITY, again, which the handle keeps on the device until its next run: for a caller whose
 * capacity was too small, without a second run.  out as for that run (host buffers).  CTOK_E_CAPACITY
 * as there; CTOK_E_ARG: there is no such result. */
int ctok_postprocessor_fetch(ctok_postprocessor* pp, ctok_pp_out* out);

/* The ragged run with every buffer resident in the device's memory and the work ordered on `stream`
 * (a hipStream_t; NULL: the default stream); n_ids = off[n_rows], n_pair_ids = pair_off[n_rows] (0
 * without pairs).  opts as above with padded == 0 (CTOK_E_ARG otherwise).  As for the other device
 * entries (ctok.h, "buffers of the device entry points"): ids arrays must be 4-byte and offset arrays
 * 8-byte aligned, CTOK_E_ARG at the entry before any device is used; out_cap may be exactly the
 * number of ids, nothing past d_out[n_out) and d_out_off[n_rows] is written; on CTOK_E_CAPACITY
 * nothing is written to d_out or d_out_off, *n_out holds the size needed and the handle keeps the
 * result for ctok_postprocessor_fetch.  No id outside the offsets' ranges is read.  The call returns
 * after the stream has finished the work. */
int ctok_postprocessor_run_device(ctok_postprocessor* pp, const ctok_pp_batch* d_in, uint64_t n_ids, uint64_t n_pair_ids,
                                  const ctok_pp_opts* opts, uint32_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                                  uint64_t* n_out, void* stream);

/* The stages of a run ("count", "scan", "write") and the HIP-event time of each in the last run.  ms
 * has room for cap values; *n receives the number of stages. */
int ctok_postprocessor_stage_ms(const ctok_postprocessor* pp, double* ms, uint64_t cap, uint64_t* n);
const char* ctok_postprocessor_stage_name(const ctok_postprocessor* pp, uint64_t i);

/* The compiled lists' sizes and what the last run did. */
typedef struct ctok_postprocessor_info {
  uint64_t steps;
  uint64_t items_single; /* the list of rows without a pair */
  uint64_t items_pair;
  uint64_t rows;
  uint64_t ids_in;
  uint64_t pair_ids_in;
  uint64_t ids_out; /* the rows' ids, without padding */
  uint64_t width;   /* the longest processed row, or the matrices' width */
} ctok_postprocessor_info;
int ctok_postprocessor_stats(const ctok_postprocessor* pp, ctok_postprocessor_info* out);

#ifdef __cplusplus
}
#endif

#endif /* CTOK_POSTPROCESSOR_H */
