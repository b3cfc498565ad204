// Host runtime of the Decoder behind include/ctok_decoder.h.
//
// Reference: Decoder::decode, src/decoders.rs:30-243 (Complexity-ML/complexity-tokenizer v0.3.3).  A
// run takes the whole batch through the program's ops on the device, one after the other
// (decoder.hip).  Every op prepares, counts per workgroup, the sums are scanned and the total comes back
// to the host, which refuses 4 GiB and grows the other text buffer to the total before the write.  An
// op leaves the documents' texts and their offsets; they are the next op's tokens, one per document.
// The caller's capacity is checked against the last op's total before anything is written to the
// caller's buffers.  The ids entry gathers the ids' tokens first.  There is no CPU path.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_decoder.h"
#include "ctok_internal.h"  // ctok_dev::scan_u64, scan_tmp_elems
#include "decoder_internal.h"
#include "host_common.h"
#include "train_host_common.h"

using ctok_host::throw_error;
using ctok_train_host::DBuf;
using decoder::HostOp;

namespace {

constexpr uint64_t kRefuseFrom = 1ull << 32;  // a batch of 4 GiB or 2^32 tokens, before or after any op

struct State {  // a batch on the device between two ops
  const uint8_t* bytes;
  uint64_t n;
  const uint64_t* tok_off;
  uint64_t n_tok;
  const uint64_t* doc_tok;
  const uint64_t* doc_off;
};

}  // namespace

struct ctok_decoder {
  int device = 0;
  std::vector<uint32_t> kinds;      // the steps
  std::vector<HostOp> ops;          // their ops
  std::vector<size_t> op_step;      // the step of op i
  // the ops' strings on the device: op i's a at at_a[i], its b at at_b[i]
  std::string blob;
  std::vector<uint64_t> at_a, at_b;
  DBuf<uint8_t> d_blob;
  bool ready = false;
  hipStream_t own = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DBuf<uint64_t> off[2], doc_off, iota, lo, hi, first, blk, tmp, in_tok_off, in_doc_tok;
  DBuf<uint64_t> g_keep, g_len, g_doc_tok, in_ids_off;
  DBuf<uint32_t> flag, in_ids;
  DBuf<uint8_t> buf[2], cand, mark, in_bytes, g_bytes;
  // the vocabulary of the ids entry
  bool has_vocab = false;
  uint64_t n_ent = 0;
  DBuf<uint2> d_ent;
  DBuf<uint8_t> d_pool;
  std::vector<double> ms;
  ctok_decoder_info info{};
  State last{};  // the last run's result, kept on the device until the next run
  uint64_t last_docs = 0;
  bool has_last = false;

  ~ctok_decoder() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own) (void)hipStreamDestroy(own);
  }

  void add_step(const ctok_dec_step& s) {
    const std::string a((const char*)s.a, s.a_len), b((const char*)s.b, s.b_len);
    const size_t before = ops.size();
    const char* err = decoder::expand(s.kind, s.flags, a, b, s.cp, s.start, s.stop, &ops);
    if (err) throw_error(CTOK_E_ARG, std::string("decoder step ") + std::to_string(kinds.size()) + ": " + err);
    for (size_t i = before; i < ops.size(); i++) {
      op_step.push_back(kinds.size());
      at_a.push_back(blob.size());
      blob += ops[i].a;
      at_b.push_back(blob.size());
      blob += ops[i].b;
    }
    kinds.push_back(s.kind);
  }

  void prepare() {
    HIPT(hipSetDevice(device));
    if (ready) return;
    d_blob.ensure(blob.size() + 16);
    if (!blob.empty()) HIPT(hipMemcpy(d_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    flag.ensure(4);
    HIPT(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    HIPT(hipEventCreate(&ev0));
    HIPT(hipEventCreate(&ev1));
    ready = true;
  }

  decoder::Step step_of(size_t i) const {
    const HostOp& h = ops[i];
    return decoder::Step{h.op, h.flags, d_blob.p + at_a[i], h.a.size(), d_blob.p + at_b[i], h.b.size()};
  }

  uint64_t scan_total(uint64_t* p, uint64_t n, hipStream_t s) {  // p[n] = the total, also returned
    uint64_t total = 0;
    tmp.ensure(ctok_dev::scan_tmp_elems(n + 1) + 64);
    HIPT(ctok_dev::scan_u64(p, n, tmp.p, tmp.cap, s));
    HIPT(hipMemcpyAsync(&total, p + n, 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    return total;
  }

  State run_op(size_t i, const State& cur, uint64_t n_docs, int* w, hipStream_t s) {
    const HostOp& h = ops[i];
    const decoder::Step st = step_of(i);
    decoder::In in{};
    in.bytes = cur.bytes;
    in.n = cur.n;
    in.tok_off = cur.tok_off;
    in.n_tok = cur.n_tok;
    in.doc_tok = cur.doc_tok;
    in.n_docs = n_docs;
    in.doc_off = cur.doc_off;
    ctok_dc::Scratch sc{};
    // (The op before may still be writing when these grow: DBuf::ensure frees with hipFree, which waits for the
    // device, and every step ends with an event wait.  An asynchronous free would need a wait here.)
    if (h.prep == decoder::P_STRIP || h.prep == decoder::P_TRIM) {
      lo.ensure(n_docs + 1);
      hi.ensure(n_docs + 1);
      in.lo = sc.lo = lo.p;
      in.hi = sc.hi = hi.p;
    }
    if (h.prep == decoder::P_WP_FIRST) {
      first.ensure(n_docs + 1);
      in.first = sc.first = first.p;
    }
    if (h.prep == decoder::P_REPLACE || h.prep == decoder::P_CLEANUP) {
      mark.ensure(cur.n + 1);
      in.mark = sc.mark = mark.p;
      if (h.prep == decoder::P_REPLACE) {
        cand.ensure(cur.n + 1);
        sc.cand = cand.p;
      }
    }
    HIPT(ctok_dc::launch_prep(h.prep, st, h.start, h.stop, in, sc, s));
    const uint64_t nblk = ctok_dc::unit_blocks(decoder::n_units(st, in));
    blk.ensure(nblk + 1);
    HIPT(ctok_dc::launch_count(st, in, blk.p, s));
    const uint64_t total = scan_total(blk.p, nblk, s) + n_docs * decoder::tail_len(st);
    if (total >= kRefuseFrom)
      throw_error(CTOK_E_CAPACITY, std::string("decoder: the output of step ") + std::to_string(op_step[i]) + " (" +
                                       decoder::kind_name(kinds[op_step[i]]) + ") reaches 4 GiB");
    const int o = *w;
    *w ^= 1;
    buf[o].ensure(total + 16);
    off[o].ensure(n_docs + 1);
    HIPT(ctok_dc::launch_write(st, in, blk.p, buf[o].p, off[o].p, s));
    info.passes++;
    if (total > info.bytes_peak) info.bytes_peak = total;
    return State{buf[o].p, total, off[o].p, n_docs, iota.p, off[o].p};
  }

  // The whole program over a batch on the device; leaves `last`.  The offsets are checked first.
  void run_ops(const uint8_t* d_bytes, uint64_t n, const uint64_t* d_tok_off, uint64_t n_tok, const uint64_t* d_doc_tok,
               uint64_t n_docs, hipStream_t s) {
    if (n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the input reaches 4 GiB");
    if (n_tok >= kRefuseFrom || n_docs >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the batch has 2^32 tokens");
    info.steps = kinds.size();
    info.docs = n_docs;
    info.tokens = n_tok;
    info.bytes_in = n;
    if (n > info.bytes_peak) info.bytes_peak = n;
    uint32_t bad = 0;
    HIPT(ctok_dc::launch_check(d_tok_off, n_tok, n, d_doc_tok, n_docs, flag.p, s));
    HIPT(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (bad) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    doc_off.ensure(n_docs + 1);
    iota.ensure(n_docs + 1);
    HIPT(ctok_dc::launch_doc_off(d_tok_off, d_doc_tok, n_docs, doc_off.p, s));
    HIPT(ctok_dc::launch_iota(iota.p, n_docs, s));
    State cur{d_bytes, n, d_tok_off, n_tok, d_doc_tok, doc_off.p};
    int w = 0;
    size_t i = 0;
    for (size_t k = 0; k < kinds.size(); k++) {
      HIPT(hipEventRecord(ev0, s));
      for (; i < ops.size() && op_step[i] == k; i++) cur = run_op(i, cur, n_docs, &w, s);
      HIPT(hipEventRecord(ev1, s));
      HIPT(hipEventSynchronize(ev1));
      float t = 0;
      HIPT(hipEventElapsedTime(&t, ev0, ev1));
      ms[k + 1] = t;
    }
    last = cur;
    last_docs = n_docs;
    has_last = true;
    info.bytes_out = cur.n;
  }

  void begin_run() {
    prepare();
    has_last = false;
    info = ctok_decoder_info{};
    ms.assign(kinds.size() + 1, 0.0);
  }

  // the result into device buffers of last.n bytes and n_docs + 1 offsets
  void deliver(uint64_t n_docs, uint8_t* d_text, uint64_t* d_text_off, hipStream_t s) {
    if (last.n) HIPT(hipMemcpyAsync(d_text, last.bytes, last.n, hipMemcpyDeviceToDevice, s));
    HIPT(hipMemcpyAsync(d_text_off, last.doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToDevice, s));
  }

  void deliver_host(uint64_t n_docs, uint8_t* text, uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out,
                    const char* who) {
    *n_bytes_out = last.n;
    if (last.n > text_cap)
      throw_error(CTOK_E_CAPACITY, std::string(who) + ": the texts need " + std::to_string(last.n) + " bytes");
    if (last.n && !text) throw_error(CTOK_E_ARG, "null argument");
    if (last.n) HIPT(hipMemcpyAsync(text, last.bytes, last.n, hipMemcpyDeviceToHost, own));
    HIPT(hipMemcpyAsync(text_off, last.doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, own));
    HIPT(hipStreamSynchronize(own));
  }

  void run_host(const uint8_t* tokens, const uint64_t* tok_off, const uint64_t* doc_tok, uint64_t n_docs, uint8_t* text,
                uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out) {
    if (doc_tok[0] != 0) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    for (uint64_t d = 0; d < n_docs; d++)
      if (doc_tok[d] > doc_tok[d + 1]) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    const uint64_t n_tok = doc_tok[n_docs];
    if (n_tok >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the batch has 2^32 tokens");
    if (!tok_off || tok_off[0] != 0) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    for (uint64_t j = 0; j < n_tok; j++)
      if (tok_off[j] > tok_off[j + 1]) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    const uint64_t n = tok_off[n_tok];
    if (n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the input reaches 4 GiB");
    if (n && !tokens) throw_error(CTOK_E_ARG, "null argument");
    for (uint64_t j = 0; j < n_tok; j++)  // every token is well-formed UTF-8 (what a Rust String is)
      if (!decoder::is_utf8(tokens, tok_off[j], tok_off[j + 1])) throw_error(CTOK_E_ARG, "a token is not valid UTF-8");
    begin_run();
    in_bytes.ensure(n + 16);
    in_tok_off.ensure(n_tok + 1);
    in_doc_tok.ensure(n_docs + 1);
    if (n) HIPT(hipMemcpyAsync(in_bytes.p, tokens, n, hipMemcpyHostToDevice, own));
    HIPT(hipMemcpyAsync(in_tok_off.p, tok_off, (n_tok + 1) * 8, hipMemcpyHostToDevice, own));
    HIPT(hipMemcpyAsync(in_doc_tok.p, doc_tok, (n_docs + 1) * 8, hipMemcpyHostToDevice, own));
    run_ops(in_bytes.p, n, in_tok_off.p, n_tok, in_doc_tok.p, n_docs, own);
    deliver_host(n_docs, text, text_cap, text_off, n_bytes_out, "ctok_decoder_run");
  }

  void run_ids(const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, uint8_t* text, uint64_t text_cap,
               uint64_t* text_off, uint64_t* n_bytes_out) {
    if (!has_vocab) throw_error(CTOK_E_ARG, "decoder: no vocabulary (set_vocab)");
    if (ids_off[0] != 0) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    for (uint64_t d = 0; d < n_docs; d++)
      if (ids_off[d] > ids_off[d + 1]) throw_error(CTOK_E_ARG, "decoder: the offsets are not in order");
    const uint64_t n_ids = ids_off[n_docs];
    if (n_ids >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the batch has 2^32 tokens");
    if (n_ids && !ids) throw_error(CTOK_E_ARG, "null argument");
    begin_run();
    hipStream_t s = own;
    in_ids.ensure(n_ids + 1);
    in_ids_off.ensure(n_docs + 1);
    if (n_ids) HIPT(hipMemcpyAsync(in_ids.p, ids, n_ids * 4, hipMemcpyHostToDevice, s));
    HIPT(hipMemcpyAsync(in_ids_off.p, ids_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HIPT(hipEventRecord(ev0, s));
    // the ids that have an entry, their places among the tokens, the tokens' lengths and offsets
    g_keep.ensure(n_ids + 1);
    HIPT(ctok_dc::launch_gather_keep(in_ids.p, n_ids, d_ent.p, n_ent, g_keep.p, s));
    const uint64_t n_tok = scan_total(g_keep.p, n_ids, s);
    g_len.ensure(n_tok + 1);
    g_doc_tok.ensure(n_docs + 1);
    HIPT(ctok_dc::launch_gather_len(in_ids.p, n_ids, d_ent.p, n_ent, g_keep.p, in_ids_off.p, n_docs, g_len.p, g_doc_tok.p, s));
    const uint64_t n = scan_total(g_len.p, n_tok, s);
    if (n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the ids' tokens reach 4 GiB");
    g_bytes.ensure(n + 16);
    HIPT(ctok_dc::launch_gather_write(in_ids.p, n_ids, d_ent.p, n_ent, d_pool.p, g_keep.p, g_len.p, g_bytes.p, s));
    HIPT(hipEventRecord(ev1, s));
    HIPT(hipEventSynchronize(ev1));
    float t = 0;
    HIPT(hipEventElapsedTime(&t, ev0, ev1));
    run_ops(g_bytes.p, n, g_len.p, n_tok, g_doc_tok.p, n_docs, s);
    ms[0] = t;
    deliver_host(n_docs, text, text_cap, text_off, n_bytes_out, "ctok_decoder_run_ids");
  }

  void set_vocab(const uint8_t* pool, uint64_t pool_len, const uint32_t* ent_off, const uint32_t* ent_len, uint64_t n) {
    if (pool_len >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "decoder: the vocabulary reaches 4 GiB");
    std::vector<uint2> ent(n);
    for (uint64_t i = 0; i < n; i++) {
      ent[i] = make_uint2(ent_off[i], ent_len[i]);
      if (ent_len[i] == CTOK_DEC_NO_ENTRY) continue;
      if ((uint64_t)ent_off[i] + ent_len[i] > pool_len) throw_error(CTOK_E_ARG, "decoder: a vocabulary entry lies outside the pool");
      if (!decoder::is_utf8(pool, ent_off[i], (uint64_t)ent_off[i] + ent_len[i]))
        throw_error(CTOK_E_ARG, "a vocabulary entry is not valid UTF-8");
    }
    prepare();
    has_vocab = false;
    d_ent.ensure(n + 1);
    d_pool.ensure(pool_len + 16);
    if (n) HIPT(hipMemcpy(d_ent.p, ent.data(), n * sizeof(uint2), hipMemcpyHostToDevice));
    if (pool_len) HIPT(hipMemcpy(d_pool.p, pool, pool_len, hipMemcpyHostToDevice));
    n_ent = n;
    has_vocab = true;
  }
};

extern "C" {

int ctok_decoder_create(const ctok_dec_step* steps, uint64_t n_steps, int device, ctok_decoder** out) {
  return ctok_host::run_guarded([&] {
    if (!out || (n_steps && !steps)) throw_error(CTOK_E_ARG, "null argument");
    *out = nullptr;
    if (n_steps > CTOK_DEC_MAX_STEPS)
      throw_error(CTOK_E_UNSUPPORTED, "decoder: more than " + std::to_string(CTOK_DEC_MAX_STEPS) + " steps");
    std::unique_ptr<ctok_decoder> dc(new ctok_decoder);
    dc->device = device;
    for (uint64_t i = 0; i < n_steps; i++) {
      if ((steps[i].a_len && !steps[i].a) || (steps[i].b_len && !steps[i].b)) throw_error(CTOK_E_ARG, "null argument");
      dc->add_step(steps[i]);
    }
    if (!n_steps) {  // the empty Sequence joins the tokens
      ctok_dec_step fuse{};
      fuse.kind = CTOK_DEC_FUSE;
      dc->add_step(fuse);
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
      (void)hipGetLastError();
      throw_error(CTOK_E_DEVICE, "decoder: no HIP device " + std::to_string(device));
    }
    *out = dc.release();
  });
}

void ctok_decoder_destroy(ctok_decoder* dc) { delete dc; }

int ctok_decoder_set_vocab(ctok_decoder* dc, const uint8_t* pool, uint64_t pool_len, const uint32_t* ent_off,
                           const uint32_t* ent_len, uint64_t n_ent) {
  return ctok_host::run_guarded([&] {
    if (!dc) throw_error(CTOK_E_ARG, "null argument");
    if (n_ent > CTOK_DEC_MAX_ID) throw_error(CTOK_E_CAPACITY, "decoder: a vocabulary id of 2^27 or more");
    if ((pool_len && !pool) || (n_ent && (!ent_off || !ent_len))) throw_error(CTOK_E_ARG, "null argument");
    dc->set_vocab(pool, pool_len, ent_off, ent_len, n_ent);
  });
}

int ctok_decoder_run(ctok_decoder* dc, const uint8_t* tokens, const uint64_t* tok_off, const uint64_t* doc_tok,
                     uint64_t n_docs, uint8_t* text, uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out) {
  return ctok_host::run_guarded([&] {
    if (!dc || !doc_tok || !text_off || !n_bytes_out) throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = 0;
    dc->run_host(tokens, tok_off, doc_tok, n_docs, text, text_cap, text_off, n_bytes_out);
  });
}

int ctok_decoder_run_ids(ctok_decoder* dc, const uint32_t* ids, const uint64_t* ids_off, uint64_t n_docs, uint8_t* text,
                         uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out) {
  return ctok_host::run_guarded([&] {
    if (!dc || !ids_off || !text_off || !n_bytes_out) throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = 0;
    dc->run_ids(ids, ids_off, n_docs, text, text_cap, text_off, n_bytes_out);
  });
}

int ctok_decoder_fetch(ctok_decoder* dc, uint8_t* text, uint64_t text_cap, uint64_t* text_off, uint64_t* n_bytes_out) {
  return ctok_host::run_guarded([&] {
    if (!dc || !text_off || !n_bytes_out) throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = 0;
    if (!dc->has_last) throw_error(CTOK_E_ARG, "ctok_decoder_fetch: no result to fetch");
    HIPT(hipSetDevice(dc->device));
    dc->deliver_host(dc->last_docs, text, text_cap, text_off, n_bytes_out, "ctok_decoder_fetch");
  });
}

int ctok_decoder_run_device(ctok_decoder* dc, const uint8_t* d_tokens, const uint64_t* d_tok_off, const uint64_t* d_doc_tok,
                            uint64_t n_docs, uint64_t n_tok, uint64_t n_bytes, uint8_t* d_text, uint64_t text_cap,
                            uint64_t* d_text_off, uint64_t* n_bytes_out, void* stream) {
  return ctok_host::run_guarded([&] {
    if (!dc || !d_tok_off || !d_doc_tok || !d_text_off || !n_bytes_out || (n_bytes && !d_tokens))
      throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = 0;
    dc->begin_run();
    hipStream_t s = (hipStream_t)stream;
    dc->run_ops(d_tokens, n_bytes, d_tok_off, n_tok, d_doc_tok, n_docs, s);
    *n_bytes_out = dc->last.n;
    if (dc->last.n > text_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_decoder_run_device: the texts need " + std::to_string(dc->last.n) + " bytes");
    if (dc->last.n && !d_text) throw_error(CTOK_E_ARG, "null argument");
    dc->deliver(n_docs, d_text, d_text_off, s);
    HIPT(hipStreamSynchronize(s));
  });
}

int ctok_decoder_stage_ms(const ctok_decoder* dc, double* ms, uint64_t cap, uint64_t* n) {
  return ctok_host::run_guarded([&] {
    if (!dc || !n || (cap && !ms)) throw_error(CTOK_E_ARG, "null argument");
    *n = dc->kinds.size() + 1;
    for (uint64_t i = 0; i < cap && i < *n; i++) ms[i] = i < dc->ms.size() ? dc->ms[i] : 0.0;
  });
}

const char* ctok_decoder_stage_name(const ctok_decoder* dc, uint64_t i) {
  if (!dc || i > dc->kinds.size()) return "";
  return i == 0 ? "gather" : decoder::kind_name(dc->kinds[i - 1]);
}

int ctok_decoder_stats(const ctok_decoder* dc, ctok_decoder_info* out) {
  return ctok_host::run_guarded([&] {
    if (!dc || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = dc->info;
  });
}

}  // extern "C"
