// Host runtime of the PostProcessor behind include/ctok_postprocessor.h.
//
// Reference: PostProcessor::process with truncate and pad, src/postprocessors.rs:34-280
// (Complexity-ML/complexity-tokenizer v0.3.3).  create compiles the program into its two flat lists
// (postproc_compile.cpp) and refuses one that is too long; the lists go to the device at the first
// run.  A run counts (postproc.hip), scans the rows' lengths, reads the total and the longest row
// back, refuses 2^32 ids, and writes into buffers of the counted size.  A host run writes into the
// handle's buffers and copies out; the device entry writes into the caller's when they are large
// enough and into the handle's when they are not, so that the caller can fetch.  There is no CPU path.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_postprocessor.h"
#include "ctok_internal.h"  // ctok_dev::scan_u64, scan_tmp_elems
#include "host_common.h"
#include "postproc_internal.h"
#include "train_host_common.h"

using ctok_host::throw_error;
using ctok_train_host::DBuf;

static_assert(CTOK_PP_MAX_ITEMS == postproc::kMaxItems, "postproc_hd.h repeats the limit of ctok_postprocessor.h");
static_assert(CTOK_PP_ONLY_FIRST == postproc::ONLY_FIRST && CTOK_PP_ONLY_SECOND == postproc::ONLY_SECOND &&
                  CTOK_PP_LONGEST_FIRST == postproc::LONGEST_FIRST,
              "postproc_hd.h repeats the strategies of ctok_postprocessor.h");

namespace {

constexpr uint64_t kRefuseFrom = 1ull << 32;  // ids of the input or the output, rows, cells of a matrix
enum Stage { S_COUNT, S_SCAN, S_WRITE, S_N };
const char* const kStageNames[S_N] = {"count", "scan", "write"};

postproc::Opts opts_of(const ctok_pp_opts* o) {
  postproc::Opts r{};
  if (!o) return r;
  if (o->truncate && o->strategy > CTOK_PP_LONGEST_FIRST) throw_error(CTOK_E_ARG, "postprocessor: no such truncation strategy");
  r.truncate = o->truncate ? 1 : 0;
  r.strategy = o->strategy;
  r.truncate_to = o->truncate_to;
  r.pad_left = o->pad_left ? 1 : 0;
  r.pad_id = o->pad_id;
  return r;
}

}  // namespace

struct ctok_postprocessor {
  int device = 0;
  uint64_t n_steps = 0;
  postproc::Program prog;
  bool ready = false;
  hipStream_t own = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  DBuf<uint16_t> d_tab;
  DBuf<uint32_t> d_val;
  ctok_pp::DevProgram dprog{};
  DBuf<uint32_t> in_ids, in_pair, out_ids, out_attn, out_type, out_special, out_row_len;
  DBuf<uint64_t> in_off, in_pair_off, off, tmp, meta;
  DBuf<uint8_t> in_has;
  DBuf<postproc::Row> rows;
  double ms[S_N] = {0, 0, 0};
  ctok_postprocessor_info info{};
  // the last result in the handle's buffers, kept until the next run
  bool has_last = false, last_padded = false;
  uint64_t last_rows = 0, last_n = 0, last_width = 0;

  ~ctok_postprocessor() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (own) (void)hipStreamDestroy(own);
  }

  void prepare() {
    HIPT(hipSetDevice(device));
    if (ready) return;
    const postproc::HostList* ls[2] = {&prog.single, &prog.pair};
    std::vector<uint16_t> tab;
    std::vector<uint32_t> val;
    size_t tab_at[2], val_at[2];
    for (int i = 0; i < 2; i++) {
      tab_at[i] = tab.size();
      val_at[i] = val.size();
      tab.insert(tab.end(), ls[i]->pa.begin(), ls[i]->pa.end());
      tab.insert(tab.end(), ls[i]->pb.begin(), ls[i]->pb.end());
      tab.insert(tab.end(), ls[i]->ps.begin(), ls[i]->ps.end());
      val.insert(val.end(), ls[i]->val.begin(), ls[i]->val.end());
    }
    d_tab.ensure(tab.size());
    d_val.ensure(val.size() + 1);
    HIPT(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (!val.empty()) HIPT(hipMemcpy(d_val.p, val.data(), val.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    postproc::List* ds[2] = {&dprog.single, &dprog.pair};
    for (int i = 0; i < 2; i++) {
      const uint32_t n = (uint32_t)ls[i]->items.size();
      const uint16_t* t = d_tab.p + tab_at[i];
      *ds[i] = postproc::List{t, t + (n + 1), t + 2 * (size_t)(n + 1), d_val.p + val_at[i], n};
    }
    meta.ensure(ctok_pp::kMetaN);
    HIPT(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    for (hipEvent_t& e : ev) HIPT(hipEventCreate(&e));
    ready = true;
  }

  void begin_run() {
    prepare();
    has_last = false;
    const uint64_t a = info.items_single, b = info.items_pair;
    info = ctok_postprocessor_info{};
    info.steps = n_steps;
    info.items_single = a;
    info.items_pair = b;
    for (double& m : ms) m = 0.0;
  }

  // count and scan of a batch on the device: leaves rows and off, returns the total; *longest is the
  // longest processed row.  Refuses before anything is written.
  uint64_t count(const postproc::In& in, const postproc::Opts& o, uint64_t* longest, hipStream_t s) {
    if (in.n_rows >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "postprocessor: the batch has 2^32 rows");
    if (in.n_ids >= kRefuseFrom || in.n_pair_ids >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "postprocessor: the input reaches 2^32 ids");
    info.rows = in.n_rows;
    info.ids_in = in.n_ids;
    info.pair_ids_in = in.n_pair_ids;
    rows.ensure(in.n_rows + 1);
    off.ensure(in.n_rows + 1);
    tmp.ensure(ctok_dev::scan_tmp_elems(in.n_rows + 1) + 64);
    HIPT(hipEventRecord(ev[0], s));
    HIPT(ctok_pp::launch_count(in, o, dprog, rows.p, off.p, meta.p, s));
    HIPT(hipEventRecord(ev[1], s));
    HIPT(ctok_dev::scan_u64(off.p, in.n_rows, tmp.p, tmp.cap, s));
    HIPT(hipEventRecord(ev[2], s));
    uint64_t m[ctok_pp::kMetaN] = {0, 0}, total = 0;
    HIPT(hipMemcpyAsync(m, meta.p, sizeof(m), hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(&total, off.p + in.n_rows, 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    float t = 0;
    HIPT(hipEventElapsedTime(&t, ev[0], ev[1]));
    ms[S_COUNT] = t;
    HIPT(hipEventElapsedTime(&t, ev[1], ev[2]));
    ms[S_SCAN] = t;
    if (m[ctok_pp::kMetaBad]) throw_error(CTOK_E_ARG, "postprocessor: the offsets are not in order");
    if (total >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "postprocessor: the output reaches 2^32 ids");
    *longest = m[ctok_pp::kMetaLongest];
    info.ids_out = total;
    info.width = *longest;
    return total;
  }

  void write_ragged(const postproc::In& in, uint64_t total, uint32_t* d_out, hipStream_t s) {
    HIPT(hipEventRecord(ev[2], s));
    HIPT(ctok_pp::launch_write_ragged(in, dprog, rows.p, off.p, total, d_out, s));
    HIPT(hipEventRecord(ev[3], s));
    HIPT(hipEventSynchronize(ev[3]));
    float t = 0;
    HIPT(hipEventElapsedTime(&t, ev[2], ev[3]));
    ms[S_WRITE] = t;
  }

  // the whole run into the handle's buffers; leaves last_*
  void run_own(const postproc::In& in, const ctok_pp_opts* opts, hipStream_t s) {
    const postproc::Opts o = opts_of(opts);
    uint64_t longest = 0;
    const uint64_t total = count(in, o, &longest, s);
    const bool padded = opts && opts->padded;
    if (!padded) {
      out_ids.ensure(total + 1);
      write_ragged(in, total, out_ids.p, s);
      last_n = total;
      last_width = longest;
    } else {
      const uint64_t width = longest > opts->pad_to ? longest : opts->pad_to;
      // (width may be any u64: the product is taken where it cannot wrap)
      if (in.n_rows && width >= (kRefuseFrom + in.n_rows - 1) / in.n_rows)
        throw_error(CTOK_E_CAPACITY, "postprocessor: the padded output reaches 2^32 ids");
      const uint64_t cells = in.n_rows * width;
      out_ids.ensure(cells + 1);
      out_attn.ensure(cells + 1);
      out_type.ensure(cells + 1);
      out_special.ensure(cells + 1);
      out_row_len.ensure(in.n_rows + 1);
      const ctok_pp::Matrix m{out_ids.p, out_attn.p, out_type.p, out_special.p, out_row_len.p, width};
      HIPT(hipEventRecord(ev[2], s));
      HIPT(ctok_pp::launch_write_matrix(in, o, dprog, rows.p, off.p, m, s));
      HIPT(hipEventRecord(ev[3], s));
      HIPT(hipEventSynchronize(ev[3]));
      float t = 0;
      HIPT(hipEventElapsedTime(&t, ev[2], ev[3]));
      ms[S_WRITE] = t;
      last_n = cells;
      last_width = width;
      info.width = width;
    }
    last_padded = padded;
    last_rows = in.n_rows;
    has_last = true;
  }

  void deliver_host(ctok_pp_out* out, const char* who) {
    out->n_ids = last_n;
    out->width = last_width;
    if (last_n > out->ids_cap)
      throw_error(CTOK_E_CAPACITY, std::string(who) + ": the result needs " + std::to_string(last_n) + " ids");
    const size_t bytes = last_n * sizeof(uint32_t);
    if (last_padded) {
      if (last_n && (!out->ids || !out->attention_mask || !out->token_type_ids || !out->special_tokens_mask))
        throw_error(CTOK_E_ARG, "null argument");
      if (last_rows && !out->row_len) throw_error(CTOK_E_ARG, "null argument");
      if (last_n) {
        HIPT(hipMemcpyAsync(out->ids, out_ids.p, bytes, hipMemcpyDeviceToHost, own));
        HIPT(hipMemcpyAsync(out->attention_mask, out_attn.p, bytes, hipMemcpyDeviceToHost, own));
        HIPT(hipMemcpyAsync(out->token_type_ids, out_type.p, bytes, hipMemcpyDeviceToHost, own));
        HIPT(hipMemcpyAsync(out->special_tokens_mask, out_special.p, bytes, hipMemcpyDeviceToHost, own));
      }
      if (last_rows) HIPT(hipMemcpyAsync(out->row_len, out_row_len.p, last_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, own));
    } else {
      if ((last_n && !out->ids) || !out->off) throw_error(CTOK_E_ARG, "null argument");
      if (last_n) HIPT(hipMemcpyAsync(out->ids, out_ids.p, bytes, hipMemcpyDeviceToHost, own));
      HIPT(hipMemcpyAsync(out->off, off.p, (last_rows + 1) * 8, hipMemcpyDeviceToHost, own));
    }
    HIPT(hipStreamSynchronize(own));
  }

  void run_host(const ctok_pp_batch& b, const ctok_pp_opts* opts, ctok_pp_out* out) {
    const uint64_t n = b.n_rows;
    if (n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "postprocessor: the batch has 2^32 rows");
    if (b.off[0] != 0) throw_error(CTOK_E_ARG, "postprocessor: the offsets are not in order");
    for (uint64_t r = 0; r < n; r++)
      if (b.off[r] > b.off[r + 1]) throw_error(CTOK_E_ARG, "postprocessor: the offsets are not in order");
    const uint64_t n_ids = b.off[n];
    uint64_t n_pair = 0;
    if (b.pair_off)  // (what the rows with a pair reach; the device checks each)
      for (uint64_t r = 0; r < n; r++)
        if ((!b.has_pair || b.has_pair[r]) && b.pair_off[r + 1] > n_pair) n_pair = b.pair_off[r + 1];
    if (n_ids >= kRefuseFrom || n_pair >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "postprocessor: the input reaches 2^32 ids");
    if ((n_ids && !b.ids) || (n_pair && !b.pair_ids)) throw_error(CTOK_E_ARG, "null argument");
    begin_run();
    in_ids.ensure(n_ids + 1);
    in_off.ensure(n + 1);
    if (n_ids) HIPT(hipMemcpyAsync(in_ids.p, b.ids, n_ids * 4, hipMemcpyHostToDevice, own));
    HIPT(hipMemcpyAsync(in_off.p, b.off, (n + 1) * 8, hipMemcpyHostToDevice, own));
    postproc::In in{};
    in.ids = in_ids.p;
    in.off = in_off.p;
    in.n_rows = n;
    in.n_ids = n_ids;
    if (b.pair_off) {
      in_pair.ensure(n_pair + 1);
      in_pair_off.ensure(n + 1);
      if (n_pair) HIPT(hipMemcpyAsync(in_pair.p, b.pair_ids, n_pair * 4, hipMemcpyHostToDevice, own));
      HIPT(hipMemcpyAsync(in_pair_off.p, b.pair_off, (n + 1) * 8, hipMemcpyHostToDevice, own));
      in.pair_ids = in_pair.p;
      in.pair_off = in_pair_off.p;
      in.n_pair_ids = n_pair;
      if (b.has_pair) {
        in_has.ensure(n + 1);
        if (n) HIPT(hipMemcpyAsync(in_has.p, b.has_pair, n, hipMemcpyHostToDevice, own));
        in.has_pair = in_has.p;
      }
    }
    run_own(in, opts, own);
    deliver_host(out, "ctok_postprocessor_run");
  }

  void run_device(const ctok_pp_batch& b, uint64_t n_ids, uint64_t n_pair_ids, const ctok_pp_opts* opts, uint32_t* d_out,
                  uint64_t out_cap, uint64_t* d_out_off, uint64_t* n_out, hipStream_t s) {
    begin_run();
    postproc::In in{};
    in.ids = b.ids;
    in.off = b.off;
    in.n_rows = b.n_rows;
    in.n_ids = n_ids;
    if (b.pair_off) {
      in.pair_ids = b.pair_ids;
      in.pair_off = b.pair_off;
      in.has_pair = b.has_pair;
      in.n_pair_ids = n_pair_ids;
    }
    const postproc::Opts o = opts_of(opts);
    uint64_t longest = 0;
    const uint64_t total = count(in, o, &longest, s);
    *n_out = total;
    if (total > out_cap) {  // into the handle's buffer, for ctok_postprocessor_fetch
      out_ids.ensure(total + 1);
      write_ragged(in, total, out_ids.p, s);
      last_padded = false;
      last_rows = in.n_rows;
      last_n = total;
      last_width = longest;
      has_last = true;
      throw_error(CTOK_E_CAPACITY, "ctok_postprocessor_run_device: the result needs " + std::to_string(total) + " ids");
    }
    if (total && !d_out) throw_error(CTOK_E_ARG, "null argument");
    HIPT(hipMemcpyAsync(d_out_off, off.p, (in.n_rows + 1) * 8, hipMemcpyDeviceToDevice, s));
    write_ragged(in, total, d_out, s);
    HIPT(hipStreamSynchronize(s));
  }
};

extern "C" {

int ctok_postprocessor_create(const ctok_pp_step* steps, uint64_t n_steps, int device, ctok_postprocessor** out) {
  return ctok_host::run_guarded([&] {
    if (!out || (n_steps && !steps)) throw_error(CTOK_E_ARG, "null argument");
    *out = nullptr;
    if (n_steps > CTOK_PP_MAX_STEPS)
      throw_error(CTOK_E_UNSUPPORTED, "postprocessor: more than " + std::to_string(CTOK_PP_MAX_STEPS) + " steps");
    std::vector<postproc::HostStep> hs(n_steps);
    for (uint64_t i = 0; i < n_steps; i++) {
      const ctok_pp_step& s = steps[i];
      if ((s.single_len && !s.single) || (s.pair_len && !s.pair) || (s.n_tok && (!s.tok_off || !s.tok_id)))
        throw_error(CTOK_E_ARG, "null argument");
      postproc::HostStep& h = hs[i];
      h.kind = s.kind;
      h.has_pair_template = (s.flags & 1u) != 0;
      if (s.single_len) h.single.assign((const char*)s.single, s.single_len);
      if (s.pair_len) h.pair.assign((const char*)s.pair, s.pair_len);
      for (uint64_t t = 0; t < s.n_tok; t++) {
        if (s.tok_off[t] > s.tok_off[t + 1] || (s.tok_off[t + 1] && !s.tok_bytes))
          throw_error(CTOK_E_ARG, "postprocessor: the special tokens' offsets are not in order");
        h.specials.emplace_back(std::string((const char*)s.tok_bytes + s.tok_off[t], s.tok_off[t + 1] - s.tok_off[t]), s.tok_id[t]);
      }
      h.id_a = s.id_a;
      h.id_b = s.id_b;
    }
    std::unique_ptr<ctok_postprocessor> pp(new ctok_postprocessor);
    pp->device = device;
    pp->n_steps = n_steps;
    std::string err;
    const postproc::CompileError ce = postproc::compile(hs, &pp->prog, &err);
    if (ce != postproc::C_OK) throw_error(ce == postproc::C_CAPACITY ? CTOK_E_CAPACITY : CTOK_E_ARG, err);
    pp->info.steps = n_steps;
    pp->info.items_single = pp->prog.single.items.size();
    pp->info.items_pair = pp->prog.pair.items.size();
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
      (void)hipGetLastError();
      throw_error(CTOK_E_DEVICE, "postprocessor: no HIP device " + std::to_string(device));
    }
    *out = pp.release();
  });
}

void ctok_postprocessor_destroy(ctok_postprocessor* pp) { delete pp; }

int ctok_postprocessor_run(ctok_postprocessor* pp, const ctok_pp_batch* in, const ctok_pp_opts* opts, ctok_pp_out* out) {
  return ctok_host::run_guarded([&] {
    if (!pp || !in || !out || !in->off) throw_error(CTOK_E_ARG, "null argument");
    out->n_ids = 0;
    out->width = 0;
    pp->run_host(*in, opts, out);
  });
}

int ctok_postprocessor_fetch(ctok_postprocessor* pp, ctok_pp_out* out) {
  return ctok_host::run_guarded([&] {
    if (!pp || !out) throw_error(CTOK_E_ARG, "null argument");
    out->n_ids = 0;
    out->width = 0;
    if (!pp->has_last) throw_error(CTOK_E_ARG, "ctok_postprocessor_fetch: no result to fetch");
    HIPT(hipSetDevice(pp->device));
    pp->deliver_host(out, "ctok_postprocessor_fetch");
  });
}

int ctok_postprocessor_run_device(ctok_postprocessor* pp, const ctok_pp_batch* d_in, uint64_t n_ids, uint64_t n_pair_ids,
                                  const ctok_pp_opts* opts, uint32_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                                  uint64_t* n_out, void* stream) {
  return ctok_host::run_guarded([&] {
    if (!pp || !d_in || !d_in->off || !d_out_off || !n_out) throw_error(CTOK_E_ARG, "null argument");
    *n_out = 0;
    if ((n_ids && !d_in->ids) || (d_in->pair_off && n_pair_ids && !d_in->pair_ids)) throw_error(CTOK_E_ARG, "null argument");
    if (opts && opts->padded) throw_error(CTOK_E_ARG, "ctok_postprocessor_run_device: the output is ragged");
    // checked before any device is used: a refused call launches nothing and writes nothing
    if (((uintptr_t)d_in->ids | (uintptr_t)d_in->pair_ids | (uintptr_t)d_out) & 3u)
      throw_error(CTOK_E_ARG, "ctok_postprocessor_run_device: the ids must be 4-byte aligned");
    if (((uintptr_t)d_in->off | (uintptr_t)d_in->pair_off | (uintptr_t)d_out_off) & 7u)
      throw_error(CTOK_E_ARG, "ctok_postprocessor_run_device: the offsets must be 8-byte aligned");
    pp->run_device(*d_in, n_ids, n_pair_ids, opts, d_out, out_cap, d_out_off, n_out, (hipStream_t)stream);
  });
}

int ctok_postprocessor_stage_ms(const ctok_postprocessor* pp, double* ms, uint64_t cap, uint64_t* n) {
  return ctok_host::run_guarded([&] {
    if (!pp || !n || (cap && !ms)) throw_error(CTOK_E_ARG, "null argument");
    *n = S_N;
    for (uint64_t i = 0; i < cap && i < S_N; i++) ms[i] = pp->ms[i];
  });
}

const char* ctok_postprocessor_stage_name(const ctok_postprocessor* pp, uint64_t i) {
  if (!pp || i >= S_N) return "";
  return kStageNames[i];
}

int ctok_postprocessor_stats(const ctok_postprocessor* pp, ctok_postprocessor_info* out) {
  return ctok_host::run_guarded([&] {
    if (!pp || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = pp->info;
  });
}

}  // extern "C"
