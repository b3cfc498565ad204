// Host runtime of the PreTokenizer behind include/ctok_pretokenizer.h.
//
// Reference: PreTokenizer::pre_tokenize, src/pretokenizers.rs:69-594 (Complexity-ML/complexity-tokenizer
// v0.3.3).  A run takes the whole batch through the program on the device, one step after the other
// (pretok.hip).  A pure splitter maps the two word bitmaps to the handle's other pair and leaves the
// text where it is; a rewriter (ByteLevel, Metaspace) counts, the spans' sums and the total come back
// to the host, which refuses 4 GiB and grows the other text buffer to the total before the write.
// The final gather counts the same way, so the caller's capacities are checked before anything is
// written.  What an empty text gives depends on the program alone (pretok_prog.h empty_fate): the
// words Metaspace makes of it are computed once, by a handle of the steps from there on over the
// replacement as a text, and the gather places them.  There is no CPU path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_pretokenizer.h"
#include "ctok_internal.h"  // ctok_dev::scan_u64, scan_tmp_elems
#include "gen/unicode_data.h"
#include "host_common.h"
#include "knobs.h"
#include "pretok_internal.h"
#include "pretok_prog.h"
#include "rust_regex.h"
#include "train_host_common.h"

using ctok_host::throw_error;
using ctok_pt::Bits;
using ctok_pt::words64;
using ctok_train_host::DBuf;
using pretok::HostStep;

namespace {

constexpr uint64_t kRefuseFrom = 1ull << 32;  // a batch of 4 GiB, before or after any step

struct State {  // a batch on the device between two steps
  const uint8_t* text;
  const uint64_t* off;
  uint64_t n;
  int bits;  // which of the handle's bitmap pairs holds its words
};

// every text is well-formed UTF-8 (what a Rust &str is)
void check_utf8(const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
  for (uint64_t i = 0; i < n_texts; i++) {
    if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    for (uint64_t p = off[i]; p < off[i + 1];) {
      uint32_t l;
      if (utf8[p] < 0x80u) {
        p++;
        continue;
      }
      if (normalize::dec(utf8, off[i + 1], p, &l) == normalize::kRaw) throw_error(CTOK_E_ARG, "a text is not valid UTF-8");
      p += l;
    }
  }
}

}  // namespace

struct ctok_pretokenizer {
  int device = 0;
  std::vector<HostStep> prog;
  // the steps' class items and literals on the device: step i's at at[i]
  std::string blob;
  std::vector<uint64_t> at;
  std::vector<pretok::StepBlob> parts;
  // the code points one start of a cyclic DFA may step through (read once, when the handle is made)
  uint32_t max_run = ctok_rt::PretokKnobs().max_regex_run;
  DBuf<uint8_t> d_blob, d_cls1, d_cls2;
  bool ready = false;
  hipStream_t own = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DBuf<uint64_t> inw[2], beg[2], off[2], len, tmp, wpos, cb, cw, ex, in_off, o_woff, o_tw, d_ew_off;
  DBuf<uint8_t> buf[2], flags, tail, carry, cand, mark, whit, in_text, o_words, d_ew_bytes;
  DBuf<uint32_t> mlen, tmax, tcarry, over;
  // the words of an empty text
  pretok::EmptyFate fate = pretok::E_NOTHING;
  size_t fate_at = 0;
  bool fate_ready = false;
  std::vector<uint64_t> ew_off{0};
  std::vector<uint8_t> ew_bytes;
  std::vector<double> ms;
  ctok_pretokenizer_info info{};
  // the last run's result, until the gather
  State last{};
  uint64_t n_words = 0, n_bytes = 0, n_empty = 0;

  ~ctok_pretokenizer() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own) (void)hipStreamDestroy(own);
  }

  void add_step(const ctok_pretok_step& s) {
    const std::string a((const char*)s.a, s.a_len);
    HostStep h;
    bool unsupported = false;
    const bool rejected = s.kind == CTOK_PRETOK_SPLIT && !ctok_rt::rust_regex_rejects(a).empty();
    const std::string err = pretok::make_step(s.kind, s.flags, a, s.cp, rejected, &h, &unsupported);
    if (!err.empty())
      throw_error(unsupported ? CTOK_E_UNSUPPORTED : CTOK_E_ARG,
                  std::string("pre-tokenizer step ") + std::to_string(prog.size()) + (unsupported ? ": split pattern " + a : "") + ": " + err);
    while (blob.size() % 4) blob.push_back('\0');
    at.push_back(blob.size());
    parts.push_back(pretok::step_blob(h));
    blob += parts.back().bytes;
    prog.push_back(h);
  }

  void prepare() {
    HIPT(hipSetDevice(device));
    if (ready) return;
    d_blob.ensure(blob.size() + 16);
    HIPT(hipMemcpy(d_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    d_cls1.ensure(sizeof(ct_cls_stage1));
    d_cls2.ensure(sizeof(ct_cls_stage2));
    HIPT(hipMemcpy(d_cls1.p, ct_cls_stage1, sizeof(ct_cls_stage1), hipMemcpyHostToDevice));
    HIPT(hipMemcpy(d_cls2.p, ct_cls_stage2, sizeof(ct_cls_stage2), hipMemcpyHostToDevice));
    HIPT(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    HIPT(hipEventCreate(&ev0));
    HIPT(hipEventCreate(&ev1));
    ready = true;
  }

  pretok::Tables tables() const { return pretok::Tables{d_cls1.p, d_cls2.p, nullptr, nullptr, 0}; }  // (\d: the kernels' own)

  pretok::Step step_of(size_t i) const { return pretok::step_view(prog[i], parts[i], d_blob.p + at[i], max_run); }

  void ensure_bits(int w, uint64_t n) {
    inw[w].ensure(words64(n) + 1);
    beg[w].ensure(words64(n) + 1);
  }
  pretok::Ctx ctx(const State& c) const { return pretok::Ctx{c.text, c.n, inw[c.bits].p, beg[c.bits].p}; }

  State run_step(size_t i, const State& cur, uint64_t n_docs, int* text_w, hipStream_t s) {
    const pretok::Step st = step_of(i);
    const pretok::Tables T = tables();
    const pretok::Ctx x = ctx(cur);
    const uint64_t nw = words64(cur.n);
    const int nb = cur.bits ^ 1;
    if (!pretok::rewrites(st.kind)) {
      ensure_bits(nb, cur.n);
      ctok_pt::Scratch sc{};
      if (st.kind == pretok::K_SCRIPTS) {
        tail.ensure(ctok_pt::wave_tiles(cur.n) + 1);
        carry.ensure(ctok_pt::wave_tiles(cur.n) + 1);
        sc.tail = tail.p;
        sc.carry = carry.p;
      }
      if (st.kind == pretok::K_SPLIT && st.mode == pretok::M_LITERAL) {
        cand.ensure(cur.n + 1);
        mark.ensure(cur.n + 1);
        sc.cand = cand.p;
        sc.mark = mark.p;
      }
      const bool dfa = st.kind == pretok::K_SPLIT && st.mode == pretok::M_DFA && cur.n;
      if (dfa) {
        mark.ensure(cur.n + 1);
        mlen.ensure(cur.n + 1);
        tmax.ensure(ctok_pt::wave_tiles(cur.n) + 1);
        tcarry.ensure(ctok_pt::wave_tiles(cur.n) + 1);
        over.ensure(1);
        sc.mark = mark.p;
        sc.len = mlen.p;
        sc.tmax = tmax.p;
        sc.tcarry = tcarry.p;
        sc.over = over.p;
      }
      if (st.kind == pretok::K_SPLIT && st.mode != pretok::M_IDENTITY && (st.flags & 15u) == pretok::B_REMOVED && cur.n) {
        wpos.ensure(nw + 1);
        tmp.ensure(ctok_dev::scan_tmp_elems(nw + 1) + 64);
        uint64_t words = 0;
        HIPT(ctok_pt::count_begins(x, wpos.p, tmp.p, tmp.cap, &words, s));
        whit.ensure(words + 1);
        HIPT(hipMemsetAsync(whit.p, 0, words + 1, s));
        sc.wpos = wpos.p;
        sc.whit = whit.p;
      }
      HIPT(ctok_pt::launch_split(T, st, x, sc, Bits{inw[nb].p, beg[nb].p}, s));
      if (dfa) refuse_long_run(i, cur, n_docs, s);
      return State{cur.text, cur.off, cur.n, nb};
    }
    info.steps_rewriting++;
    len.ensure(nw + 1);
    uint64_t total = 0;
    if (cur.n) {
      HIPT(ctok_pt::launch_rw_count(T, st, x, len.p, s));
      tmp.ensure(ctok_dev::scan_tmp_elems(nw + 1) + 64);
      HIPT(ctok_dev::scan_u64(len.p, nw, tmp.p, tmp.cap, s));  // len[nw] = the total
      HIPT(hipMemcpyAsync(&total, len.p + nw, 8, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
    } else {
      HIPT(hipMemsetAsync(len.p, 0, 8, s));
    }
    if (total >= kRefuseFrom)
      throw_error(CTOK_E_CAPACITY, std::string("pre-tokenizer: the output of step ") + std::to_string(i) + " (" +
                                       pretok::kind_name(st.kind) + ") reaches 4 GiB");
    const int w = *text_w;
    *text_w ^= 1;
    buf[w].ensure(total + 16);
    flags.ensure(total + 16);
    off[w].ensure(n_docs + 1);
    ensure_bits(nb, total);
    HIPT(ctok_pt::launch_rw_write(T, st, x, len.p, cur.off, n_docs, buf[w].p, flags.p, off[w].p, s));
    HIPT(ctok_pt::launch_pack(flags.p, total, Bits{inw[nb].p, beg[nb].p}, s));
    return State{buf[w].p, off[w].p, total, nb};
  }

  // A start of step i's DFA passed the cap: CTOK_E_UNSUPPORTED naming the lowest-numbered such text.
  // (The step's bitmaps are scratch: nothing has reached the caller's buffers.)
  void refuse_long_run(size_t i, const State& cur, uint64_t n_docs, hipStream_t s) {
    uint32_t at_byte = 0;
    HIPT(hipMemcpyAsync(&at_byte, over.p, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (at_byte == 0xFFFFFFFFu) return;
    std::vector<uint64_t> h_off(n_docs + 1);
    HIPT(hipMemcpyAsync(h_off.data(), cur.off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    const uint64_t text = (uint64_t)(std::upper_bound(h_off.begin(), h_off.end(), (uint64_t)at_byte) - h_off.begin()) - 1;
    throw_error(CTOK_E_UNSUPPORTED, "pre-tokenizer step " + std::to_string(i) + ": text " + std::to_string(text) +
                                        " holds a word in which a match of the split pattern may run past " +
                                        std::to_string(max_run) + " code points, the cap of a pattern whose matches are unbounded");
  }

  // the words an empty text owns (once; a run of another handle on this handle's device)
  void prepare_fate() {
    if (fate_ready) return;
    fate = pretok::empty_fate(prog, &fate_at);
    if (fate == pretok::E_EMPTY_WORD) ew_off = {0, 0};
    if (fate == pretok::E_METASPACE) {
      ctok_pretokenizer sub;
      sub.device = device;
      for (size_t i = fate_at; i < prog.size(); i++) {
        sub.at.push_back(sub.blob.size());
        sub.parts.push_back(parts[i]);
        sub.blob += parts[i].bytes;
        sub.prog.push_back(prog[i]);
      }
      sub.prog[0].flags &= ~1u;  // (Metaspace with a prefix over "" is Metaspace without one over the replacement)
      const std::string& r = prog[fate_at].cp_u8;
      const uint64_t o[2] = {0, r.size()};
      // (the buffers are sized by the run's own counts: every Metaspace with a prefix adds a replacement)
      sub.upload_and_run((const uint8_t*)r.data(), o, 1);
      const uint64_t nb = sub.n_bytes, nwd = sub.n_words;
      std::vector<uint64_t> wo(nwd + 1);
      std::vector<uint8_t> by(nb + 1);
      uint64_t tw[2];
      sub.gather_to_host(1, by.data(), wo.data(), tw);
      ew_off.assign(wo.begin(), wo.begin() + nwd + 1);
      ew_bytes.assign(by.begin(), by.begin() + nb);
    }
    d_ew_off.ensure(ew_off.size());
    d_ew_bytes.ensure(ew_bytes.size() + 1);
    HIPT(hipMemcpy(d_ew_off.p, ew_off.data(), ew_off.size() * 8, hipMemcpyHostToDevice));
    if (!ew_bytes.empty()) HIPT(hipMemcpy(d_ew_bytes.p, ew_bytes.data(), ew_bytes.size(), hipMemcpyHostToDevice));
    fate_ready = true;
  }

  // The whole program over n_docs > 0 texts and the gather's counts: n_words, n_bytes.
  void run_steps(const uint8_t* text, const uint64_t* d_off, uint64_t n, uint64_t n_docs, hipStream_t s) {
    if (n >= kRefuseFrom || n_docs >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pre-tokenizer: the input reaches 4 GiB");
    prepare_fate();
    info = ctok_pretokenizer_info{};
    info.steps = prog.size();
    info.bytes_in = info.bytes_peak = n;
    ms.assign(prog.size() + 1, 0.0);
    ensure_bits(0, n);
    HIPT(ctok_pt::launch_init(n, d_off, n_docs, Bits{inw[0].p, beg[0].p}, s));
    n_empty = 0;
    if (fate != pretok::E_NOTHING) {
      // which texts are empty is read off the input's offsets, before any step: a text that loses all its
      // words on the way is not the empty word
      ex.ensure(n_docs + 1);
      tmp.ensure(ctok_dev::scan_tmp_elems(n_docs + 1) + 64);
      HIPT(ctok_pt::launch_empty(d_off, n_docs, ex.p, s));
      HIPT(ctok_dev::scan_u64(ex.p, n_docs, tmp.p, tmp.cap, s));  // ex[d] = empty texts before d, ex[n_docs] = all
      HIPT(hipMemcpyAsync(&n_empty, ex.p + n_docs, 8, hipMemcpyDeviceToHost, s));
    }
    State cur{text, d_off, n, 0};
    int text_w = 0;
    for (size_t i = 0; i < prog.size(); i++) {
      HIPT(hipEventRecord(ev0, s));
      cur = run_step(i, cur, n_docs, &text_w, s);
      if (cur.n > info.bytes_peak) info.bytes_peak = cur.n;
      HIPT(hipEventRecord(ev1, s));
      HIPT(hipEventSynchronize(ev1));
      float t = 0;
      HIPT(hipEventElapsedTime(&t, ev0, ev1));
      ms[i] = t;
    }
    HIPT(hipEventRecord(ev0, s));
    const uint64_t nw = words64(cur.n);
    cb.ensure(nw + 1);
    cw.ensure(nw + 1);
    uint64_t tot[2] = {0, 0};
    if (cur.n) {
      HIPT(ctok_pt::launch_gather_count(ctx(cur), cb.p, cw.p, s));
      tmp.ensure(ctok_dev::scan_tmp_elems(nw + 1) + 64);
      HIPT(ctok_dev::scan_u64(cb.p, nw, tmp.p, tmp.cap, s));
      HIPT(ctok_dev::scan_u64(cw.p, nw, tmp.p, tmp.cap, s));
      HIPT(hipMemcpyAsync(&tot[0], cb.p + nw, 8, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(&tot[1], cw.p + nw, 8, hipMemcpyDeviceToHost, s));
    } else {
      HIPT(hipMemsetAsync(cb.p, 0, 8, s));
      HIPT(hipMemsetAsync(cw.p, 0, 8, s));
    }
    HIPT(hipStreamSynchronize(s));
    n_bytes = tot[0] + n_empty * ew_bytes.size();
    n_words = tot[1] + n_empty * (ew_off.size() - 1);
    if (n_bytes >= kRefuseFrom || n_words >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pre-tokenizer: the words reach 4 GiB");
    last = cur;
    info.bytes_out = n_bytes;
    info.words = n_words;
  }

  // the gather's write, into device buffers of at least n_bytes, n_words + 1 and n_docs + 1 elements
  void gather(uint64_t n_docs, uint8_t* d_words, uint64_t* d_word_off, uint64_t* d_text_word, hipStream_t s) {
    ctok_pt::Gather g{};
    g.posb = cb.p;
    g.posw = cw.p;
    g.doc_off = last.off;
    g.n_docs = n_docs;
    g.ex = fate != pretok::E_NOTHING && n_empty ? ex.p : nullptr;
    g.ew = ew_off.size() - 1;
    g.eb = ew_bytes.size();
    g.ew_off = d_ew_off.p;
    g.ew_bytes = d_ew_bytes.p;
    g.n_words = n_words;
    g.n_bytes = n_bytes;
    g.words = d_words;
    g.word_off = d_word_off;
    g.text_word = d_text_word;
    HIPT(ctok_pt::launch_gather(ctx(last), g, s));
    HIPT(hipEventRecord(ev1, s));
    HIPT(hipEventSynchronize(ev1));
    float t = 0;
    HIPT(hipEventElapsedTime(&t, ev0, ev1));
    ms[prog.size()] = t;
  }

  // n_texts > 0 host texts through the program: leaves n_bytes and n_words, and the gather to do
  void upload_and_run(const uint8_t* utf8, const uint64_t* h_off, uint64_t n_texts) {
    check_utf8(utf8, h_off, n_texts);
    const uint64_t nb = h_off[n_texts];
    if (nb >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pre-tokenizer: the input reaches 4 GiB");
    prepare();
    in_text.ensure(nb + 16);
    in_off.ensure(n_texts + 1);
    if (nb) HIPT(hipMemcpyAsync(in_text.p, utf8, nb, hipMemcpyHostToDevice, own));
    HIPT(hipMemcpyAsync(in_off.p, h_off, (n_texts + 1) * 8, hipMemcpyHostToDevice, own));
    run_steps(in_text.p, in_off.p, nb, n_texts, own);
  }

  // the gather of upload_and_run's result into host buffers of n_bytes, n_words + 1 and n_texts + 1 elements
  void gather_to_host(uint64_t n_texts, uint8_t* words, uint64_t* word_off, uint64_t* text_word) {
    hipStream_t s = own;
    o_words.ensure(n_bytes + 1);
    o_woff.ensure(n_words + 1);
    o_tw.ensure(n_texts + 1);
    gather(n_texts, o_words.p, o_woff.p, o_tw.p, s);
    if (n_bytes) HIPT(hipMemcpyAsync(words, o_words.p, n_bytes, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(word_off, o_woff.p, (n_words + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(text_word, o_tw.p, (n_texts + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
  }

  void run_host(const uint8_t* utf8, const uint64_t* h_off, uint64_t n_texts, uint8_t* words, uint64_t words_cap,
                uint64_t* word_off, uint64_t word_cap, uint64_t* text_word, uint64_t* n_bytes_out, uint64_t* n_words_out) {
    upload_and_run(utf8, h_off, n_texts);
    *n_bytes_out = n_bytes;
    *n_words_out = n_words;
    if (n_bytes > words_cap || n_words > word_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_pretokenizer_run: the words need " + std::to_string(n_bytes) + " bytes and " +
                                       std::to_string(n_words) + " offsets");
    if ((n_bytes && !words) || !word_off) throw_error(CTOK_E_ARG, "null argument");
    gather_to_host(n_texts, words, word_off, text_word);
  }
};

extern "C" {

int ctok_pretokenizer_create(const ctok_pretok_step* steps, uint64_t n_steps, int device, ctok_pretokenizer** out) {
  return ctok_host::run_guarded([&] {
    if (!out || (n_steps && !steps)) throw_error(CTOK_E_ARG, "null argument");
    *out = nullptr;
    if (n_steps > CTOK_PRETOK_MAX_STEPS)
      throw_error(CTOK_E_UNSUPPORTED, "pre-tokenizer: more than " + std::to_string(CTOK_PRETOK_MAX_STEPS) + " steps");
    std::unique_ptr<ctok_pretokenizer> pt(new ctok_pretokenizer);
    pt->device = device;
    for (uint64_t i = 0; i < n_steps; i++) {
      if (steps[i].a_len && !steps[i].a) throw_error(CTOK_E_ARG, "null argument");
      pt->add_step(steps[i]);
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
      (void)hipGetLastError();
      throw_error(CTOK_E_DEVICE, "pre-tokenizer: no HIP device " + std::to_string(device));
    }
    *out = pt.release();
  });
}

void ctok_pretokenizer_destroy(ctok_pretokenizer* pt) { delete pt; }

int ctok_pretok_split_class(const uint8_t* pattern, uint64_t len) {
  const std::string p(pattern ? (const char*)pattern : "", pattern ? len : 0);
  if (!ctok_rt::rust_regex_rejects(p).empty()) return pretok::PC_REJECTED;
  return (int)pretok::classify_split(p, nullptr);
}

int ctok_pretok_split_plan(const uint8_t* pattern, uint64_t len, ctok_pretok_split_info* out) {
  return ctok_host::run_guarded([&] {
    if (!out || (len && !pattern)) throw_error(CTOK_E_ARG, "null argument");
    *out = ctok_pretok_split_info{};
    const std::string p(pattern ? (const char*)pattern : "", pattern ? len : 0);
    std::string why = ctok_rt::rust_regex_rejects(p);
    HostStep h;
    if (!why.empty()) {
      out->gate = pretok::PC_REJECTED;
      why = "the Rust regex crate rejects the pattern: " + why;
    } else {
      out->gate = (int32_t)pretok::plan_split(p, &h, &why);
    }
    if (out->gate == pretok::PC_DFA) {
      out->n_symbols = h.dfa.n_symbols;
      out->n_states = h.dfa.n_states;
      out->n_nfa = h.dfa.n_nfa;
      out->cyclic = h.dfa.cyclic ? 1 : 0;
      out->longest_match = h.dfa.longest;
      out->table_bytes = (uint64_t)h.dfa.trans.size() * 2;
      out->table_in_lds = out->table_bytes <= ctok_pt::kDfaLdsBytes ? 1 : 0;
    }
    snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
  });
}

int ctok_pretok_limits(ctok_pretok_limits_info* out) {
  return ctok_host::run_guarded([&] {
    if (!out) throw_error(CTOK_E_ARG, "null argument");
    *out = ctok_pretok_limits_info{};
    out->max_regex_run = ctok_rt::PretokKnobs().max_regex_run;
    out->max_symbols = regex_dfa::kMaxSymbols;
    out->max_states = regex_dfa::kMaxStates;
    out->max_nfa_states = regex_dfa::kMaxNfa;
    out->lds_table_bytes = ctok_pt::kDfaLdsBytes;
    out->scan_tile_bytes = ctok_pt::kWaveTile;
    out->scan_round_bytes = (uint64_t)ctok_pt::kWaveTile * ctok_pt::kThreads;
  });
}

int ctok_pretokenizer_run(ctok_pretokenizer* pt, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, uint8_t* words,
                          uint64_t words_cap, uint64_t* word_off, uint64_t word_cap, uint64_t* text_word,
                          uint64_t* n_bytes_out, uint64_t* n_words_out) {
  return ctok_host::run_guarded([&] {
    if (!pt || !text_word || !n_bytes_out || !n_words_out || (n_texts && (!off || (off[n_texts] && !utf8))))
      throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = *n_words_out = 0;
    if (!n_texts) {
      text_word[0] = 0;
      if (word_off) word_off[0] = 0;
      return;
    }
    pt->run_host(utf8, off, n_texts, words, words_cap, word_off, word_cap, text_word, n_bytes_out, n_words_out);
  });
}

int ctok_pretokenizer_run_device(ctok_pretokenizer* pt, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_texts,
                                 uint64_t n_bytes, uint8_t* d_words, uint64_t words_cap, uint64_t* d_word_off,
                                 uint64_t word_cap, uint64_t* d_text_word, uint64_t* n_bytes_out, uint64_t* n_words_out,
                                 void* stream) {
  return ctok_host::run_guarded([&] {
    if (!pt || !d_text_word || !d_word_off || !n_bytes_out || !n_words_out || (n_texts && !d_off) || (n_bytes && !d_utf8))
      throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = *n_words_out = 0;
    pt->prepare();
    hipStream_t s = (hipStream_t)stream;
    if (!n_texts) {
      HIPT(hipMemsetAsync(d_text_word, 0, 8, s));
      HIPT(hipMemsetAsync(d_word_off, 0, 8, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    pt->run_steps(d_utf8, d_off, n_bytes, n_texts, s);
    *n_bytes_out = pt->n_bytes;
    *n_words_out = pt->n_words;
    if (pt->n_bytes > words_cap || pt->n_words > word_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_pretokenizer_run_device: the words need " + std::to_string(pt->n_bytes) +
                                       " bytes and " + std::to_string(pt->n_words) + " offsets");
    if (pt->n_bytes && !d_words) throw_error(CTOK_E_ARG, "null argument");
    pt->gather(n_texts, d_words, d_word_off, d_text_word, s);
    HIPT(hipStreamSynchronize(s));
  });
}

int ctok_pretokenizer_stage_ms(const ctok_pretokenizer* pt, double* ms, uint64_t cap, uint64_t* n) {
  return ctok_host::run_guarded([&] {
    if (!pt || !n || (cap && !ms)) throw_error(CTOK_E_ARG, "null argument");
    *n = pt->prog.size() + 1;
    for (uint64_t i = 0; i < cap && i < *n; i++) ms[i] = i < pt->ms.size() ? pt->ms[i] : 0.0;
  });
}

const char* ctok_pretokenizer_stage_name(const ctok_pretokenizer* pt, uint64_t i) {
  if (!pt || i > pt->prog.size()) return "";
  return i == pt->prog.size() ? "gather" : pretok::kind_name(pt->prog[i].kind);
}

int ctok_pretokenizer_stats(const ctok_pretokenizer* pt, ctok_pretokenizer_info* out) {
  return ctok_host::run_guarded([&] {
    if (!pt || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = pt->info;
  });
}

}  // extern "C"
