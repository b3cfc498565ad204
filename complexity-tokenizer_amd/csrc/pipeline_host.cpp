// Host runtime of the pipeline tokenizer behind include/ctok_pipeline.h: the reference's
// HuggingFaceTokenizer (src/huggingface/mod.rs:247-334, :551-613, :1080-1101, Complexity-ML/
// complexity-tokenizer v0.3.3) with any normaliser and pre-tokenizer.  wordbpe_compile.cpp turns
// vocab, merges and added tokens into tables at create; a call chains, on one stream and without a
// trip through host memory,
//   ctok_normalizer_run_device -> ctok_pretokenizer_run_device -> the id-keyed word BPE (wordbpe.hip):
//   segments -> symbols -> merges -> emit
// The buffers only grow.  A component that reports CTOK_E_CAPACITY gets the size it asked for and
// runs once more.  Every count is read back before the stage that is sized by it runs, so a segment
// above the cap, a flagged word above the work bound and a batch that reaches 4 GiB fail the call
// before any merge kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_pipeline.h"
#include "ctok_internal.h"  // ctok_dev::scan_u32, scan_tmp_elems
#include "gen/alnum_data.h"
#include "host_common.h"
#include "knobs.h"
#include "pipeline_enc_internal.h"
#include "pipeline_win_internal.h"
#include "train_host_common.h"
#include "wordbpe_compile.h"
#include "wordbpe_internal.h"

using namespace ctok_wb;
using ctok_host::throw_error;
using ctok_train_host::DBuf;

static_assert(wordbpe::kErrUnsupported == CTOK_E_UNSUPPORTED && wordbpe::kErrArg == CTOK_E_ARG &&
                  wordbpe::kErrCapacity == CTOK_E_CAPACITY,
              "wordbpe_compile.h repeats the codes of ctok.h");

namespace {

constexpr uint64_t kRefuseFrom = 0xFFFFFF00ull;  // bytes, words or texts of one call: 4 GiB less the slack of the u32 scans

const char* const kStageNames[CTOK_PIPELINE_STAGES] = {"normalize", "pre_tokenize", "segments", "symbols", "merges", "emit"};

const char* const kEncStageNames[CTOK_PIPELINE_ENCODING_STAGES] = {"find", "spans", "rows"};

const char* const kWinStageNames[CTOK_PIPELINE_WINDOW_STAGES] = {"plan", "write"};

uint64_t find_work_cap() {
  uint64_t cap = ctok_pe::kMaxFindWork;
  if (auto e = ctok_rt::env_u64("CTOK_PIPELINE_MAX_FIND_WORK")) cap = std::min<uint64_t>(cap, *e);
  return cap;
}

uint64_t word_cap() {
  uint64_t cap = kMaxWordSymbols;
  if (auto e = ctok_rt::env_u64("CTOK_PIPELINE_MAX_WORD_SYMBOLS")) cap = std::min<uint64_t>(cap, *e);
  return cap;
}

template <typename T>
void upload(DBuf<T>& d, const T* src, size_t n, hipStream_t s) {
  d.ensure(n + 1);
  if (n) HIPT(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
}

// a component's error, with its message, as this call's
[[noreturn]] void rethrow(int rc) { throw_error(rc, std::string(ctok_last_error())); }

bool valid_utf8(const uint8_t* t, uint64_t a, uint64_t e) {
  while (a < e) {
    uint32_t cp = 0;
    const uint32_t l = wordbpe::dec_char(t, a, e, &cp);
    if (!l) return false;
    a += l;
  }
  return true;
}

}  // namespace

struct ctok_pipeline {
  wordbpe::Compiled c;
  ctok_normalizer* nz = nullptr;
  ctok_pretokenizer* pt = nullptr;
  int device = 0;
  uint64_t cap = kMaxWordSymbols;
  uint64_t flag_cap = kMaxFlaggedWordBytes;  // of this handle's added tokens (wordbpe_internal.h)
  uint64_t match_cap = ~0ull;                // bytes of a batch the filter pass takes
  hipStream_t own = nullptr;
  hipEvent_t ev[CTOK_PIPELINE_STAGES + 1] = {};
  hipEvent_t ev_merge = nullptr;  // the merges begin: after the counts of the symbols stage came back
  double stage_ms[CTOK_PIPELINE_STAGES] = {};
  ctok_pipeline_info info{};
  // the Encoding path (pipeline_enc.hip)
  uint64_t find_cap = ctok_pe::kMaxFindWork;
  hipEvent_t ev_enc[2 * CTOK_PIPELINE_ENCODING_STAGES] = {};  // begin and end of find, spans, rows
  double enc_ms[CTOK_PIPELINE_ENCODING_STAGES] = {};
  ctok_pipeline_encoding_info enc_info{};
  std::vector<uint32_t> len_id, len_val, special_id;  // id -> bytes of its vocab string; the special added tokens' ids
  DBuf<uint32_t> d_len_id, d_len_val, d_special;
  DBuf<uint64_t> wstart, wend, work, rep, lens, tmp64, e_off, e_seq_off, e_na, e_row_off;
  DBuf<uint32_t> e_wids, e_out, e_type, e_spec;
  std::vector<uint8_t> h_text;
  std::vector<uint64_t> h_off, h_row_off, h_seq_off, h_na, h_offsets;
  std::vector<uint32_t> h_out, h_type, h_spec, h_wids, h_seq_ids;
  // padded batches and stride windows (pipeline_win.hip)
  uint32_t default_pad_id = 0;  // the reference's choice: [PAD], then <pad>, then 0 (mod.rs:505-510)
  hipEvent_t ev_win[2 * CTOK_PIPELINE_WINDOW_STAGES] = {};  // begin and end of plan, write
  double win_ms[CTOK_PIPELINE_WINDOW_STAGES] = {};
  ctok_pipeline_window_info win_info{};
  DBuf<uint64_t> w_row_win, w_rep, w_len, w_start, w_off_len, w_seq_len, w_offsets;
  DBuf<uint32_t> w_tokenless, w_row, w_ids, w_attn, w_type, w_spec, w_word, w_seq;
  std::vector<uint64_t> hw_row_win, hw_len, hw_start, hw_off_len, hw_seq_len, hw_offsets;
  std::vector<uint32_t> hw_row, hw_ids, hw_attn, hw_type, hw_spec, hw_word, hw_seq;
  // the tables
  DBuf<wordbpe::CpSlot> d_cps;
  DBuf<strmerge::PairSlot> d_pairs;
  DBuf<uint8_t> d_abytes;
  DBuf<uint32_t> d_aoff, d_aid, d_aflags, d_agroup, d_alo, d_ahi;
  Tables T{};
  // a call's buffers
  DBuf<uint8_t> in_text, norm, words;
  DBuf<uint64_t> in_off, norm_off, word_off, text_word, tok_off, state3;
  DBuf<uint32_t> wbits, mbits, kbits, kpc, krank, wseg, segoff, nsym, soff, fcnt, wpos, sym, list2, list3, state, ctr, tmp, ids;
  DBuf<wordbpe::Seg> segs;
  Batch B{};
  uint32_t n2 = 0, n3 = 0, n_sym_run = 0;  // between the two phases of a run
  uint64_t n_state = 0;
  uint64_t n_ids = 0;
  std::vector<uint32_t> h_ids;
  std::vector<uint64_t> h_tok_off;

  ~ctok_pipeline() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_enc)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_win)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_rec)
      if (e) (void)hipEventDestroy(e);
    if (ev_merge) (void)hipEventDestroy(ev_merge);
    if (own) (void)hipStreamDestroy(own);
  }

  void to_device() {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
      (void)hipGetLastError();
      throw_error(CTOK_E_DEVICE, "pipeline: no HIP device " + std::to_string(device));
    }
    HIPT(hipSetDevice(device));
    HIPT(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    for (auto& e : ev) HIPT(hipEventCreate(&e));
    for (auto& e : ev_enc) HIPT(hipEventCreate(&e));
    for (auto& e : ev_win) HIPT(hipEventCreate(&e));
    for (auto& e : ev_rec) HIPT(hipEventCreate(&e));
    HIPT(hipEventCreate(&ev_merge));
    upload(d_len_id, len_id.data(), len_id.size(), own);
    upload(d_len_val, len_val.data(), len_val.size(), own);
    upload(d_special, special_id.data(), special_id.size(), own);
    upload(d_cps, c.cps.data(), c.cps.size(), own);
    upload(d_pairs, c.pairs.data(), c.pairs.size(), own);
    upload(d_abytes, c.a_bytes.data(), c.a_bytes.size(), own);
    upload(d_aoff, c.a_off.data(), c.a_off.size(), own);
    upload(d_aid, c.a_id.data(), c.a_id.size(), own);
    upload(d_aflags, c.a_flags.data(), c.a_flags.size(), own);
    upload(d_agroup, c.a_group.data(), c.a_group.size(), own);
    upload(d_alo, wb_alnum_lo, (size_t)WB_N_ALNUM, own);
    upload(d_ahi, wb_alnum_hi, (size_t)WB_N_ALNUM, own);
    HIPT(hipStreamSynchronize(own));
    T.pairs = wordbpe::PairView{d_pairs.p, (uint32_t)c.pairs.size() - 1};
    T.cps = wordbpe::CpView{d_cps.p, (uint32_t)c.cps.size() - 1};
    T.added = wordbpe::AddedView{d_abytes.p, d_aoff.p, d_aid.p, d_aflags.p, d_agroup.p, d_alo.p, d_ahi.p, (uint32_t)WB_N_ALNUM,
                                 (uint32_t)c.a_id.size()};
    for (int i = 0; i < 8; i++) T.first_byte[i] = c.first_byte[i];
    if (c.max_group_bytes) {
      flag_cap = std::min<uint64_t>(kMaxFlaggedWordBytes, kFlaggedWork / c.max_group_bytes);
      match_cap = kMatchWork / c.max_group_bytes;
    }
  }

  void scan(const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t s) {  // out[n] = the total
    tmp.ensure(ctok_dev::scan_tmp_elems(n + 1) + 64);
    if (n) HIPT(ctok_dev::scan_u32(in, out, n, nullptr, tmp.p, tmp.cap, s));
    else HIPT(hipMemsetAsync(out, 0, 4, s));
  }

  uint32_t read_u32(const uint32_t* d, hipStream_t s) {
    uint32_t v = 0;
    HIPT(hipMemcpyAsync(&v, d, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    return v;
  }

  // Everything up to the count of the ids (n_ids); emit() writes them.  n > 0.
  void run(const uint8_t* d_text, const uint64_t* d_off, uint64_t n, uint64_t nb, uint32_t flags, hipStream_t s) {
    run_words(d_text, d_off, n, nb, flags, s);
    run_merges(s, nullptr);
  }

  // The first phase: the words, their segments and symbols, and every refusal of a segment's size.
  void run_words(const uint8_t* d_text, const uint64_t* d_off, uint64_t n, uint64_t nb, uint32_t flags, hipStream_t s) {
    HIPT(hipSetDevice(device));
    for (double& t : stage_ms) t = 0;
    info = ctok_pipeline_info{};
    info.texts = n;
    info.bytes_in = nb;
    if (nb >= kRefuseFrom || n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pipeline: the input reaches 4 GiB");

    // 1. the normaliser
    HIPT(hipEventRecord(ev[0], s));
    const uint8_t* text = d_text;
    const uint64_t* off = d_off;
    uint64_t tb = nb;
    if (nz) {
      norm.ensure(nb + 64);
      norm_off.ensure(n + 1);
      uint64_t need = 0;
      int rc = ctok_normalizer_run_device(nz, d_text, d_off, n, nb, norm.p, norm.cap, norm_off.p, &need, s);
      if (rc == CTOK_E_CAPACITY && need > norm.cap && need < kRefuseFrom) {
        norm.ensure(need + 64);
        rc = ctok_normalizer_run_device(nz, d_text, d_off, n, nb, norm.p, norm.cap, norm_off.p, &need, s);
      }
      if (rc) rethrow(rc);
      text = norm.p;
      off = norm_off.p;
      tb = need;
    }
    info.bytes_normalized = tb;
    HIPT(hipEventRecord(ev[1], s));

    // 2. the pre-tokenizer; without one the whole normalised text is one word
    const uint8_t* wtext = text;
    const uint64_t* woff = off;
    uint64_t wbytes = tb, n_words = n;
    text_word.ensure(n + 1);
    if (pt) {
      words.ensure(tb + 64);
      word_off.ensure(tb / 2 + n + 65);
      uint64_t need_b = 0, need_w = 0;
      int rc = ctok_pretokenizer_run_device(pt, text, off, n, tb, words.p, words.cap, word_off.p, word_off.cap - 1, text_word.p,
                                            &need_b, &need_w, s);
      if (rc == CTOK_E_CAPACITY && (need_b > words.cap || need_w > word_off.cap - 1) && need_b < kRefuseFrom && need_w < kRefuseFrom) {
        words.ensure(need_b + 64);
        word_off.ensure(need_w + 65);
        rc = ctok_pretokenizer_run_device(pt, text, off, n, tb, words.p, words.cap, word_off.p, word_off.cap - 1, text_word.p,
                                          &need_b, &need_w, s);
      }
      if (rc) rethrow(rc);
      wtext = words.p;
      woff = word_off.p;
      wbytes = need_b;
      n_words = need_w;
    } else {
      HIPT(launch_iota(text_word.p, n + 1, s));
    }
    if (wbytes + n_words >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pipeline: the words reach 4 GiB");
    info.bytes_words = wbytes;
    info.words = n_words;
    HIPT(hipEventRecord(ev[2], s));

    // 3. the segments
    const uint32_t n_w = (uint32_t)((wbytes + 31) / 32);
    const bool with_added = !c.a_id.empty() && !(flags & CTOK_PIPELINE_TOKENIZE);
    wbits.ensure((size_t)n_w + 1);
    ctr.ensure(kNumCtr);
    HIPT(hipMemsetAsync(wbits.p, 0, ((size_t)n_w + 1) * 4, s));
    HIPT(hipMemsetAsync(ctr.p, 0, kNumCtr * 4, s));
    HIPT(hipMemsetAsync(ctr.p + kCtrPanic, 0xFF, 4, s));
    B = Batch{};
    B.text = wtext;
    B.n_bytes = (uint32_t)wbytes;
    B.n_w = n_w;
    B.word_off = woff;
    B.n_words = (uint32_t)n_words;
    B.text_word = text_word.p;
    B.n_texts = n;
    B.wbits = wbits.p;
    B.ctr = ctr.p;
    B.flag_cap = (uint32_t)flag_cap;
    if (with_added && wbytes > match_cap)
      throw_error(CTOK_E_UNSUPPORTED, "a batch of " + std::to_string(wbytes) + " bytes of words: the added tokens that share a "
                                          "first byte hold " + std::to_string(c.max_group_bytes) + " bytes, and with them batches of more than " +
                                          std::to_string(match_cap) + " bytes are not supported");
    HIPT(launch_word_bits(B, s));
    uint32_t n_segs = (uint32_t)n_words;
    if (with_added) {
      mbits.ensure((size_t)n_w + 1);
      wseg.ensure(n_words + 1);
      segoff.ensure(n_words + 1);
      B.mbits = mbits.p;
      B.wseg = wseg.p;
      HIPT(launch_match_bits(T, B, s));
      HIPT(launch_seg_count(T, B, s));
      scan(wseg.p, segoff.p, n_words, s);
      B.segoff = segoff.p;
      uint32_t h_ctr[kNumCtr] = {};
      HIPT(hipMemcpyAsync(h_ctr, ctr.p, kNumCtr * 4, hipMemcpyDeviceToHost, s));
      n_segs = read_u32(segoff.p + n_words, s);
      if (h_ctr[kCtrMaxFlagged])
        throw_error(CTOK_E_UNSUPPORTED, "a word of " + std::to_string(h_ctr[kCtrMaxFlagged]) +
                                            " bytes holds an added token: one thread walks such a word, words of more than " +
                                            std::to_string(flag_cap) + " bytes are not supported with these added tokens");
      if (n_segs > wbytes + n_words) throw_error(CTOK_E_DEVICE, "pipeline: more segments than bytes");
    }
    segs.ensure((size_t)n_segs + 1);
    B.segs = segs.p;
    B.n_segs = n_segs;
    HIPT(launch_seg_write(T, B, s));
    info.segments = n_segs;
    HIPT(hipEventRecord(ev[3], s));

    // 4. the initial symbols, the segments' sizes and classes
    kbits.ensure((size_t)n_w + 1);
    kpc.ensure((size_t)n_w + 1);
    krank.ensure((size_t)n_w + 2);
    B.kbits = kbits.p;
    B.kpc = kpc.p;
    B.krank = krank.p;
    HIPT(launch_keep_bits(T, B, s));
    scan(kpc.p, krank.p, (uint64_t)n_w + 1, s);
    const uint32_t n_sym = read_u32(krank.p + n_w + 1, s);
    if (n_sym > wbytes) throw_error(CTOK_E_DEVICE, "pipeline: more symbols than bytes");
    sym.ensure((size_t)n_sym + 1);
    nsym.ensure((size_t)n_segs + 1);
    soff.ensure((size_t)n_segs + 1);
    fcnt.ensure((size_t)n_segs + 1);
    wpos.ensure((size_t)n_segs + 1);
    // a segment of more than kTier1 symbols has more than kTier1 bytes, one of more than kTier2 more than kTier2
    const uint64_t cap2 = wbytes / kTier1 + 1, cap3 = wbytes / kTier2 + 1;
    list2.ensure(cap2);
    list3.ensure(cap3);
    state3.ensure(cap3);
    B.sym = sym.p;
    B.nsym = nsym.p;
    B.soff = soff.p;
    B.fcnt = fcnt.p;
    B.wpos = wpos.p;
    B.list2 = list2.p;
    B.list3 = list3.p;
    B.state3 = state3.p;
    HIPT(launch_symbols(T, B, s));
    HIPT(launch_seg_info(B, s));
    HIPT(hipEventRecord(ev[4], s));
    uint32_t h_ctr[kNumCtr] = {};
    HIPT(hipMemcpyAsync(h_ctr, ctr.p, kNumCtr * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    n2 = h_ctr[kCtrList2], n3 = h_ctr[kCtrList3];
    n_state = (uint64_t)h_ctr[kCtrState] | (uint64_t)h_ctr[kCtrState + 1] << 32;
    n_sym_run = n_sym;
    if (n2 > cap2 || n3 > cap3 || n_state > n_sym) throw_error(CTOK_E_DEVICE, "pipeline: the segment list is out of bounds");
    info.symbols = n_sym;
    info.tier2_segments = n2;
    info.tier3_segments = n3;
    info.max_segment_symbols = h_ctr[kCtrMaxSym];
    if (h_ctr[kCtrMaxSym] > cap)
      throw_error(CTOK_E_UNSUPPORTED, "a word of " + std::to_string(h_ctr[kCtrMaxSym]) + " symbols: the merge loop is quadratic "
                                          "in a word's length, words of more than " + std::to_string(cap) +
                                          " symbols are not supported");
  }

  // The second phase: the merges and the count of the ids.  before_panic (may be null) sees the segment of
  // a merge panic before it is reported, and may report something that comes first instead.
  void run_merges(hipStream_t s, const std::function<void(uint32_t)>* before_panic) {
    const uint32_t n_segs = B.n_segs, n_sym = n_sym_run;
    // 5. the merges
    HIPT(hipEventRecord(ev_merge, s));
    state.ensure(4 * n_state + 1);
    B.state = state.p;
    HIPT(launch_merge(T, B, n2, n3, s));
    scan(fcnt.p, wpos.p, n_segs, s);
    HIPT(hipEventRecord(ev[5], s));
    const uint32_t panic_seg = read_u32(ctr.p + kCtrPanic, s);
    if (panic_seg != wordbpe::kNoPanic) {
      if (panic_seg >= n_segs) throw_error(CTOK_E_DEVICE, "pipeline: the panic report is out of bounds");
      const uint32_t at = read_u32(soff.p + panic_seg, s);
      if (at >= n_sym) throw_error(CTOK_E_DEVICE, "pipeline: the panic report is out of bounds");
      const uint32_t rank = read_u32(sym.p + at, s);
      if (before_panic) (*before_panic)(panic_seg);
      throw_error(CTOK_E_PANIC, "index out of bounds: the len is " + std::to_string(c.n_filtered) + " but the index is " +
                                    std::to_string(rank));
    }
    n_ids = read_u32(wpos.p + n_segs, s);
    if (n_ids > (uint64_t)n_sym + n_segs) throw_error(CTOK_E_DEVICE, "pipeline: more ids than symbols");
    info.ids = n_ids;
  }

  void emit(uint32_t* d_ids, uint64_t* d_tok_off, hipStream_t s) {
    HIPT(launch_emit(B, d_ids, d_tok_off, s));
    HIPT(hipEventRecord(ev[6], s));
    HIPT(hipStreamSynchronize(s));
    for (int i = 0; i < CTOK_PIPELINE_STAGES; i++) {
      float ms = 0;
      HIPT(hipEventElapsedTime(&ms, i == 4 ? ev_merge : ev[i], ev[i + 1]));
      stage_ms[i] = ms;
    }
  }

  // ---- the Encoding path (include/ctok_pipeline.h, "Encodings") ----------------------------------------
  uint64_t h_rep0[ctok_pe::kNumRep] = {ctok_pe::kNoPanic, 0, ~0ull, ~0ull, ~0ull};
  uint64_t n_cells = 0;
  const uint32_t* r_ids = nullptr;      // the processed ids and their rows: the post-processor's, or the ids as they are
  const uint64_t* r_row_off = nullptr;

  [[noreturn]] static void throw_boundary(uint64_t report) {
    throw_error(CTOK_E_PANIC, "byte index " + std::to_string(report & 0xFFFFFFFFull) + " is not a char boundary");
  }

  // n_rows * per_row sequences (row r: sequences r * per_row ..) through tokenize, the word search, the
  // token spans, the post-processor and the row masks.  Everything stays in the handle's buffers.  The
  // errors in order: the refusals (4 GiB, word symbols, find work), then of the panics the lowest
  // sequence's, the char boundary before the merge, and the subtraction last.  n_rows > 0.
  void encodings(const uint8_t* d_text, const uint64_t* d_off, uint64_t n_rows, uint32_t per_row, uint64_t nb, ctok_postprocessor* pp,
                 hipStream_t s) {
    using namespace ctok_pe;
    const uint64_t n = n_rows * per_row;
    for (double& t : enc_ms) t = 0;
    enc_info = ctok_pipeline_encoding_info{};
    enc_info.rows = n_rows;
    enc_info.sequences = n;
    run_words(d_text, d_off, n, nb, CTOK_PIPELINE_TOKENIZE, s);
    const uint64_t n_words = B.n_words;
    if (B.n_segs != n_words) throw_error(CTOK_E_DEVICE, "pipeline: tokenize has a segment per word");
    enc_info.words = n_words;

    // the words' spans
    wstart.ensure(n_words + 1);
    wend.ensure(n_words + 1);
    work.ensure(n + 1);
    rep.ensure(kNumRep);
    HIPT(hipMemcpyAsync(rep.p, h_rep0, sizeof(h_rep0), hipMemcpyHostToDevice, s));
    const Find f{d_text, d_off, n, B.text, B.word_off, B.text_word, n_words, wstart.p, wend.p, work.p, (unsigned long long*)rep.p, find_cap,
                 find_cap / kFindCompareShare};
    HIPT(hipEventRecord(ev_enc[0], s));
    HIPT(launch_word_find(f, s));
    HIPT(hipEventRecord(ev_enc[1], s));
    uint64_t h_rep[kNumRep] = {};
    HIPT(hipMemcpyAsync(h_rep, rep.p, sizeof(h_rep), hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    enc_info.max_find_work = h_rep[kRepMaxWork];
    if (h_rep[kRepOver] != ~0ull) {
      const uint64_t q = h_rep[kRepOver];
      if (q >= n) throw_error(CTOK_E_DEVICE, "pipeline: the work report is out of bounds");
      uint64_t w = 0;
      HIPT(hipMemcpyAsync(&w, work.p + q, 8, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      throw_error(CTOK_E_UNSUPPORTED, "sequence " + std::to_string(q) + " (row " + std::to_string(q / per_row) +
                                          (per_row == 2 ? (q & 1 ? ", the pair" : ", the text") : "") + "): the search for its words' offsets has work " +
                                          std::to_string(w) + ", one wavefront walks a sequence and a word that is not found scans to the text's end; "
                                          "work of more than " + std::to_string(find_cap) + " is not supported");
    }
    if (h_rep[kRepCompares] != ~0ull) {
      const uint64_t q = h_rep[kRepCompares];
      throw_error(CTOK_E_UNSUPPORTED, "sequence " + std::to_string(q) + " (row " + std::to_string(q / per_row) +
                                          (per_row == 2 ? (q & 1 ? ", the pair" : ", the text") : "") +
                                          "): the search for its words' offsets compares more than " +
                                          std::to_string(find_cap / kFindCompareShare) +
                                          " bytes of partial matches at one position in 64, which is not supported");
    }
    const uint64_t find_panic = h_rep[kRepPanic];
    if (find_panic != kNoPanic && (find_panic >> 32) >= n) throw_error(CTOK_E_DEVICE, "pipeline: the panic report is out of bounds");

    // the merges; a merge panic is reported unless the char-boundary panic is the same or a lower sequence's
    const std::function<void(uint32_t)> before_merge_panic = [&](uint32_t word) {
      if (find_panic == kNoPanic) return;
      std::vector<uint64_t> tw(n + 1);
      HIPT(hipMemcpyAsync(tw.data(), B.text_word, (n + 1) * 8, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      const uint64_t q = (uint64_t)(std::upper_bound(tw.begin(), tw.end(), (uint64_t)word) - tw.begin()) - 1;
      if ((find_panic >> 32) <= q) throw_boundary(find_panic);
    };
    run_merges(s, &before_merge_panic);
    if (find_panic != kNoPanic) throw_boundary(find_panic);
    ids.ensure(n_ids + 1);
    tok_off.ensure(n + 1);
    emit(ids.p, tok_off.p, s);
    enc_info.ids = n_ids;

    // the token spans
    lens.ensure(n_ids + 2);
    e_off.ensure(2 * n_ids + 2);
    e_wids.ensure(n_ids + 1);
    tmp64.ensure(ctok_dev::scan_tmp_elems(n_ids + 1) + 64);
    const Spans sp{ids.p, n_ids, lens.p, d_len_id.p, d_len_val.p, (uint32_t)len_id.size(), wpos.p, (uint32_t)n_words, B.text_word, n,
                   wstart.p, wend.p, e_off.p, e_wids.p};
    HIPT(hipEventRecord(ev_enc[2], s));
    HIPT(launch_tok_len(sp, s));
    if (n_ids) HIPT(ctok_dev::scan_u64(lens.p, n_ids, tmp64.p, tmp64.cap, s));
    HIPT(launch_tok_spans(sp, s));
    HIPT(hipEventRecord(ev_enc[3], s));

    // the rows
    e_seq_off.ensure(n_rows + 1);
    e_na.ensure(n_rows + 1);
    Rows r{};
    r.tok_off = tok_off.p;
    r.per_row = per_row;
    r.n_rows = n_rows;
    r.seq_off = e_seq_off.p;
    r.n_a = e_na.p;
    r.special = d_special.p;
    r.n_special = (uint32_t)special_id.size();
    r.rep = (unsigned long long*)rep.p;
    HIPT(hipEventRecord(ev_enc[4], s));
    HIPT(launch_row_heads(r, s));
    r_ids = ids.p;
    r_row_off = e_seq_off.p;
    n_cells = n_ids;
    if (pp) {
      e_row_off.ensure(n_rows + 1);
      e_out.ensure(n_ids + 4 * n_rows + 64);
      ctok_pp_batch in{};
      in.ids = ids.p;
      in.off = e_seq_off.p;
      in.n_rows = n_rows;
      uint64_t need = 0;
      int rc = ctok_postprocessor_run_device(pp, &in, n_ids, 0, nullptr, e_out.p, e_out.cap, e_row_off.p, &need, s);
      if (rc == CTOK_E_CAPACITY && need > e_out.cap) {
        e_out.ensure(need + 1);
        rc = ctok_postprocessor_run_device(pp, &in, n_ids, 0, nullptr, e_out.p, e_out.cap, e_row_off.p, &need, s);
      }
      if (rc) rethrow(rc);
      r_ids = e_out.p;
      r_row_off = e_row_off.p;
      n_cells = need;
    }
    enc_info.cells = n_cells;
    e_type.ensure(n_cells + 1);
    e_spec.ensure(n_cells + 1);
    r.out_ids = r_ids;
    r.row_off = r_row_off;
    r.n_cells = n_cells;
    r.type_ids = e_type.p;
    r.special_mask = e_spec.p;
    HIPT(launch_enc_rows(r, s));
    HIPT(hipEventRecord(ev_enc[5], s));
    uint64_t short_row = 0;
    HIPT(hipMemcpyAsync(&short_row, rep.p + kRepShort, 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    for (int i = 0; i < CTOK_PIPELINE_ENCODING_STAGES; i++) {
      float ms = 0;
      HIPT(hipEventElapsedTime(&ms, ev_enc[2 * i], ev_enc[2 * i + 1]));
      enc_ms[i] = ms;
    }
    if (short_row != ~0ull) throw_error(CTOK_E_PANIC, "attempt to subtract with overflow");
  }

  // Host texts (and pair texts) checked and copied to in_text / in_off, the sequences in row order: 2r is
  // row r's text, 2r + 1 its pair.  Returns the bytes.  n_rows > 0.
  uint64_t upload_rows(const uint8_t* utf8, const uint64_t* off, uint64_t n_rows, const uint8_t* pair_utf8, const uint64_t* pair_off) {
    if (off[0] != 0 || (pair_off && pair_off[0] != 0)) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n_rows; i++) {
      if (off[i] > off[i + 1] || (pair_off && pair_off[i] > pair_off[i + 1])) throw_error(CTOK_E_ARG, "offsets must not decrease");
      if (!valid_utf8(utf8, off[i], off[i + 1])) throw_error(CTOK_E_ARG, "text " + std::to_string(i) + " is not UTF-8");
      if (pair_off && !valid_utf8(pair_utf8, pair_off[i], pair_off[i + 1]))
        throw_error(CTOK_E_ARG, "pair text " + std::to_string(i) + " is not UTF-8");
    }
    const uint64_t nb = off[n_rows] + (pair_off ? pair_off[n_rows] : 0), n = n_rows * (pair_off ? 2 : 1);
    if (nb >= kRefuseFrom || n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pipeline: the input reaches 4 GiB");
    const uint8_t* text = utf8;
    const uint64_t* toff = off;
    if (pair_off) {
      h_text.resize(nb);
      h_off.resize(n + 1);
      uint64_t at = 0;
      for (uint64_t i = 0; i < n_rows; i++) {
        h_off[2 * i] = at;
        if (off[i + 1] > off[i]) std::copy(utf8 + off[i], utf8 + off[i + 1], h_text.begin() + at);
        at += off[i + 1] - off[i];
        h_off[2 * i + 1] = at;
        if (pair_off[i + 1] > pair_off[i]) std::copy(pair_utf8 + pair_off[i], pair_utf8 + pair_off[i + 1], h_text.begin() + at);
        at += pair_off[i + 1] - pair_off[i];
      }
      h_off[n] = at;
      text = h_text.data();
      toff = h_off.data();
    }
    HIPT(hipSetDevice(device));
    in_text.ensure(nb + 64);
    in_off.ensure(n + 1);
    if (nb) HIPT(hipMemcpyAsync(in_text.p, text, nb, hipMemcpyHostToDevice, own));
    HIPT(hipMemcpyAsync(in_off.p, toff, (n + 1) * 8, hipMemcpyHostToDevice, own));
    return nb;
  }

  // ---- padded batches and stride windows (include/ctok_pipeline.h, "Padded batches ...") -----------------
  ctok_pw::Win W{};
  hipEvent_t ev_rec[2] = {};  // the records, which belong to the plan stage but run after its counts came back

  static uint32_t window_mode(uint32_t flags) {
    return (flags & CTOK_P_WINDOWS) ? pwin::kWindows : (flags & CTOK_P_TRUNCATE) ? pwin::kCut : pwin::kNone;
  }

  // The rows of a window call and their plan: everything up to n_windows and width.  The errors in order:
  // those of the encode, then the panic of the lowest row, then the 2^32 windows.  n_rows > 0.
  void window_plan(const uint8_t* d_text, const uint64_t* d_off, uint64_t n_rows, uint32_t per_row, uint64_t nb, ctok_postprocessor* pp,
                   const ctok_pipeline_window_opts& o, hipStream_t s) {
    using namespace ctok_pw;
    for (double& t : win_ms) t = 0;
    win_info = ctok_pipeline_window_info{};
    win_info.rows = n_rows;
    W = Win{};
    if (o.flags & CTOK_P_ADD_SPECIAL) {
      encodings(d_text, d_off, n_rows, per_row, nb, pp, s);
      W.ids = r_ids;
      W.type_ids = e_type.p;
      W.special_mask = e_spec.p;
      W.row_off = r_row_off;
      W.offsets = e_off.p;
      W.word_ids = e_wids.p;
    } else {
      // Encoding::from_ids over the id path: no post-processor, no offsets, and `tokens` without the ids that
      // have no vocab string
      for (double& t : enc_ms) t = 0;
      enc_info = ctok_pipeline_encoding_info{};
      const uint64_t n = n_rows * per_row;
      run(d_text, d_off, n, nb, 0, s);
      ids.ensure(n_ids + 1);
      tok_off.ensure(n + 1);
      emit(ids.p, tok_off.p, s);
      e_seq_off.ensure(n_rows + 1);
      e_na.ensure(n_rows + 1);
      ctok_pe::Rows r{};
      r.tok_off = tok_off.p;
      r.per_row = per_row;
      r.n_rows = n_rows;
      r.seq_off = e_seq_off.p;
      r.n_a = e_na.p;
      HIPT(ctok_pe::launch_row_heads(r, s));
      w_tokenless.ensure(n_rows + 1);
      HIPT(hipMemsetAsync(w_tokenless.p, 0, n_rows * 4, s));
      HIPT(launch_tokenless(ids.p, n_ids, e_seq_off.p, n_rows, d_len_id.p, (uint32_t)len_id.size(), w_tokenless.p, s));
      W.ids = ids.p;
      W.row_off = e_seq_off.p;
      W.tokenless = w_tokenless.p;
    }
    W.seq_off = e_seq_off.p;
    W.n_a = e_na.p;
    W.n_rows = n_rows;
    W.mode = window_mode(o.flags);
    W.pad_left = (o.flags & CTOK_P_PAD_LEFT) ? 1 : 0;
    W.pad_id = (o.flags & CTOK_P_PAD_ID) ? o.pad_id : default_pad_id;
    W.m = o.max_length;
    W.stride = W.mode == pwin::kWindows ? o.stride : 0;
    w_row_win.ensure(n_rows + 2);
    w_rep.ensure(kNumRep);
    tmp64.ensure(ctok_dev::scan_tmp_elems(n_rows + 1) + 64);
    W.row_win = w_row_win.p;
    W.rep = (unsigned long long*)w_rep.p;
    const uint64_t rep0[kNumRep] = {kNoRow, 0};
    uint64_t h_rep[kNumRep] = {}, n_win = 0;
    HIPT(hipMemcpyAsync(w_rep.p, rep0, sizeof(rep0), hipMemcpyHostToDevice, s));
    HIPT(hipEventRecord(ev_win[0], s));
    HIPT(launch_plan(W, s));
    HIPT(ctok_dev::scan_u64(w_row_win.p, n_rows, tmp64.p, tmp64.cap, s));
    HIPT(hipEventRecord(ev_win[1], s));
    HIPT(hipMemcpyAsync(h_rep, w_rep.p, sizeof(h_rep), hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(&n_win, w_row_win.p + n_rows, 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (h_rep[kRepPanic] != kNoRow) {
      const uint64_t r = h_rep[kRepPanic];
      if (r >= n_rows) throw_error(CTOK_E_DEVICE, "pipeline: the panic report is out of bounds");
      uint64_t ro[2] = {}, so[2] = {};
      uint32_t less = 0;
      HIPT(hipMemcpyAsync(ro, W.row_off + r, 16, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(so, W.seq_off + r, 16, hipMemcpyDeviceToHost, s));
      if (W.tokenless) HIPT(hipMemcpyAsync(&less, W.tokenless + r, 4, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      const uint64_t t = so[1] - so[0] - less;
      // (the text of Encoding._slice: the package's own truncate / truncate_with_stride raise it for this row)
      throw_error(CTOK_E_PANIC, "range end index " + std::to_string(pwin::panic_end(W.mode, ro[1] - ro[0], t, W.m, W.stride)) +
                                    " out of range for slice of length " + std::to_string(t) + " (tokens)");
    }
    if (n_win < n_rows) throw_error(CTOK_E_DEVICE, "pipeline: fewer windows than rows");
    if (n_win >> 32) throw_error(CTOK_E_ARG, "pipeline: " + std::to_string(n_win) + " windows: a call must stay below 2^32");
    const uint64_t longest = h_rep[kRepMain];
    W.target = (o.flags & CTOK_P_PAD_TO_MAX) ? W.m : (o.flags & CTOK_P_PAD_LONGEST) ? longest : 0;
    W.n_windows = n_win;
    W.width = std::max(longest, W.target);
    win_info.windows = n_win;
    win_info.width = W.width;
  }

  // The records and the arrays into d (capacities checked by the caller).
  void window_write(const ctok_pipeline_windows_device& d, hipStream_t s) {
    using namespace ctok_pw;
    W.win_len = d.win_len;
    W.win_row = d.win_row;
    W.win_start = d.win_start;
    W.win_off_len = d.win_off_len;
    W.win_seq_len = d.win_seq_len;
    W.out_ids = d.ids;
    W.out_attn = d.attention_mask;
    W.out_type = d.type_ids;
    W.out_special = d.special_tokens_mask;
    W.out_offsets = d.offsets;
    W.out_word = d.word_ids;
    W.out_seq = d.sequence_ids;
    HIPT(hipEventRecord(ev_rec[0], s));
    HIPT(launch_records(W, s));
    HIPT(hipEventRecord(ev_rec[1], s));
    HIPT(hipEventRecord(ev_win[2], s));
    HIPT(launch_write(W, s));
    HIPT(hipEventRecord(ev_win[3], s));
    HIPT(hipStreamSynchronize(s));
    float plan = 0, rec = 0, wr = 0;
    HIPT(hipEventElapsedTime(&plan, ev_win[0], ev_win[1]));
    HIPT(hipEventElapsedTime(&rec, ev_rec[0], ev_rec[1]));
    HIPT(hipEventElapsedTime(&wr, ev_win[2], ev_win[3]));
    win_ms[0] = (double)plan + rec;
    win_ms[1] = wr;
    const uint64_t cells = W.n_windows * W.width;
    win_info.bytes_written = cells * 4 * (1 + (d.attention_mask != nullptr) + (d.type_ids != nullptr) + (d.special_tokens_mask != nullptr) +
                                          (d.word_ids != nullptr) + (d.sequence_ids != nullptr)) + (d.offsets ? cells * 16 : 0);
  }
};

namespace {

std::vector<std::string> strings_of(const uint8_t* bytes, const uint64_t* off, uint64_t n, const char* what) {
  std::vector<std::string> out;
  if (n && (!off || (off[n] && !bytes))) throw_error(CTOK_E_ARG, std::string("null ") + what);
  out.reserve(n);
  for (uint64_t i = 0; i < n; i++) {
    if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    out.emplace_back((const char*)bytes + off[i], off[i + 1] - off[i]);
  }
  return out;
}

}  // namespace

extern "C" {

int ctok_pipeline_create(const ctok_pipeline_tables* tb, ctok_normalizer* nz, ctok_pretokenizer* pt, int device,
                         ctok_pipeline** out) {
  if (!out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    if (!tb || (tb->n_vocab && !tb->vocab_id) || (tb->n_added && (!tb->added_id || !tb->added_flags)))
      throw_error(CTOK_E_ARG, "null argument");
    if (tb->n_merge_strings & 1) throw_error(CTOK_E_ARG, "the merges are pairs: an odd number of strings was given");
    const std::vector<std::string> vs = strings_of(tb->vocab_bytes, tb->vocab_off, tb->n_vocab, "vocab");
    const std::vector<std::string> ms = strings_of(tb->merge_bytes, tb->merge_off, tb->n_merge_strings, "merges");
    const std::vector<std::string> as = strings_of(tb->added_bytes, tb->added_off, tb->n_added, "added tokens");
    std::vector<std::pair<std::string, uint32_t>> vocab;
    vocab.reserve(vs.size());
    for (uint64_t i = 0; i < vs.size(); i++) vocab.emplace_back(vs[i], tb->vocab_id[i]);
    std::vector<std::pair<std::string, std::string>> merges;
    merges.reserve(ms.size() / 2);
    for (size_t i = 0; i + 1 < ms.size(); i += 2) merges.emplace_back(ms[i], ms[i + 1]);
    std::vector<wordbpe::AddedToken> added;
    for (uint64_t i = 0; i < as.size(); i++) {
      const uint32_t f = tb->added_flags[i];
      added.push_back(wordbpe::AddedToken{as[i], tb->added_id[i],
                                          ((f & CTOK_PIPELINE_AT_SINGLE_WORD) ? (uint32_t)wordbpe::kSingleWord : 0u) |
                                              ((f & CTOK_PIPELINE_AT_LSTRIP) ? (uint32_t)wordbpe::kLstrip : 0u) |
                                              ((f & CTOK_PIPELINE_AT_RSTRIP) ? (uint32_t)wordbpe::kRstrip : 0u)});
    }
    auto p = std::make_unique<ctok_pipeline>();
    p->nz = nz;
    p->pt = pt;
    p->device = device;
    p->cap = word_cap();
    p->find_cap = find_work_cap();
    // id -> the bytes of its vocab string: of the strings that share an id the last one, which is what
    // id_to_token answers; ids need not be dense, so a sorted table
    {
      std::vector<std::pair<uint32_t, uint32_t>> il;
      il.reserve(vocab.size());
      for (const auto& kv : vocab) il.emplace_back(kv.second, (uint32_t)std::min<size_t>(kv.first.size(), 0xFFFFFFFFu));
      std::stable_sort(il.begin(), il.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      for (size_t i = 0; i < il.size(); i++) {
        if (i + 1 < il.size() && il[i + 1].first == il[i].first) continue;
        p->len_id.push_back(il[i].first);
        p->len_val.push_back(il[i].second);
      }
      std::map<std::string, uint32_t> special;  // content -> id as the reference's map keeps it: the last entry of a content
      for (uint64_t i = 0; i < as.size(); i++)
        if (tb->added_flags[i] & CTOK_PIPELINE_AT_SPECIAL) special[as[i]] = tb->added_id[i];
      for (const auto& kv : special) p->special_id.push_back(kv.second);
      for (const char* name : {"<pad>", "[PAD]"})
        if (auto it = special.find(name); it != special.end()) p->default_pad_id = it->second;
      std::sort(p->special_id.begin(), p->special_id.end());
      p->special_id.erase(std::unique(p->special_id.begin(), p->special_id.end()), p->special_id.end());
    }
    std::string err;
    const int rc = wordbpe::compile(vocab, merges, added, &p->c, &err);
    if (rc != wordbpe::kOk) throw_error(rc, err);
    p->to_device();
    *out = p.release();
  });
}

void ctok_pipeline_destroy(ctok_pipeline* p) { delete p; }

int ctok_pipeline_encode_batch(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n, uint32_t flags,
                               const uint32_t** ids, const uint64_t** tok_off) {
  return ctok_host::run_guarded([&] {
    if (!p || !ids || !tok_off || (n && (!off || (off[n] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    p->h_ids.clear();
    p->h_tok_off.assign(n + 1, 0);
    *ids = p->h_ids.data();
    *tok_off = p->h_tok_off.data();
    for (double& t : p->stage_ms) t = 0;
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++) {
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      if (!valid_utf8(utf8, off[i], off[i + 1])) throw_error(CTOK_E_ARG, "text " + std::to_string(i) + " is not UTF-8");
    }
    const uint64_t nb = off[n];
    if (nb >= kRefuseFrom || n >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "pipeline: the input reaches 4 GiB");
    HIPT(hipSetDevice(p->device));
    hipStream_t s = p->own;
    p->in_text.ensure(nb + 64);
    p->in_off.ensure(n + 1);
    p->tok_off.ensure(n + 1);
    if (nb) HIPT(hipMemcpyAsync(p->in_text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemcpyAsync(p->in_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    p->run(p->in_text.p, p->in_off.p, n, nb, flags, s);
    p->ids.ensure(p->n_ids + 1);
    p->emit(p->ids.p, p->tok_off.p, s);
    p->h_ids.resize(p->n_ids);
    if (p->n_ids) HIPT(hipMemcpyAsync(p->h_ids.data(), p->ids.p, p->n_ids * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(p->h_tok_off.data(), p->tok_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    *ids = p->h_ids.data();
    *tok_off = p->h_tok_off.data();
  });
}

int ctok_pipeline_encode_batch_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n, uint64_t nb,
                                      uint32_t flags, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_tok_off, uint64_t* n_ids_out,
                                      void* stream) {
  return ctok_host::run_guarded([&] {
    if (!p || !d_tok_off || !n_ids_out || (n && !d_off) || (nb && !d_utf8)) throw_error(CTOK_E_ARG, "null argument");
    *n_ids_out = 0;
    HIPT(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    for (double& t : p->stage_ms) t = 0;
    if (!n) {
      HIPT(hipMemsetAsync(d_tok_off, 0, 8, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    p->run(d_utf8, d_off, n, nb, flags, s);
    *n_ids_out = p->n_ids;
    if (p->n_ids > ids_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_pipeline_encode_batch_device: the ids need " + std::to_string(p->n_ids) + " entries");
    if (p->n_ids && !d_ids) throw_error(CTOK_E_ARG, "null argument");
    p->emit(d_ids, d_tok_off, s);
  });
}

int ctok_pipeline_encode_encodings(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n_rows, const uint8_t* pair_utf8,
                                   const uint64_t* pair_off, ctok_postprocessor* pp, ctok_pipeline_encodings* out) {
  return ctok_host::run_guarded([&] {
    if (!p || !out || (n_rows && (!off || (off[n_rows] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    if (pair_off && n_rows && pair_off[n_rows] && !pair_utf8) throw_error(CTOK_E_ARG, "null argument");
    const uint32_t per_row = pair_off ? 2 : 1;
    p->h_out.clear(), p->h_type.clear(), p->h_spec.clear(), p->h_wids.clear(), p->h_seq_ids.clear(), p->h_offsets.clear(), p->h_na.assign(n_rows, 0);
    p->h_row_off.assign(n_rows + 1, 0);
    p->h_seq_off.assign(n_rows + 1, 0);
    *out = ctok_pipeline_encodings{p->h_out.data(), p->h_type.data(), p->h_spec.data(), p->h_row_off.data(), p->h_offsets.data(),
                                   p->h_wids.data(), p->h_seq_ids.data(), p->h_seq_off.data(), p->h_na.data(), n_rows};
    for (double& t : p->stage_ms) t = 0;
    for (double& t : p->enc_ms) t = 0;
    if (!n_rows) return;
    const uint64_t nb = p->upload_rows(utf8, off, n_rows, pair_utf8, pair_off);
    hipStream_t s = p->own;
    p->encodings(p->in_text.p, p->in_off.p, n_rows, per_row, nb, pp, s);
    const uint64_t ni = p->n_ids, nc = p->n_cells;
    p->h_out.resize(nc), p->h_type.resize(nc), p->h_spec.resize(nc), p->h_wids.resize(ni), p->h_seq_ids.resize(ni), p->h_offsets.resize(2 * ni);
    if (nc) {
      HIPT(hipMemcpyAsync(p->h_out.data(), p->r_ids, nc * 4, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(p->h_type.data(), p->e_type.p, nc * 4, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(p->h_spec.data(), p->e_spec.p, nc * 4, hipMemcpyDeviceToHost, s));
    }
    if (ni) {
      HIPT(hipMemcpyAsync(p->h_wids.data(), p->e_wids.p, ni * 4, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(p->h_seq_ids.data(), p->ids.p, ni * 4, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(p->h_offsets.data(), p->e_off.p, ni * 16, hipMemcpyDeviceToHost, s));
    }
    HIPT(hipMemcpyAsync(p->h_row_off.data(), p->r_row_off, (n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(p->h_seq_off.data(), p->e_seq_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(p->h_na.data(), p->e_na.p, n_rows * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    *out = ctok_pipeline_encodings{p->h_out.data(), p->h_type.data(), p->h_spec.data(), p->h_row_off.data(), p->h_offsets.data(),
                                   p->h_wids.data(), p->h_seq_ids.data(), p->h_seq_off.data(), p->h_na.data(), n_rows};
  });
}

int ctok_pipeline_encode_encodings_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_rows, int pairs,
                                          uint64_t nb, ctok_postprocessor* pp, ctok_pipeline_encodings_device* out, void* stream) {
  return ctok_host::run_guarded([&] {
    if (!p || !out || !out->row_off || !out->seq_off || (n_rows && (!d_off || !out->n_a)) || (nb && !d_utf8))
      throw_error(CTOK_E_ARG, "null argument");
    out->n_cells = out->n_ids = 0;
    // checked before any device is used: a refused call launches nothing and writes nothing
    if (((uintptr_t)out->ids | (uintptr_t)out->type_ids | (uintptr_t)out->special_tokens_mask | (uintptr_t)out->word_ids | (uintptr_t)out->seq_ids) & 3u)
      throw_error(CTOK_E_ARG, "ctok_pipeline_encode_encodings_device: the ids must be 4-byte aligned");
    if (((uintptr_t)d_off | (uintptr_t)out->row_off | (uintptr_t)out->seq_off | (uintptr_t)out->n_a | (uintptr_t)out->offsets) & 7u)
      throw_error(CTOK_E_ARG, "ctok_pipeline_encode_encodings_device: the offsets must be 8-byte aligned");
    HIPT(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    for (double& t : p->stage_ms) t = 0;
    for (double& t : p->enc_ms) t = 0;
    if (!n_rows) {
      HIPT(hipMemsetAsync(out->row_off, 0, 8, s));
      HIPT(hipMemsetAsync(out->seq_off, 0, 8, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    if (n_rows >= kRefuseFrom / 2) throw_error(CTOK_E_CAPACITY, "pipeline: the input reaches 4 GiB");
    p->encodings(d_utf8, d_off, n_rows, pairs ? 2 : 1, nb, pp, s);
    const uint64_t ni = p->n_ids, nc = p->n_cells;
    out->n_cells = nc;
    out->n_ids = ni;
    if (nc > out->cells_cap || ni > out->ids_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_pipeline_encode_encodings_device: the rows need " + std::to_string(nc) + " cells, the offsets and word ids " +
                                       std::to_string(ni) + " entries");
    if ((nc && (!out->ids || !out->type_ids || !out->special_tokens_mask)) || (ni && (!out->offsets || !out->word_ids)))
      throw_error(CTOK_E_ARG, "null argument");
    if (nc) {
      HIPT(hipMemcpyAsync(out->ids, p->r_ids, nc * 4, hipMemcpyDeviceToDevice, s));
      HIPT(hipMemcpyAsync(out->type_ids, p->e_type.p, nc * 4, hipMemcpyDeviceToDevice, s));
      HIPT(hipMemcpyAsync(out->special_tokens_mask, p->e_spec.p, nc * 4, hipMemcpyDeviceToDevice, s));
    }
    if (ni) {
      HIPT(hipMemcpyAsync(out->word_ids, p->e_wids.p, ni * 4, hipMemcpyDeviceToDevice, s));
      if (out->seq_ids) HIPT(hipMemcpyAsync(out->seq_ids, p->ids.p, ni * 4, hipMemcpyDeviceToDevice, s));
      HIPT(hipMemcpyAsync(out->offsets, p->e_off.p, ni * 16, hipMemcpyDeviceToDevice, s));
    }
    HIPT(hipMemcpyAsync(out->row_off, p->r_row_off, (n_rows + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIPT(hipMemcpyAsync(out->seq_off, p->e_seq_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIPT(hipMemcpyAsync(out->n_a, p->e_na.p, n_rows * 8, hipMemcpyDeviceToDevice, s));
    HIPT(hipStreamSynchronize(s));
  });
}

namespace {

// before any device is used
void check_window_opts(const ctok_pipeline_window_opts* o) {
  if (!o) throw_error(CTOK_E_ARG, "null argument");
  if ((o->flags & CTOK_P_WINDOWS) && o->stride >= o->max_length)
    throw_error(CTOK_E_ARG, "stride must be smaller than max_length (the reference loops forever)");
}

}  // namespace

int ctok_pipeline_encode_windows(ctok_pipeline* p, const uint8_t* utf8, const uint64_t* off, uint64_t n_rows, const uint8_t* pair_utf8,
                                 const uint64_t* pair_off, ctok_postprocessor* pp, const ctok_pipeline_window_opts* opts,
                                 ctok_pipeline_windows* out) {
  return ctok_host::run_guarded([&] {
    if (!p || !out || (n_rows && (!off || (off[n_rows] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    if (pair_off && n_rows && pair_off[n_rows] && !pair_utf8) throw_error(CTOK_E_ARG, "null argument");
    check_window_opts(opts);
    p->hw_row_win.assign(n_rows + 1, 0);
    *out = ctok_pipeline_windows{};
    out->row_win = p->hw_row_win.data();
    out->n_rows = n_rows;
    for (double& t : p->stage_ms) t = 0;
    for (double& t : p->enc_ms) t = 0;
    for (double& t : p->win_ms) t = 0;
    p->win_info = ctok_pipeline_window_info{};
    if (!n_rows) return;
    const uint64_t nb = p->upload_rows(utf8, off, n_rows, pair_utf8, pair_off);
    hipStream_t s = p->own;
    p->window_plan(p->in_text.p, p->in_off.p, n_rows, pair_off ? 2 : 1, nb, pp, *opts, s);
    const uint64_t nw = p->W.n_windows, width = p->W.width, cells = nw * width;
    const bool offs = opts->want & CTOK_PIPELINE_WIN_OFFSETS, word = opts->want & CTOK_PIPELINE_WIN_WORD_IDS,
               seq = opts->want & CTOK_PIPELINE_WIN_SEQUENCE_IDS;
    ctok_pipeline_windows_device d{};
    p->w_ids.ensure(cells + 1), p->w_attn.ensure(cells + 1), p->w_type.ensure(cells + 1), p->w_spec.ensure(cells + 1);
    p->w_len.ensure(nw + 1), p->w_row.ensure(nw + 1), p->w_start.ensure(nw + 1), p->w_off_len.ensure(nw + 1), p->w_seq_len.ensure(nw + 1);
    d.ids = p->w_ids.p, d.attention_mask = p->w_attn.p, d.type_ids = p->w_type.p, d.special_tokens_mask = p->w_spec.p;
    d.win_len = p->w_len.p, d.win_row = p->w_row.p, d.win_start = p->w_start.p, d.win_off_len = p->w_off_len.p, d.win_seq_len = p->w_seq_len.p;
    if (offs) p->w_offsets.ensure(2 * cells + 1), d.offsets = p->w_offsets.p;
    if (word) p->w_word.ensure(cells + 1), d.word_ids = p->w_word.p;
    if (seq) p->w_seq.ensure(cells + 1), d.sequence_ids = p->w_seq.p;
    p->window_write(d, s);
    const auto down32 = [&](std::vector<uint32_t>& h, const uint32_t* src, uint64_t n) {
      h.resize(n);
      if (n) HIPT(hipMemcpyAsync(h.data(), src, n * 4, hipMemcpyDeviceToHost, s));
      return (const uint32_t*)h.data();
    };
    const auto down64 = [&](std::vector<uint64_t>& h, const uint64_t* src, uint64_t n) {
      h.resize(n);
      if (n) HIPT(hipMemcpyAsync(h.data(), src, n * 8, hipMemcpyDeviceToHost, s));
      return (const uint64_t*)h.data();
    };
    out->ids = down32(p->hw_ids, d.ids, cells);
    out->attention_mask = down32(p->hw_attn, d.attention_mask, cells);
    out->type_ids = down32(p->hw_type, d.type_ids, cells);
    out->special_tokens_mask = down32(p->hw_spec, d.special_tokens_mask, cells);
    if (offs) out->offsets = down64(p->hw_offsets, d.offsets, 2 * cells);
    if (word) out->word_ids = down32(p->hw_word, d.word_ids, cells);
    if (seq) out->sequence_ids = down32(p->hw_seq, d.sequence_ids, cells);
    out->win_len = down64(p->hw_len, d.win_len, nw);
    out->win_row = down32(p->hw_row, d.win_row, nw);
    out->win_start = down64(p->hw_start, d.win_start, nw);
    out->win_off_len = down64(p->hw_off_len, d.win_off_len, nw);
    out->win_seq_len = down64(p->hw_seq_len, d.win_seq_len, nw);
    out->row_win = down64(p->hw_row_win, p->w_row_win.p, n_rows + 1);
    HIPT(hipStreamSynchronize(s));
    out->n_windows = nw;
    out->width = width;
  });
}

int ctok_pipeline_encode_windows_device(ctok_pipeline* p, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_rows, uint64_t nb,
                                        ctok_postprocessor* pp, const ctok_pipeline_window_opts* opts, ctok_pipeline_windows_device* out,
                                        void* stream) {
  return ctok_host::run_guarded([&] {
    if (!p || !out || !out->row_win || !out->win_len || !out->win_row || (n_rows && !d_off) || (nb && !d_utf8))
      throw_error(CTOK_E_ARG, "null argument");
    out->n_windows = out->width = 0;
    // checked before any device is used: a refused call launches nothing and writes nothing
    check_window_opts(opts);
    if (((uintptr_t)out->ids | (uintptr_t)out->attention_mask | (uintptr_t)out->type_ids | (uintptr_t)out->special_tokens_mask |
         (uintptr_t)out->word_ids | (uintptr_t)out->sequence_ids | (uintptr_t)out->win_row) & 3u)
      throw_error(CTOK_E_ARG, "ctok_pipeline_encode_windows_device: the u32 arrays must be 4-byte aligned");
    if (((uintptr_t)d_off | (uintptr_t)out->offsets | (uintptr_t)out->win_len | (uintptr_t)out->win_start | (uintptr_t)out->win_off_len |
         (uintptr_t)out->win_seq_len | (uintptr_t)out->row_win) & 7u)
      throw_error(CTOK_E_ARG, "ctok_pipeline_encode_windows_device: the u64 arrays must be 8-byte aligned");
    HIPT(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    for (double& t : p->stage_ms) t = 0;
    for (double& t : p->enc_ms) t = 0;
    for (double& t : p->win_ms) t = 0;
    p->win_info = ctok_pipeline_window_info{};
    if (!n_rows) {
      HIPT(hipMemsetAsync(out->row_win, 0, 8, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    if (n_rows >= kRefuseFrom / 2) throw_error(CTOK_E_CAPACITY, "pipeline: the input reaches 4 GiB");
    p->window_plan(d_utf8, d_off, n_rows, (opts->flags & CTOK_P_PAIRS) ? 2 : 1, nb, pp, *opts, s);
    const uint64_t nw = p->W.n_windows, width = p->W.width;
    out->n_windows = nw;
    out->width = width;
    HIPT(hipMemcpyAsync(out->row_win, p->w_row_win.p, (n_rows + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIPT(hipStreamSynchronize(s));
    if (nw > out->win_cap || nw * width > out->cap)
      throw_error(CTOK_E_CAPACITY, "ctok_pipeline_encode_windows_device: " + std::to_string(nw) + " windows of width " + std::to_string(width) +
                                       " are needed");
    if (nw * width && !out->ids) throw_error(CTOK_E_ARG, "null argument");
    p->window_write(*out, s);
  });
}

int ctok_pipeline_window_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_WINDOW_STAGES]) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    for (int i = 0; i < CTOK_PIPELINE_WINDOW_STAGES; i++) out[i] = p->win_ms[i];
  });
}

const char* ctok_pipeline_window_stage_name(uint64_t i) { return i < CTOK_PIPELINE_WINDOW_STAGES ? kWinStageNames[i] : ""; }

int ctok_pipeline_window_stats(const ctok_pipeline* p, ctok_pipeline_window_info* out) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = p->win_info;
  });
}

int ctok_pipeline_encoding_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_ENCODING_STAGES]) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    for (int i = 0; i < CTOK_PIPELINE_ENCODING_STAGES; i++) out[i] = p->enc_ms[i];
  });
}

const char* ctok_pipeline_encoding_stage_name(uint64_t i) { return i < CTOK_PIPELINE_ENCODING_STAGES ? kEncStageNames[i] : ""; }

void ctok_pipeline_encoding_limits(const ctok_pipeline* p, ctok_pipeline_encoding_limits_t* out) {
  if (!out) return;
  out->max_find_work = p ? p->find_cap : find_work_cap();
  out->max_special_tokens = ctok_pe::kMaxSpecial;
  out->max_find_compares = out->max_find_work / ctok_pe::kFindCompareShare;
}

int ctok_pipeline_encoding_stats(const ctok_pipeline* p, ctok_pipeline_encoding_info* out) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = p->enc_info;
  });
}

int ctok_pipeline_stage_ms(const ctok_pipeline* p, double out[CTOK_PIPELINE_STAGES]) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    for (int i = 0; i < CTOK_PIPELINE_STAGES; i++) out[i] = p->stage_ms[i];
  });
}

const char* ctok_pipeline_stage_name(uint64_t i) { return i < CTOK_PIPELINE_STAGES ? kStageNames[i] : ""; }

void ctok_pipeline_limits(const ctok_pipeline* p, ctok_pipeline_limits_t* out) {
  if (!out) return;
  out->tier1 = kTier1;
  out->tier2 = kTier2;
  out->max_word_symbols = p ? p->cap : word_cap();
  out->max_flagged_word_bytes = p ? p->flag_cap : kMaxFlaggedWordBytes;
  out->max_added_group_bytes = wordbpe::kMaxGroupBytes;
  out->max_batch_bytes = p && p->match_cap < kRefuseFrom ? p->match_cap : kRefuseFrom - 1;
  out->max_added_tokens = wordbpe::kMaxAdded;
  out->max_added_token_bytes = wordbpe::kMaxAddedBytes;
  out->max_merges = wordbpe::kMaxMerges;
}

int ctok_pipeline_stats(const ctok_pipeline* p, ctok_pipeline_info* out) {
  return ctok_host::run_guarded([&] {
    if (!p || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = p->info;
  });
}

}  // extern "C"
