// Host runtime of the stand-alone models behind include/ctok_models.h: WordLevelModel,
// CharBpeModel and ByteLevelBpeModel (reference src/models.rs:300-741, Complexity-ML/
// complexity-tokenizer v0.3.3).  The strings stay here: strmerge_compile.cpp turns vocab and merges
// into symbol tables at create; encode runs on the device (strmerge.hip) in four stages, with the
// White_Space split of the BPE trainer (bpe_train.hip launch_ws_bits) and scan.hip's scans:
//   start bits -> run list, symbol counts, classes -> initial symbols and merges -> emit
// A word above the cap (strmerge_internal.h kMaxWordSymbols) fails the call before the merges.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_models.h"
#include "bpe_train_internal.h"  // ctok_bpe::launch_ws_bits
#include "ctok_internal.h"       // ctok_dev::scan_u32, scan_tmp_elems
#include "host_common.h"
#include "knobs.h"
#include "strmerge_compile.h"
#include "strmerge_internal.h"
#include "train_host_common.h"

using namespace ctok_sm;
using ctok_host::throw_error;
using ctok_train_host::DBuf;

static_assert(strmerge::kErrUnsupported == CTOK_E_UNSUPPORTED && strmerge::kErrArg == CTOK_E_ARG &&
                  strmerge::kErrCapacity == CTOK_E_CAPACITY,
              "strmerge_compile.h repeats the codes of ctok.h");

namespace {

uint64_t word_cap() {
  uint64_t cap = kMaxWordSymbols;
  if (auto e = ctok_rt::env_u64("CTOK_MODELS_MAX_WORD_SYMBOLS")) cap = std::min<uint64_t>(cap, *e);
  return cap;
}

template <typename T>
void upload(DBuf<T>& d, const T* src, size_t n, hipStream_t s) {
  d.ensure(n);
  if (n) HIPT(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
}

}  // namespace

struct ctok_sm_model {
  strmerge::Kind kind = strmerge::kWordLevel;
  strmerge::Compiled c;
  uint64_t n_vocab = 0;
  bool prefix_space = false;
  int device = 0;
  hipStream_t s = nullptr;
  hipEvent_t ev[CTOK_MODELS_STAGES + 1] = {};
  double stage_ms[CTOK_MODELS_STAGES] = {};
  // the tables
  DBuf<strmerge::PairSlot> d_pairs;
  DBuf<uint32_t> d_sym_id, d_byte2sym;
  DBuf<wptab::Slot> d_slots;
  DBuf<uint8_t> d_blob;
  Model M{};
  // a call's buffers
  DBuf<uint8_t> text;
  DBuf<uint64_t> doc_off, tok_off, state3;
  DBuf<uint32_t> bits, dbits, pc, cpc, wrank, crank, runs, nsym, soff, fcnt, wpos, tok, list2, list3, state, ctr, tmp;
  DBuf<uint32_t> eflag, ebefore, ids;
  std::vector<uint32_t> h_ids;
  std::vector<uint64_t> h_tok_off;

  ~ctok_sm_model() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }

  void to_device() {
    HIPT(hipSetDevice(device));
    HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev) HIPT(hipEventCreate(&e));
    upload(d_pairs, c.pairs.data(), c.pairs.size(), s);
    upload(d_sym_id, c.sym_id.data(), c.sym_id.size(), s);
    upload(d_byte2sym, c.byte2sym, 256, s);
    upload(d_slots, c.strings.slots.data(), c.strings.slots.size(), s);
    upload(d_blob, c.strings.blob.data(), c.strings.blob.size(), s);
    HIPT(hipStreamSynchronize(s));
    M.kind = (uint32_t)kind;
    M.pairs = strmerge::PairView{d_pairs.p, (uint32_t)c.pairs.size() - 1};
    M.sym_id = d_sym_id.p;
    M.byte2sym = d_byte2sym.p;
    M.strings = wptab::View{d_slots.p, d_blob.p, (uint32_t)c.strings.slots.size() - 1, c.strings.max_len};
    M.foreign = c.foreign;
    M.prefix_space = prefix_space ? 1u : 0u;
  }

  void scan(const uint32_t* in, uint32_t* out, uint64_t n) {  // out[n] = the total
    if (n) HIPT(ctok_dev::scan_u32(in, out, n, nullptr, tmp.p, tmp.cap, s));
    else HIPT(hipMemsetAsync(out, 0, 4, s));
  }

  void encode(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    HIPT(hipSetDevice(device));
    h_ids.clear();
    h_tok_off.assign(n + 1, 0);
    for (double& t : stage_ms) t = 0;
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    const uint64_t nb = off[n];
    if (nb + n >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a batch of 4 GiB or more");
    const bool virt = kind == strmerge::kByteLevel && prefix_space;
    if (!nb) {  // only empty texts: each is the one-symbol word " " under the prefix space, else nothing
      if (virt) {
        h_ids.assign(n, c.sym_id[c.byte2sym[0x20]]);
        for (uint64_t i = 0; i <= n; i++) h_tok_off[i] = i;
      }
      return;
    }
    const uint32_t n_w = (uint32_t)((nb + 31) / 32);
    text.ensure(nb + 16);
    doc_off.ensure(n + 1);
    tok_off.ensure(n + 1);
    bits.ensure(n_w);
    pc.ensure((size_t)n_w + 1);
    wrank.ensure((size_t)n_w + 1);
    ctr.ensure(kNumCtr);
    tmp.ensure(ctok_dev::scan_tmp_elems(std::max<uint64_t>(nb, n) + 1) + 64);
    if (kind == strmerge::kByteLevel) dbits.ensure(n_w);
    if (kind == strmerge::kCharBpe) {
      cpc.ensure((size_t)n_w + 1);
      crank.ensure((size_t)n_w + 1);
    }
    HIPT(hipMemcpyAsync(text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(doc_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(ctr.p, 0, kNumCtr * 4, s));
    Batch B{};
    B.text = text.p;
    B.n_bytes = (uint32_t)nb;
    B.n_w = n_w;
    B.doc_off = doc_off.p;
    B.n_docs = n;
    B.bits = bits.p;
    B.dbits = dbits.p;
    B.wrank = wrank.p;
    B.crank = crank.p;
    B.ctr = ctr.p;

    // 1. start bits
    HIPT(hipEventRecord(ev[0], s));
    if (kind == strmerge::kByteLevel) HIPT(launch_byte_starts(B, s));
    else HIPT(ctok_bpe::launch_ws_bits(text.p, (uint32_t)nb, doc_off.p, n, bits.p, s));
    HIPT(hipEventRecord(ev[1], s));

    // 2. the run list, the symbol counts and the classes
    HIPT(launch_popc(B, pc.p, kind == strmerge::kCharBpe ? cpc.p : nullptr, s));
    scan(pc.p, wrank.p, n_w);
    if (kind == strmerge::kCharBpe) scan(cpc.p, crank.p, n_w);
    uint32_t n_runs = 0;
    HIPT(hipMemcpyAsync(&n_runs, wrank.p + n_w, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (n_runs > nb) throw_error(CTOK_E_DEVICE, "models encode: more words than bytes");
    runs.ensure((size_t)n_runs + 1);
    nsym.ensure((size_t)n_runs + 1);
    soff.ensure((size_t)n_runs + 1);
    fcnt.ensure((size_t)n_runs + 1);
    wpos.ensure((size_t)n_runs + 1);
    // a run of more than kTier1 symbols has kTier1 bytes or more, one of more than kTier2 has kTier2
    const uint64_t cap2 = nb / kTier1 + 1, cap3 = nb / kTier2 + 1;
    list2.ensure(cap2);
    list3.ensure(cap3);
    state3.ensure(cap3);
    B.runs = runs.p;
    B.nsym = nsym.p;
    B.soff = soff.p;
    B.fcnt = fcnt.p;
    B.wpos = wpos.p;
    B.list2 = list2.p;
    B.list3 = list3.p;
    B.state3 = state3.p;
    HIPT(launch_runs(B, s));
    HIPT(launch_word_info(M, B, n_runs, s));
    scan(nsym.p, soff.p, n_runs);
    HIPT(hipEventRecord(ev[2], s));
    uint32_t h_ctr[kNumCtr] = {};
    uint32_t n_sym = 0;
    HIPT(hipMemcpyAsync(h_ctr, ctr.p, kNumCtr * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(&n_sym, soff.p + n_runs, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    const uint32_t n2 = h_ctr[kCtrList2], n3 = h_ctr[kCtrList3];
    const uint64_t n_state = (uint64_t)h_ctr[kCtrState] | (uint64_t)h_ctr[kCtrState + 1] << 32;
    if (n2 > cap2 || n3 > cap3 || n_sym > nb + n || n_state > nb + n)
      throw_error(CTOK_E_DEVICE, "models encode: the word list is out of bounds");
    const uint64_t cap = word_cap();
    if (h_ctr[kCtrMaxSym] > cap)
      throw_error(CTOK_E_UNSUPPORTED, "a word of " + std::to_string(h_ctr[kCtrMaxSym]) + " symbols: the merge loop is quadratic "
                                          "in a word's length, words of more than " + std::to_string(cap) +
                                          " symbols are not supported");

    // 3. initial symbols and merges
    tok.ensure((size_t)n_sym + 1);
    state.ensure(4 * n_state + 1);
    B.tok = tok.p;
    B.state = state.p;
    HIPT(launch_merge(M, B, n_runs, n2, n3, s));
    HIPT(hipEventRecord(ev[3], s));

    // 4. emit
    scan(fcnt.p, wpos.p, n_runs);
    uint32_t n_ids = 0, n_empty = 0;
    if (virt) {
      eflag.ensure(n + 1);
      ebefore.ensure(n + 1);
      HIPT(launch_empty_flags(B, eflag.p, s));
      scan(eflag.p, ebefore.p, n);
      B.empty_before = ebefore.p;
      HIPT(hipMemcpyAsync(&n_empty, ebefore.p + n, 4, hipMemcpyDeviceToHost, s));
    }
    HIPT(hipMemcpyAsync(&n_ids, wpos.p + n_runs, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (n_ids > n_sym || n_empty > n) throw_error(CTOK_E_DEVICE, "models encode: more ids than symbols");
    const uint64_t total = (uint64_t)n_ids + n_empty;
    ids.ensure(total + 1);
    HIPT(launch_emit(M, B, n_runs, ids.p, tok_off.p, s));
    HIPT(hipEventRecord(ev[4], s));
    h_ids.resize(total);
    if (total) HIPT(hipMemcpyAsync(h_ids.data(), ids.p, total * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(h_tok_off.data(), tok_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    for (int i = 0; i < CTOK_MODELS_STAGES; i++) {
      float ms = 0;
      HIPT(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      stage_ms[i] = ms;
    }
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

int create(strmerge::Kind kind, const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
           uint64_t n_vocab, const uint8_t* merge_bytes, const uint64_t* merge_off, uint64_t n_merge_strings,
           const char* suffix, const char* unk_token, int add_prefix_space, int device, ctok_sm_model** out) {
  if (!out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    if (!unk_token || !suffix || (n_vocab && !vocab_id)) throw_error(CTOK_E_ARG, "null argument");
    if (n_merge_strings & 1) throw_error(CTOK_E_ARG, "the merges are pairs: an odd number of strings was given");
    const std::vector<std::string> vs = strings_of(vocab_bytes, vocab_off, n_vocab, "vocab");
    const std::vector<std::string> ms = strings_of(merge_bytes, merge_off, n_merge_strings, "merges");
    std::vector<std::pair<std::string, uint32_t>> vocab;
    vocab.reserve(n_vocab);
    for (uint64_t i = 0; i < n_vocab; i++) vocab.emplace_back(vs[i], vocab_id[i]);
    std::vector<std::pair<std::string, std::string>> merges;
    merges.reserve(ms.size() / 2);
    for (size_t i = 0; i + 1 < ms.size(); i += 2) merges.emplace_back(ms[i], ms[i + 1]);
    auto m = std::make_unique<ctok_sm_model>();
    m->kind = kind;
    m->n_vocab = n_vocab;
    m->prefix_space = add_prefix_space != 0;
    m->device = device;
    std::string err;
    const int rc = strmerge::compile(kind, vocab, merges, suffix, unk_token, &m->c, &err);
    if (rc != strmerge::kOk) throw_error(rc, err);
    m->to_device();
    *out = m.release();
  });
}

int encode_batch(ctok_sm_model* m, strmerge::Kind kind, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                 const uint32_t** ids, const uint64_t** tok_off) {
  return ctok_host::run_guarded([&] {
    if (!m || !ids || !tok_off || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    if (m->kind != kind) throw_error(CTOK_E_ARG, "the handle is another model's");
    m->encode(utf8, off, n_texts);
    *ids = m->h_ids.data();
    *tok_off = m->h_tok_off.data();
  });
}

}  // namespace

extern "C" {

int ctok_wl_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                         uint64_t n_vocab, const char* unk_token, int device, ctok_wl_model** out) {
  return create(strmerge::kWordLevel, vocab_bytes, vocab_off, vocab_id, n_vocab, nullptr, nullptr, 0, "", unk_token, 0,
                device, out);
}

int ctok_cbpe_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                           uint64_t n_vocab, const uint8_t* merge_bytes, const uint64_t* merge_off,
                           uint64_t n_merge_strings, const char* end_of_word_suffix, const char* unk_token,
                           int device, ctok_cbpe_model** out) {
  return create(strmerge::kCharBpe, vocab_bytes, vocab_off, vocab_id, n_vocab, merge_bytes, merge_off, n_merge_strings,
                end_of_word_suffix, unk_token, 0, device, out);
}

int ctok_blbpe_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id,
                            uint64_t n_vocab, const uint8_t* merge_bytes, const uint64_t* merge_off,
                            uint64_t n_merge_strings, const char* unk_token, int add_prefix_space, int device,
                            ctok_blbpe_model** out) {
  return create(strmerge::kByteLevel, vocab_bytes, vocab_off, vocab_id, n_vocab, merge_bytes, merge_off, n_merge_strings,
                "", unk_token, add_prefix_space, device, out);
}

void ctok_wl_model_destroy(ctok_wl_model* m) { delete m; }
void ctok_cbpe_model_destroy(ctok_cbpe_model* m) { delete m; }
void ctok_blbpe_model_destroy(ctok_blbpe_model* m) { delete m; }
uint64_t ctok_wl_model_vocab_size(const ctok_wl_model* m) { return m ? m->n_vocab : 0; }
uint64_t ctok_cbpe_model_vocab_size(const ctok_cbpe_model* m) { return m ? m->n_vocab : 0; }
uint64_t ctok_blbpe_model_vocab_size(const ctok_blbpe_model* m) { return m ? m->n_vocab : 0; }

int ctok_wl_model_encode_batch(ctok_wl_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                               const uint32_t** ids, const uint64_t** tok_off) {
  return encode_batch(m, strmerge::kWordLevel, utf8, off, n_texts, ids, tok_off);
}
int ctok_cbpe_model_encode_batch(ctok_cbpe_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                 const uint32_t** ids, const uint64_t** tok_off) {
  return encode_batch(m, strmerge::kCharBpe, utf8, off, n_texts, ids, tok_off);
}
int ctok_blbpe_model_encode_batch(ctok_blbpe_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                  const uint32_t** ids, const uint64_t** tok_off) {
  return encode_batch(m, strmerge::kByteLevel, utf8, off, n_texts, ids, tok_off);
}

void ctok_models_limits(uint32_t* tier1, uint32_t* tier2, uint64_t* max_word_symbols) {
  if (tier1) *tier1 = kTier1;
  if (tier2) *tier2 = kTier2;
  if (max_word_symbols) *max_word_symbols = word_cap();
}

int ctok_models_stage_ms(const ctok_sm_model* m, double out[CTOK_MODELS_STAGES]) {
  return ctok_host::run_guarded([&] {
    if (!m || !out) throw_error(CTOK_E_ARG, "null argument");
    for (int i = 0; i < CTOK_MODELS_STAGES; i++) out[i] = m->stage_ms[i];
  });
}

}  // extern "C"
