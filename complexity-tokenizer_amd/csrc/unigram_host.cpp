// Host runtime of the Unigram trainer and model behind include/ctok_unigram.h.
//
// Reference: UnigramTrainer, src/trainers.rs:287-546, and UnigramModel, src/models.rs:150-299
// (Complexity-ML/complexity-tokenizer v0.3.3).  This file restates their control flow; the
// O(corpus) work runs on the GPU (unigram.hip):
//   pretokenize (:344-354)          NFC by the tokenizer's pre-tokenization (pretokenize_device, its
//                                   piece bitmap ignored), Metaspace by k_meta_*; the sentences come
//                                   back to the host, which keeps them for the training
//   the seed vocab (:392-425)       every substring counted per chunk in the device count table
//                                   (k_sub_count, the table and chunk rules of the word counting);
//                                   the host merges the chunks, sets the specials, sorts by (count
//                                   descending, bytes ascending), truncates and takes the logarithms
//   EM (:428-472)                   the string table and the lattice once per training; an iteration
//                                   uploads score[] and live[], runs k_viterbi and k_back_train and
//                                   reads count[] back; the stable sort, the truncation and the
//                                   logarithms on the host
//   UnigramModel::tokenize          the same lattice and Viterbi kernels, the model's backtrack
// This unit is built with -ffp-contract=off (csrc/Makefile): count / total and ln round once each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ctok_unigram.h"
#include "ctok_internal.h"  // ctok_dev::scan_u32, scan_u64, scan_tmp_elems
#include "host_common.h"
#include "knobs.h"
#include "train_host_common.h"
#include "unigram_hd.h"
#include "unigram_internal.h"
#include "wordcount_hd.h"

using namespace ctok_uni;
using ctok_host::throw_error;
using ctok_train_host::DBuf;
using ctok_train_host::now_ms;

namespace {

constexpr char kMeta[] = "\xE2\x96\x81";

// str::chars().count() of a UTF-8 string; not UTF-8 is an argument error
uint64_t chars_of(const uint8_t* t, uint64_t n, const char* what) {
  uint64_t chars = 0;
  for (uint64_t i = 0; i < n; chars++) {
    const uint8_t b = t[i];
    uint32_t len, c;
    if (b < 0x80u) { len = 1; c = b; }
    else if (b >= 0xC2u && b < 0xE0u) { len = 2; c = b & 0x1Fu; }
    else if (b >= 0xE0u && b < 0xF0u) { len = 3; c = b & 0x0Fu; }
    else if (b >= 0xF0u && b < 0xF5u) { len = 4; c = b & 0x07u; }
    else throw_error(CTOK_E_ARG, std::string(what) + " is not valid UTF-8");
    if (i + len > n) throw_error(CTOK_E_ARG, std::string(what) + " is not valid UTF-8");
    for (uint32_t j = 1; j < len; j++) {
      if ((t[i + j] & 0xC0u) != 0x80u) throw_error(CTOK_E_ARG, std::string(what) + " is not valid UTF-8");
      c = (c << 6) | (t[i + j] & 0x3Fu);
    }
    if ((len == 3 && c < 0x800u) || (len == 4 && c < 0x10000u) || (c >= 0xD800u && c < 0xE000u) || c > 0x10FFFFu)
      throw_error(CTOK_E_ARG, std::string(what) + " is not valid UTF-8");
    i += len;
  }
  return chars;
}
uint64_t chars_of(const std::string& s, const char* what) { return chars_of((const uint8_t*)s.data(), s.size(), what); }

struct Strings {  // the storage behind a ctok_bpe_strings view
  std::string bytes;
  std::vector<uint64_t> off{0};
  void clear() {
    bytes.clear();
    off.assign(1, 0);
  }
  void add(const char* p, size_t n) {
    bytes.append(p, n);
    off.push_back(bytes.size());
  }
  void add(const std::string& s) { add(s.data(), s.size()); }
  size_t size() const { return off.size() - 1; }
  void view(ctok_bpe_strings* v) const {
    v->bytes = (const uint8_t*)bytes.data();
    v->off = off.data();
    v->n = off.size() - 1;
  }
};

std::string byte_level_nfc_json() {
  // normalizer NFC with a ByteLevel pre-tokenizer (whose pieces are not used); the byte alphabet
  // as vocab so that the loader accepts the model
  std::string j = "{\"model\":{\"type\":\"BPE\",\"merges\":[],\"vocab\":{";
  int n = 0;
  for (int b = 0; b < 256; b++) {
    const bool keep = (b >= 0x21 && b <= 0x7E) || (b >= 0xA1 && b <= 0xAC) || (b >= 0xAE && b <= 0xFF);
    const std::string c = ctok_train_host::utf8_of(keep ? (uint32_t)b : 256u + (uint32_t)n++);
    if (b) j += ',';
    j += '"';
    if (c == "\"" || c == "\\") j += '\\';
    j += c + "\":" + std::to_string(b);
  }
  return j + "}},\"normalizer\":{\"type\":\"NFC\"},\"pre_tokenizer\":{\"type\":\"ByteLevel\",\"add_prefix_space\":false}}";
}

struct DevTable {  // a wptab table on the device
  DBuf<wptab::Slot> slots;
  DBuf<uint8_t> blob;
  wptab::View view{};
  void upload(const std::vector<wptab::Pattern>& pats, hipStream_t s) {
    wptab::Built b;
    const int rc = wptab::build(pats, &b);
    if (rc == wptab::kDuplicate) throw_error(CTOK_E_ARG, "two vocab strings give the same pattern");
    if (rc != wptab::kOk) throw_error(CTOK_E_CAPACITY, "the vocab's string table cannot be built");
    slots.ensure(b.slots.size());
    blob.ensure(b.blob.size());
    HIPT(hipMemcpyAsync(slots.p, b.slots.data(), b.slots.size() * sizeof(wptab::Slot), hipMemcpyHostToDevice, s));
    HIPT(hipMemcpyAsync(blob.p, b.blob.data(), b.blob.size(), hipMemcpyHostToDevice, s));
    HIPT(hipStreamSynchronize(s));  // (b goes out of use)
    view = wptab::View{slots.p, blob.p, (uint32_t)b.slots.size() - 1, b.max_len};
  }
};

// Sentences resident on the device with what the lattice and the Viterbi kernels index them by.
struct DevSents {
  DBuf<uint8_t> text;
  DBuf<uint64_t> soff;
  DBuf<uint32_t> bits, lead, cidx, sent_c, tmp;
  Sents x{};
  uint32_t n_chars = 0;

  // text (n_bytes, 16 spare bytes behind them zeroed) and soff (n_sent + 1) are on the device
  void index(uint64_t n_bytes, uint64_t n_sent, hipStream_t s) {
    if (n_bytes >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "4 GiB of text or more");
    x = Sents{text.p, (uint32_t)n_bytes, soff.p, n_sent};
    const uint64_t words = (n_bytes + 31) / 32 + 1;
    bits.ensure(words);
    lead.ensure(n_bytes + 1);
    cidx.ensure(n_bytes + 1);
    sent_c.ensure(n_sent + 1);
    n_chars = 0;
    if (!n_bytes) {  // (no char anywhere: every sentence is empty)
      HIPT(hipMemsetAsync(sent_c.p, 0, (n_sent + 1) * 4, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    tmp.ensure(2 * (ctok_dev::scan_tmp_elems(n_bytes + 1) + 64));  // (u64 elements of scratch in u32 words)
    HIPT(hipMemsetAsync(bits.p, 0, words * 4, s));
    HIPT(launch_sent_bits(x, bits.p, s));
    HIPT(launch_lead_flags(x, lead.p, s));
    HIPT(ctok_dev::scan_u32(lead.p, cidx.p, n_bytes, nullptr, tmp.p, tmp.cap, s));  // cidx[n_bytes] = the chars
    HIPT(launch_sent_chars(x, cidx.p, sent_c.p, s));
    HIPT(hipMemcpyAsync(&n_chars, cidx.p + n_bytes, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (n_chars > n_bytes) throw_error(CTOK_E_DEVICE, "Unigram: more chars than bytes");
  }
};

uint64_t as_usize(double x) {  // Rust's `as usize`: saturating, NaN gives 0
  if (!(x > 0.0)) return 0;
  if (x >= 18446744073709551616.0) return ~0ull;
  return (uint64_t)x;
}

}  // namespace

// ===================================================================================== the trainer

struct ctok_uni_trainer {
  uint64_t vocab_size = 8000;
  std::vector<std::string> specials;
  uint64_t initial_vocab_size = 1000000;
  double shrinking_factor = 0.75;
  uint64_t n_iterations = 16;
  uint64_t max_piece_length = 16;
  int device = 0;
  // the trainings
  std::vector<std::pair<std::string, double>> vocab;
  std::string sent_bytes;  // the last training's sentences
  std::vector<uint64_t> sent_off{0};
  std::unordered_map<std::string, uint64_t> sub_counts;
  std::vector<std::string> seed;       // the seed vocab's strings: symbol -> string
  std::vector<uint32_t> exp_sym;       // the last E-step: the vocab before its M-step as symbols,
  std::vector<uint64_t> exp_cnt;       //   and the times each was used
  std::vector<uint64_t> sizes;
  ctok_uni_trainer_info st{};
  // views handed out
  Strings v_vocab, v_sub, v_exp;
  std::vector<double> v_score;
  std::vector<uint64_t> v_sub_cnt, v_exp_cnt;
  // device state
  ctok* pretok = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev[2] = {};
  DBuf<uint64_t> m_len, m_nsent, m_tmp, wc_keys;
  DBuf<uint8_t> m_out;
  DBuf<uint64_t> m_soff;
  DBuf<uint32_t> c_bits, wc_vals, wc_used, wc_ctr, d_pos, d_len, d_cnt;
  DevSents up;  // a chunk of sentences given directly; then the whole corpus
  DevTable table;
  DBuf<uint32_t> lat, back_len, back_sym, live, err;
  DBuf<double> score;
  DBuf<unsigned long long> count;

  ~ctok_uni_trainer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (pretok) ctok_destroy(pretok);
    if (s) (void)hipStreamDestroy(s);
  }

  void ensure_device() {
    HIPT(hipSetDevice(device));
    if (!s) HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev)
      if (!e) HIPT(hipEventCreate(&e));
  }

  void ensure_pretok() {
    if (pretok) return;
    const std::string j = byte_level_nfc_json();
    if (ctok_create_from_buffer(j.data(), j.size(), &pretok) != CTOK_OK)
      throw_error(CTOK_E_DEVICE, std::string("Unigram trainer normaliser: ") + ctok_last_error());
  }

  // *into += the span between the two events (both complete: the stream was synchronised)
  void add_ms(double* into) {
    float ms = 0;
    HIPT(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *into += ms;
  }

  void reset_run() {
    sent_bytes.clear();
    sent_off.assign(1, 0);
    sub_counts.clear();
    seed.clear();
    exp_sym.clear();
    exp_cnt.clear();
    sizes.clear();
    st = ctok_uni_trainer_info{};
  }

  static uint64_t chunk_bytes() {
    uint64_t chunk = 16ull << 20;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_CHUNK_BYTES")) chunk = std::max<uint64_t>(1, *e);
    return chunk;
  }

  // ---- pretokenize (:344-354) and the substring counts (:392-405) of n texts --------------------------
  // The texts go to the device in text-aligned chunks of about CTOK_TRAIN_CHUNK_BYTES (a longer
  // text is a chunk by itself), as in ctok_trainer_count.
  void collect_texts(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    ensure_device();
    ensure_pretok();
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    const uint64_t chunk = chunk_bytes();
    std::vector<uint64_t> coff;
    for (uint64_t d0 = 0; d0 < n;) {
      uint64_t d1 = d0 + 1;  // at least one text per chunk
      while (d1 < n && off[d1 + 1] - off[d0] <= chunk) d1++;
      if (off[d1] - off[d0] >= 0x40000000ull) throw_error(CTOK_E_CAPACITY, "a text of 1 GiB or more");
      coff.resize(d1 - d0 + 1);
      for (uint64_t i = d0; i <= d1; i++) coff[i - d0] = off[i] - off[d0];
      st.chunks++;
      if (!coff.back()) {  // only empty texts: each is the sentence "▁"
        std::string b;
        std::vector<uint64_t> o{0};
        for (uint64_t i = d0; i < d1; i++) {
          b += kMeta;
          o.push_back(b.size());
        }
        count_given(b, o);
      } else {
        meta_chunk(utf8 + off[d0], coff.data(), d1 - d0);
      }
      d0 = d1;
    }
  }

  // One chunk with at least one byte: NFC and Metaspace on the device, the sentences to the host,
  // their substrings counted where they lie.
  void meta_chunk(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    ctok_host::pretokenize_device(pretok, device, utf8, off, n, [&](const ctok_host::DevicePretok& r) {
      hipStream_t q = (hipStream_t)r.stream;
      if (r.n_docs != n) throw_error(CTOK_E_DEVICE, "Unigram: the pre-tokenization lost texts");
      const uint64_t n_spans = meta_spans(r.n_bytes);
      m_len.ensure(n_spans + 1);
      m_nsent.ensure(n_spans + 1);
      m_tmp.ensure(ctok_dev::scan_tmp_elems(n_spans + 1) + 64);
      HIPT(hipEventRecord(ev[0], q));
      HIPT(launch_meta_measure(r.text, r.n_bytes, r.doc_off, r.n_docs, m_len.p, m_nsent.p, q));
      HIPT(ctok_dev::scan_u64(m_len.p, n_spans, m_tmp.p, m_tmp.cap, q));    // [n_spans] = the total
      HIPT(ctok_dev::scan_u64(m_nsent.p, n_spans, m_tmp.p, m_tmp.cap, q));
      uint64_t total = 0, ns = 0;
      HIPT(hipMemcpyAsync(&total, m_len.p + n_spans, 8, hipMemcpyDeviceToHost, q));
      HIPT(hipMemcpyAsync(&ns, m_nsent.p + n_spans, 8, hipMemcpyDeviceToHost, q));
      HIPT(hipStreamSynchronize(q));
      // a text adds 3 bytes, a space grows from 1 byte to 3
      if (total > 3 * (r.n_bytes + r.n_docs) || ns > r.n_bytes + r.n_docs || ns > total)
        throw_error(CTOK_E_DEVICE, "Metaspace: more output than the input allows");
      if (total >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a chunk of 4 GiB or more");
      m_out.ensure(total + 16);
      m_soff.ensure(ns + 1);
      HIPT(hipMemsetAsync(m_out.p + total, 0, 16, q));
      HIPT(launch_meta_write(r.text, r.n_bytes, r.doc_off, r.n_docs, m_len.p, m_nsent.p, m_out.p, m_soff.p, q));
      HIPT(hipMemcpyAsync(m_soff.p + ns, &total, 8, hipMemcpyHostToDevice, q));
      HIPT(hipEventRecord(ev[1], q));
      std::string b(total, '\0');
      std::vector<uint64_t> o(ns + 1);
      if (total) HIPT(hipMemcpyAsync(&b[0], m_out.p, total, hipMemcpyDeviceToHost, q));
      HIPT(hipMemcpyAsync(o.data(), m_soff.p, (ns + 1) * 8, hipMemcpyDeviceToHost, q));
      HIPT(hipStreamSynchronize(q));
      add_ms(&st.ms_text);
      for (uint64_t k = 0; k < ns; k++)
        if (o[k] >= o[k + 1] || o[k + 1] > total) throw_error(CTOK_E_DEVICE, "Metaspace: sentence offsets out of order");
      if (ns && o[0] != 0) throw_error(CTOK_E_DEVICE, "Metaspace: the first sentence does not start the text");
      count_sentences(Sents{m_out.p, (uint32_t)total, m_soff.p, ns}, b, o, q);
      append(b, o);
    });
  }

  void append(const std::string& b, const std::vector<uint64_t>& o) {
    const uint64_t base = sent_bytes.size();
    sent_bytes += b;
    for (size_t k = 1; k < o.size(); k++) sent_off.push_back(base + o[k]);
  }

  // sentences given on the host: to the device, counted, kept
  void count_given(const std::string& b, const std::vector<uint64_t>& o) {
    const uint64_t nb = b.size(), ns = o.size() - 1;
    if (nb >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a chunk of 4 GiB or more");
    up.text.ensure(nb + 16);
    up.soff.ensure(ns + 1);
    if (nb) HIPT(hipMemcpyAsync(up.text.p, b.data(), nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(up.text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(up.soff.p, o.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
    count_sentences(Sents{up.text.p, (uint32_t)nb, up.soff.p, ns}, b, o, s);
    append(b, o);
  }

  // The substrings of one chunk of sentences (on the device as x, on the host as b / o) into
  // sub_counts.  The table starts at half the candidates and is built once more at twice the
  // candidates when it overflows (the rule of the word counting); no capacity within
  // CTOK_TRAIN_COUNT_SLOTS or the device's memory is an error.
  void count_sentences(const Sents& x, const std::string& b, const std::vector<uint64_t>& o, hipStream_t q) {
    if (!x.n_bytes || !max_piece_length) return;
    uint64_t cands = 0, chars = 0;
    for (uint64_t k = 0; k < x.n_sent; k++) {
      uint64_t m = 0;
      for (uint64_t p = o[k]; p < o[k + 1]; p++) m += uni::is_lead((uint8_t)b[p]);
      const uint64_t L = max_piece_length;
      cands += m <= L ? m * (m + 1) / 2 : L * (L + 1) / 2 + (m - L) * L;
      chars += m;
    }
    (void)chars;
    uint64_t slot_cap = 1ull << 31;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_COUNT_SLOTS")) slot_cap = std::max<uint64_t>(2, std::min<uint64_t>(slot_cap, *e));
    auto pow2_in_cap = [&](uint64_t want) {
      uint64_t c = 1024;
      while (c < want && c < (1ull << 31)) c <<= 1;
      while (c > slot_cap) c >>= 1;
      return c;
    };
    const uint64_t words = ((uint64_t)x.n_bytes + 31) / 32 + 1;
    c_bits.ensure(words);
    wc_ctr.ensure(ctok_wc::kNumCtr);
    HIPT(hipMemsetAsync(c_bits.p, 0, words * 4, q));
    HIPT(launch_sent_bits(x, c_bits.p, q));
    uint64_t tcap = pow2_in_cap(cands / 2);
    uint32_t c[ctok_wc::kNumCtr] = {0, 0, 0, 0};
    for (int attempt = 0;; attempt++) {
      if (!wc_keys.try_ensure(tcap) || !wc_vals.try_ensure(tcap) || !wc_used.try_ensure(tcap))
        throw_error(CTOK_E_CAPACITY, "the substring count table of " + std::to_string(tcap) + " slots cannot be allocated");
      HIPT(hipEventRecord(ev[0], q));
      HIPT(hipMemsetAsync(wc_keys.p, 0xFF, tcap * 8, q));
      HIPT(hipMemsetAsync(wc_vals.p, 0, tcap * 4, q));
      HIPT(hipMemsetAsync(wc_ctr.p, 0, ctok_wc::kNumCtr * 4, q));
      const ctok_wc::Table T{wc_keys.p, wc_vals.p, (uint32_t)(tcap - 1), wc_used.p, wc_ctr.p};
      HIPT(launch_sub_count(x, c_bits.p, max_piece_length, T, q));
      HIPT(hipEventRecord(ev[1], q));
      HIPT(hipMemcpyAsync(c, wc_ctr.p, ctok_wc::kNumCtr * 4, hipMemcpyDeviceToHost, q));
      HIPT(hipStreamSynchronize(q));
      add_ms(&st.ms_count);
      st.table_capacity = std::max<uint64_t>(st.table_capacity, tcap);
      if (c[ctok_wc::kCtrOverflow] & 2u) throw_error(CTOK_E_CAPACITY, "a substring of 65535 bytes or more");
      if (!c[ctok_wc::kCtrOverflow]) {
        drain(T, c[ctok_wc::kCtrUsed], b, q);
        return;
      }
      const uint64_t larger = pow2_in_cap(2 * cands);
      if (attempt == 1 || larger <= tcap)
        throw_error(CTOK_E_CAPACITY, "the substring count table overflows at " + std::to_string(tcap) + " slots");
      tcap = larger;
      st.rerun_chunks++;
    }
  }

  void drain(const ctok_wc::Table& T, uint32_t n_used, const std::string& b, hipStream_t q) {
    if (!n_used) return;
    if (n_used > (uint64_t)T.mask + 1) throw_error(CTOK_E_DEVICE, "substring counting: more slots used than the table has");
    d_pos.ensure(n_used);
    d_len.ensure(n_used);
    d_cnt.ensure(n_used);
    HIPT(hipEventRecord(ev[0], q));
    HIPT(launch_sub_drain(T, n_used, d_pos.p, d_len.p, d_cnt.p, q));
    HIPT(hipEventRecord(ev[1], q));
    std::vector<uint32_t> pos(n_used), len(n_used), cnt(n_used);
    HIPT(hipMemcpyAsync(pos.data(), d_pos.p, (size_t)n_used * 4, hipMemcpyDeviceToHost, q));
    HIPT(hipMemcpyAsync(len.data(), d_len.p, (size_t)n_used * 4, hipMemcpyDeviceToHost, q));
    HIPT(hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)n_used * 4, hipMemcpyDeviceToHost, q));
    HIPT(hipStreamSynchronize(q));
    add_ms(&st.ms_count);
    sub_counts.reserve(sub_counts.size() + n_used);
    for (uint32_t i = 0; i < n_used; i++) {
      if (!len[i] || (uint64_t)pos[i] + len[i] > b.size()) throw_error(CTOK_E_DEVICE, "substring counting: a slot outside the text");
      sub_counts[b.substr(pos[i], len[i])] += cnt[i];
    }
  }

  // ---- train_from_sentences (:390-482) ---------------------------------------------------------------
  // sent_bytes / sent_off and sub_counts are ready.  A training that fails leaves the vocab as it
  // was before the call.
  void train(double t_start) {
    const auto before = vocab;
    try {
      train_steps();
    } catch (...) {
      vocab = before;
      exp_sym.clear();
      exp_cnt.clear();
      st.ms_host = now_ms() - t_start;
      throw;
    }
    st.ms_host = now_ms() - t_start;
  }

  void train_steps() {
    const uint64_t n_sent = sent_off.size() - 1;
    st.sentences = n_sent;
    // the seed vocab: the substrings, every special set to 1 (:408-410), sorted by count
    // descending and, the convention, bytes ascending (:413-415)
    std::vector<std::pair<std::string, uint64_t>> items;
    {
      std::unordered_map<std::string, bool> sp;  // special -> already in items
      for (const auto& t : specials) sp.emplace(t, false);
      items.reserve(sub_counts.size() + sp.size());
      for (const auto& kv : sub_counts)
        if (!sp.count(kv.first)) items.push_back(kv);
      for (const auto& kv : sp) items.emplace_back(kv.first, 1);
    }
    const auto before_in_seed = [](const std::pair<std::string, uint64_t>& a, const std::pair<std::string, uint64_t>& b) {
      return a.second != b.second ? a.second > b.second : a.first < b.first;  // (std::string compares as unsigned bytes)
    };
    if (items.size() > initial_vocab_size) {  // only the survivors are put in order
      std::nth_element(items.begin(), items.begin() + initial_vocab_size, items.end(), before_in_seed);
      items.resize(initial_vocab_size);
    }
    std::sort(items.begin(), items.end(), before_in_seed);
    double total = 0.0;
    for (const auto& it : items) total += (double)it.second;
    vocab.clear();
    for (const auto& it : items) vocab.emplace_back(it.first, std::log((double)it.second / total));
    st.seed_vocab = vocab.size();
    seed.clear();
    for (const auto& it : items) seed.push_back(it.first);
    const size_t n_seed = vocab.size();
    std::vector<uint32_t> vsym(n_seed);  // vocab entry -> seed index, the symbol of the device
    for (size_t i = 0; i < n_seed; i++) vsym[i] = (uint32_t)i;

    bool ready = false;
    Viterbi V{};
    std::vector<double> h_score;
    std::vector<uint32_t> h_live;
    std::vector<unsigned long long> h_count;
    for (uint64_t it = 0; it < n_iterations; it++) {
      if (vocab.size() <= vocab_size) break;
      if (!ready) {
        if (n_seed >= 0xFFFFFFFFull) throw_error(CTOK_E_CAPACITY, "a seed vocab of 2^32 entries or more");
        setup_em(items, &V);
        h_score.assign(n_seed, 0.0);
        h_live.assign(n_seed, 0);
        h_count.assign(n_seed, 0);
        ready = true;
      }
      // E-step (:434-441)
      std::fill(h_live.begin(), h_live.end(), 0u);
      double unk = -100.0;  // vocab_map.get("<unk>") or -100.0 (:519)
      for (size_t i = 0; i < vocab.size(); i++) {
        h_score[vsym[i]] = vocab[i].second;
        h_live[vsym[i]] = 1;
        if (vocab[i].first == "<unk>") unk = vocab[i].second;
      }
      V.fb_score = unk;
      V.fb_sym = uni::kNone;
      uint32_t h_err = 0;
      HIPT(hipMemcpyAsync(score.p, h_score.data(), n_seed * 8, hipMemcpyHostToDevice, s));
      HIPT(hipMemcpyAsync(live.p, h_live.data(), n_seed * 4, hipMemcpyHostToDevice, s));
      HIPT(hipMemsetAsync(count.p, 0, n_seed * 8, s));
      HIPT(hipMemsetAsync(err.p, 0, 4, s));
      HIPT(hipEventRecord(ev[0], s));
      HIPT(launch_viterbi(V, s));
      HIPT(launch_back_train(V, count.p, err.p, s));
      HIPT(hipEventRecord(ev[1], s));
      HIPT(hipMemcpyAsync(h_count.data(), count.p, n_seed * 8, hipMemcpyDeviceToHost, s));
      HIPT(hipMemcpyAsync(&h_err, err.p, 4, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      add_ms(&st.ms_viterbi);
      if (h_err & 2u) throw_error(CTOK_E_DEVICE, "Unigram: broken back pointers");
      if (h_err & 1u)
        throw_error(CTOK_E_PANIC, "src/trainers.rs:534: index out of bounds: no token reaches a position of a sentence");
      // M-step (:444-471)
      const uint64_t target = std::max<uint64_t>(as_usize((double)vocab.size() * shrinking_factor), vocab_size);
      std::vector<uint32_t> order(vocab.size());
      for (size_t i = 0; i < vocab.size(); i++) order[i] = (uint32_t)i;
      exp_sym = vsym;  // (the strings are made when ctok_uni_trainer_expected_counts asks)
      exp_cnt.resize(vsym.size());
      for (size_t i = 0; i < vsym.size(); i++) exp_cnt[i] = h_count[vsym[i]];
      std::stable_sort(order.begin(), order.end(),
                       [&](uint32_t a, uint32_t b) { return h_count[vsym[a]] > h_count[vsym[b]]; });
      if (order.size() > target) order.resize(target);
      double total_count = 0.0;
      for (uint32_t i : order) total_count += (double)h_count[vsym[i]];
      std::vector<std::pair<std::string, double>> nv;
      std::vector<uint32_t> ns;
      nv.reserve(order.size());
      ns.reserve(order.size());
      for (uint32_t i : order) {
        const double c = (double)h_count[vsym[i]];
        nv.emplace_back(std::move(vocab[i].first), total_count > 0.0 ? std::log(c / total_count) : -100.0);
        ns.push_back(vsym[i]);
      }
      vocab.swap(nv);
      vsym.swap(ns);
      sizes.push_back(vocab.size());
      st.iterations++;
    }
    // :475-479
    for (const auto& t : specials) {
      bool found = false;
      for (const auto& v : vocab)
        if (v.first == t) {
          found = true;
          break;
        }
      if (!found) vocab.emplace_back(t, -100.0);
    }
  }

  // the whole corpus, the string table of the seed vocab and the lattice, once per training
  void setup_em(const std::vector<std::pair<std::string, uint64_t>>& items, Viterbi* V) {
    ensure_device();
    const uint64_t nb = sent_bytes.size(), ns = sent_off.size() - 1;
    if (nb >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "sentences of 4 GiB or more");
    std::vector<wptab::Pattern> pats;
    uint64_t longest = 0;
    for (size_t i = 0; i < items.size(); i++) {
      const std::string& t = items[i].first;
      if (t.empty()) continue;  // (can never match; it stays in the vocab)
      if (t.size() >= 0xFFFFFFFFull) throw_error(CTOK_E_CAPACITY, "a vocab string of 4 GiB or more");
      pats.push_back(wptab::Pattern{(const uint8_t*)t.data(), (uint32_t)t.size(), 0, (uint32_t)i});
      uint64_t m = 0;
      for (char ch : t) m += uni::is_lead((uint8_t)ch);
      longest = std::max(longest, m);
    }
    table.upload(pats, s);
    const uint64_t wl = std::min(max_piece_length, longest);
    const uint64_t wv = max_piece_length ? std::max<uint64_t>(wl, 1) : 0;
    if (wv > kMaxWindow) throw_error(CTOK_E_CAPACITY, "a window of more than " + std::to_string(kMaxWindow) + " chars");
    st.window = wl;
    up.text.ensure(nb + 16);
    up.soff.ensure(ns + 1);
    if (nb) HIPT(hipMemcpyAsync(up.text.p, sent_bytes.data(), nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(up.text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(up.soff.p, sent_off.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
    HIPT(hipEventRecord(ev[0], s));
    up.index(nb, ns, s);
    st.chars = up.n_chars;
    const uint64_t nc = up.n_chars;
    if (!lat.try_ensure(std::max<uint64_t>(wl * nc, 1)) || !back_len.try_ensure(nc + 1) || !back_sym.try_ensure(nc + 1))
      throw_error(CTOK_E_CAPACITY, "the lattice of " + std::to_string(wl * nc) + " entries cannot be allocated");
    HIPT(launch_lattice(up.x, up.bits.p, up.cidx.p, table.view, (uint32_t)wl, up.n_chars, lat.p, s));
    HIPT(hipEventRecord(ev[1], s));
    HIPT(hipStreamSynchronize(s));
    add_ms(&st.ms_lattice);
    const size_t n_seed = items.size();
    score.ensure(n_seed);
    live.ensure(n_seed);
    count.ensure(n_seed);
    err.ensure(1);
    *V = Viterbi{up.sent_c.p, ns,      lat.p,  up.n_chars, (uint32_t)wl, (uint32_t)wv,
                 score.p,     live.p,  -100.0, uni::kNone, back_len.p,   back_sym.p};
  }
};

// ======================================================================================= the model

struct ctok_uni_model {
  std::unordered_map<std::string, uint32_t> vocab;  // string -> its last index
  std::vector<double> h_score;                       // by index
  uint32_t unk_id = 0;
  double min_score = -10.0;
  uint32_t wl = 0;
  int device = 0;
  hipStream_t s = nullptr;
  bool on_device = false;
  DevTable table;
  DevSents d;
  DBuf<double> score;
  DBuf<uint32_t> lat, back_len, back_sym, cnt, pos, ids, tmp;
  DBuf<uint64_t> tok_off;
  std::vector<uint32_t> h_ids;
  std::vector<uint64_t> h_tok_off;

  ~ctok_uni_model() {
    if (s) (void)hipStreamDestroy(s);
  }

  void ensure_device() {
    HIPT(hipSetDevice(device));
    if (!s) HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (on_device) return;
    std::vector<wptab::Pattern> pats;
    for (const auto& kv : vocab)
      if (!kv.first.empty())
        pats.push_back(wptab::Pattern{(const uint8_t*)kv.first.data(), (uint32_t)kv.first.size(), 0, kv.second});
    table.upload(pats, s);
    score.ensure(h_score.size() + 1);
    if (!h_score.empty()) HIPT(hipMemcpyAsync(score.p, h_score.data(), h_score.size() * 8, hipMemcpyHostToDevice, s));
    HIPT(hipStreamSynchronize(s));
    on_device = true;
  }

  void encode(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    h_ids.clear();
    h_tok_off.assign(n + 1, 0);
    ensure_device();
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    const uint64_t nb = off[n];
    if (!nb) return;
    if (nb >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a batch of 4 GiB or more");
    d.text.ensure(nb + 16);
    d.soff.ensure(n + 1);
    HIPT(hipMemcpyAsync(d.text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(d.text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(d.soff.p, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    d.index(nb, n, s);
    const uint64_t nc = d.n_chars;
    if (!lat.try_ensure(std::max<uint64_t>((uint64_t)wl * nc, 1)) || !back_len.try_ensure(nc + 1) || !back_sym.try_ensure(nc + 1))
      throw_error(CTOK_E_CAPACITY, "the lattice of " + std::to_string((uint64_t)wl * nc) + " entries cannot be allocated");
    cnt.ensure(n + 1);
    pos.ensure(n + 1);
    tok_off.ensure(n + 1);
    tmp.ensure(2 * (ctok_dev::scan_tmp_elems(n + 1) + 64));
    const Viterbi V{d.sent_c.p, n,       lat.p,     d.n_chars, wl,         std::max<uint32_t>(wl, 1),
                    score.p,    nullptr, min_score, unk_id,    back_len.p, back_sym.p};
    HIPT(launch_lattice(d.x, d.bits.p, d.cidx.p, table.view, wl, d.n_chars, lat.p, s));
    HIPT(launch_viterbi(V, s));
    HIPT(launch_back_count(V, cnt.p, s));
    HIPT(ctok_dev::scan_u32(cnt.p, pos.p, n, nullptr, tmp.p, tmp.cap, s));  // pos[n] = the total
    uint32_t total = 0;
    HIPT(hipMemcpyAsync(&total, pos.p + n, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (total > nc) throw_error(CTOK_E_DEVICE, "Unigram encode: more ids than chars");
    ids.ensure((uint64_t)total + 1);
    HIPT(launch_back_emit(V, pos.p, ids.p, tok_off.p, s));
    h_ids.resize(total);
    if (total) HIPT(hipMemcpyAsync(h_ids.data(), ids.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(h_tok_off.data(), tok_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
  }
};

// =========================================================================================== C ABI

extern "C" {

int ctok_uni_trainer_create(const ctok_uni_trainer_config* cfg, ctok_uni_trainer** out) {
  if (!cfg || !out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    auto tr = std::make_unique<ctok_uni_trainer>();
    tr->vocab_size = cfg->vocab_size;
    tr->initial_vocab_size = cfg->initial_vocab_size;
    tr->shrinking_factor = cfg->shrinking_factor;
    tr->n_iterations = cfg->n_iterations;
    tr->max_piece_length = cfg->max_piece_length;
    tr->device = cfg->device;
    if (cfg->n_special && !cfg->special_off) throw_error(CTOK_E_ARG, "null special_off");
    if (cfg->n_special && cfg->special_off[cfg->n_special] && !cfg->special) throw_error(CTOK_E_ARG, "null special");
    for (uint64_t i = 0; i < cfg->n_special; i++) {
      if (cfg->special_off[i] > cfg->special_off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      tr->specials.emplace_back(cfg->special + cfg->special_off[i], cfg->special_off[i + 1] - cfg->special_off[i]);
      (void)chars_of(tr->specials.back(), "a special token");
    }
    *out = tr.release();
  });
}

void ctok_uni_trainer_destroy(ctok_uni_trainer* tr) { delete tr; }

int ctok_uni_trainer_train(ctok_uni_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    const double t0 = now_ms();
    tr->reset_run();
    tr->collect_texts(utf8, off, n_texts);
    tr->train(t0);
  });
}

int ctok_uni_trainer_train_sentences(ctok_uni_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n && (!off || (off[n] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    const double t0 = now_ms();
    if (n && off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++) {
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      (void)chars_of(utf8 + off[i], off[i + 1] - off[i], "a sentence");
    }
    tr->reset_run();
    tr->ensure_device();
    const uint64_t chunk = ctok_uni_trainer::chunk_bytes();
    for (uint64_t d0 = 0; d0 < n;) {  // sentence-aligned chunks, as the texts'
      uint64_t d1 = d0 + 1;
      while (d1 < n && off[d1 + 1] - off[d0] <= chunk) d1++;
      std::string b((const char*)utf8 + off[d0], off[d1] - off[d0]);
      std::vector<uint64_t> o(d1 - d0 + 1);
      for (uint64_t i = d0; i <= d1; i++) o[i - d0] = off[i] - off[d0];
      tr->st.chunks++;
      tr->count_given(b, o);
      d0 = d1;
    }
    tr->train(t0);
  });
}

uint64_t ctok_uni_trainer_vocab_size(const ctok_uni_trainer* tr) { return tr ? tr->vocab.size() : 0; }

int ctok_uni_trainer_result(ctok_uni_trainer* tr, ctok_bpe_strings* vocab, const double** score) {
  return ctok_host::run_guarded([&] {
    if (!tr || !vocab || !score) throw_error(CTOK_E_ARG, "null argument");
    tr->v_vocab.clear();
    tr->v_score.clear();
    for (const auto& kv : tr->vocab) {
      tr->v_vocab.add(kv.first);
      tr->v_score.push_back(kv.second);
    }
    tr->v_vocab.view(vocab);
    *score = tr->v_score.data();
  });
}

int ctok_uni_trainer_sentences(ctok_uni_trainer* tr, ctok_bpe_strings* sentences) {
  return ctok_host::run_guarded([&] {
    if (!tr || !sentences) throw_error(CTOK_E_ARG, "null argument");
    sentences->bytes = (const uint8_t*)tr->sent_bytes.data();
    sentences->off = tr->sent_off.data();
    sentences->n = tr->sent_off.size() - 1;
  });
}

int ctok_uni_trainer_substring_counts(ctok_uni_trainer* tr, ctok_bpe_strings* strings, const uint64_t** count) {
  return ctok_host::run_guarded([&] {
    if (!tr || !strings || !count) throw_error(CTOK_E_ARG, "null argument");
    std::vector<std::pair<std::string, uint64_t>> v(tr->sub_counts.begin(), tr->sub_counts.end());
    std::sort(v.begin(), v.end());
    tr->v_sub.clear();
    tr->v_sub_cnt.clear();
    for (const auto& kv : v) {
      tr->v_sub.add(kv.first);
      tr->v_sub_cnt.push_back(kv.second);
    }
    tr->v_sub.view(strings);
    *count = tr->v_sub_cnt.data();
  });
}

int ctok_uni_trainer_expected_counts(ctok_uni_trainer* tr, ctok_bpe_strings* strings, const uint64_t** count) {
  return ctok_host::run_guarded([&] {
    if (!tr || !strings || !count) throw_error(CTOK_E_ARG, "null argument");
    tr->v_exp.clear();
    tr->v_exp_cnt.clear();
    for (size_t i = 0; i < tr->exp_sym.size(); i++) {
      tr->v_exp.add(tr->seed.at(tr->exp_sym[i]));
      tr->v_exp_cnt.push_back(tr->exp_cnt[i]);
    }
    tr->v_exp.view(strings);
    *count = tr->v_exp_cnt.data();
  });
}

int ctok_uni_trainer_stats(const ctok_uni_trainer* tr, ctok_uni_trainer_info* out) {
  return ctok_host::run_guarded([&] {
    if (!tr || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = tr->st;
    out->vocab_sizes = tr->sizes.data();
  });
}

int ctok_uni_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const double* score, uint64_t n,
                          const char* unk_token, int device, ctok_uni_model** out) {
  if (!out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    if (!unk_token || (n && (!vocab_off || !score || (vocab_off[n] && !vocab_bytes)))) throw_error(CTOK_E_ARG, "null argument");
    if (n >= 0xFFFFFFFFull) throw_error(CTOK_E_CAPACITY, "a vocab of 2^32 - 1 entries or more");
    auto m = std::make_unique<ctok_uni_model>();
    m->device = device;
    double min_score = 0.0;
    uint64_t longest = 0;
    for (uint64_t i = 0; i < n; i++) {
      if (vocab_off[i] > vocab_off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      std::string t((const char*)vocab_bytes + vocab_off[i], vocab_off[i + 1] - vocab_off[i]);
      longest = std::max(longest, chars_of(t, "a vocab string"));
      m->vocab[std::move(t)] = (uint32_t)i;  // a repeated string keeps its last index (:208)
      m->h_score.push_back(score[i]);
      if (score[i] < min_score) min_score = score[i];  // f64::min: a NaN is ignored (:210)
    }
    if (longest > kMaxWindow)
      throw_error(CTOK_E_CAPACITY, "a vocab string of more than " + std::to_string(kMaxWindow) + " chars");
    m->wl = (uint32_t)longest;
    const auto it = m->vocab.find(unk_token);
    m->unk_id = it != m->vocab.end() ? it->second : 0;
    m->min_score = min_score - 10.0;
    *out = m.release();
  });
}

void ctok_uni_model_destroy(ctok_uni_model* m) { delete m; }
uint64_t ctok_uni_model_vocab_size(const ctok_uni_model* m) { return m ? m->vocab.size() : 0; }

int ctok_uni_model_encode_batch(ctok_uni_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                                const uint32_t** ids, const uint64_t** tok_off) {
  return ctok_host::run_guarded([&] {
    if (!m || !ids || !tok_off || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    m->encode(utf8, off, n_texts);
    *ids = m->h_ids.data();
    *tok_off = m->h_tok_off.data();
  });
}

}  // extern "C"
