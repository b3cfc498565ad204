// Host runtime of the WordPiece trainer and model behind include/ctok_wordpiece.h.
//
// Reference: WordPieceTrainer, src/trainers.rs:64-279, and WordPieceModel, src/models.rs:17-142
// (Complexity-ML/complexity-tokenizer v0.3.3).  This file restates their control flow; the
// O(corpus) and O(words) work runs on the GPU:
//   pretokenize (:79-89)              NFC by the tokenizer's pre-tokenization (pretokenize_device, its
//                                     piece bitmap ignored), Lowercase (lowercase.hip), the White_Space
//                                     split (bpe_train.hip k_ws_bits), the words counted per chunk in
//                                     the device hash table (wordcount.hip); the host drops the
//                                     whitespace runs and merges the chunks
//   train_from_word_freqs (:130-225)  the vocab and every string on the host; the words' longest
//                                     matches, tokens and pair counts on the device (wordpiece.hip),
//                                     the best pair by bpe_train.hip's k_pair_best
//   WordPieceModel::encode            k_wp_match over the vocab, k_wp_walk's model flavour
// A token is a string in the reference; on the device it is its key (include/ctok_wordpiece.h), so
// the pair table's key order is the tie rule and launch_pair_best is used as it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ctok_wordpiece.h"
#include "ctok_internal.h"  // ctok_dev::scan_u32, scan_u64, scan_tmp_elems
#include "host_common.h"
#include "knobs.h"
#include "lowercase_hd.h"
#include "lowercase_host.h"
#include "pair_best_hd.h"
#include "train_host_common.h"
#include "wordcount_internal.h"
#include "wordpiece_internal.h"
#include "ws_split_hd.h"

using namespace ctok_wp;
using ctok_bpe::Best;
using ctok_host::throw_error;
using ctok_train_host::DBuf;
using ctok_train_host::now_ms;
using ctok_train_host::utf8_of;

namespace {

constexpr uint32_t kKeyChar = 1u << 31;
constexpr uint32_t kKeySpill = kKeyChar + 0x110000u;

// the chars of a UTF-8 string (str::chars); not UTF-8 is an argument error
std::vector<uint32_t> chars_of(const std::string& w, const char* what) {
  std::vector<uint32_t> out;
  const uint8_t* t = (const uint8_t*)w.data();
  for (uint64_t i = 0; i < w.size();) {
    uint32_t len;
    const uint32_t c = lowercase::decode(t, w.size(), i, &len);
    if (c == lowercase::kRaw || (c >= 0x80u && len != lowercase::utf8_len(c)) || (c >= 0xD800u && c < 0xE000u) ||
        c > 0x10FFFFu)
      throw_error(CTOK_E_ARG, std::string(what) + " is not valid UTF-8");
    out.push_back(c);
    i += len;
  }
  return out;
}

struct Strings {  // the storage behind a ctok_bpe_strings view
  std::string bytes;
  std::vector<uint64_t> off{0};
  void clear() {
    bytes.clear();
    off.assign(1, 0);
  }
  void add(const std::string& s) {
    bytes += s;
    off.push_back(bytes.size());
  }
  void view(ctok_bpe_strings* v) const {
    v->bytes = (const uint8_t*)bytes.data();
    v->off = off.data();
    v->n = off.size() - 1;
  }
};

bool starts_with(const std::string& s, const std::string& p) { return s.size() >= p.size() && !s.compare(0, p.size(), p); }

// ---- Lowercase on the device -------------------------------------------------------------------------

}  // namespace

// text: n_bytes > 0 device bytes of n_docs > 0 texts (doc_off[0] = 0, doc_off[n_docs] = n_bytes)
// (declared in lowercase_host.h: the Normalizer's Lowercase step uses it too)
Lowered ctok_wp::lower_device(LowerBufs& b, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                              uint64_t n_docs, hipStream_t s, uint64_t refuse_from) {
  const uint64_t n_spans = (n_bytes + kLowerSpan - 1) / kLowerSpan;
  b.len.ensure(n_spans + 1);
  b.changed.ensure(1);
  HIPT(hipMemsetAsync(b.changed.p, 0, 4, s));
  HIPT(launch_lower_count(text, n_bytes, doc_off, n_docs, b.len.p, b.changed.p, s));
  uint32_t changed = 0;
  HIPT(hipMemcpyAsync(&changed, b.changed.p, 4, hipMemcpyDeviceToHost, s));
  HIPT(hipStreamSynchronize(s));
  if (!changed) return Lowered{text, doc_off, n_bytes, false};
  b.tmp.ensure(ctok_dev::scan_tmp_elems(n_spans + 1) + 64);
  HIPT(ctok_dev::scan_u64(b.len.p, n_spans, b.tmp.p, b.tmp.cap, s));  // len[n_spans] = the total
  uint64_t total = 0;
  HIPT(hipMemcpyAsync(&total, b.len.p + n_spans, 8, hipMemcpyDeviceToHost, s));
  HIPT(hipStreamSynchronize(s));
  if (total > n_bytes + n_bytes / 2 + 4) throw_error(CTOK_E_DEVICE, "lowercase: more output than 3/2 of the input");
  if (total >= refuse_from) throw_error(CTOK_E_CAPACITY, "lowercase: the output reaches " + std::to_string(refuse_from) + " bytes");
  b.out.ensure(total + 16);
  b.out_off.ensure(n_docs + 1);
  HIPT(hipMemsetAsync(b.out.p + total, 0, 16, s));
  HIPT(launch_lower_write(text, n_bytes, doc_off, n_docs, b.len.p, b.out.p, b.out_off.p, s));
  return Lowered{b.out.p, b.out_off.p, total, true};
}

namespace {

std::string byte_level_nfc_json() {
  // normalizer NFC with a ByteLevel pre-tokenizer (whose pieces are not used); the byte alphabet
  // as vocab so that the loader accepts the model
  std::string j = "{\"model\":{\"type\":\"BPE\",\"merges\":[],\"vocab\":{";
  int n = 0;
  for (int b = 0; b < 256; b++) {
    const bool keep = (b >= 0x21 && b <= 0x7E) || (b >= 0xA1 && b <= 0xAC) || (b >= 0xAE && b <= 0xFF);
    const std::string c = utf8_of(keep ? (uint32_t)b : 256u + (uint32_t)n++);
    if (b) j += ',';
    j += '"';
    if (c == "\"" || c == "\\") j += '\\';
    j += c + "\":" + std::to_string(b);
  }
  return j + "}},\"normalizer\":{\"type\":\"NFC\"},\"pre_tokenizer\":{\"type\":\"ByteLevel\",\"add_prefix_space\":false}}";
}

// the patterns of vocab string v (include/ctok_wordpiece.h) with symbol sym
void add_patterns(std::vector<wptab::Pattern>& pats, const std::string& v, const std::string& prefix, uint32_t sym) {
  if (v.empty()) return;
  pats.push_back(wptab::Pattern{(const uint8_t*)v.data(), (uint32_t)v.size(), 0, sym});
  if (starts_with(v, prefix) && v.size() > prefix.size())
    pats.push_back(wptab::Pattern{(const uint8_t*)v.data() + prefix.size(), (uint32_t)(v.size() - prefix.size()), 1, sym});
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

}  // namespace

// ===================================================================================== the trainer

struct ctok_wp_trainer {
  uint64_t vocab_size = 30000;
  uint32_t min_frequency = 2;
  std::vector<std::string> specials;
  std::string prefix = "##";
  uint64_t max_chars = 100;
  int device = 0;
  // the last counting and the trainings
  std::unordered_map<std::string, uint32_t> counts;
  std::unordered_map<std::string, uint32_t> vocab;  // never cleared: a second training starts from it
  std::vector<std::pair<std::string, std::string>> merges;
  std::vector<std::string> words;                    // of the last training, sorted
  std::unordered_map<uint32_t, std::string> key_str;  // the tokens' keys
  ctok_wp_trainer_info st{};
  // views handed out
  Strings v_vocab, v_merges, v_words, v_tokens, v_first, v_second;
  std::vector<uint32_t> v_vocab_id, v_freqs;
  std::vector<uint64_t> v_tok_off;
  std::vector<int64_t> v_pc;
  // device state
  ctok* pretok = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev[10] = {};
  Best* h_best = nullptr;    // pinned
  uint8_t* h_pat = nullptr;  // pinned: a round's new string
  size_t h_pat_cap = 0;
  LowerBufs lower;
  DevTable table;
  DBuf<uint8_t> wbytes, wc_bytes, d_pat;
  DBuf<uint64_t> wc_keys, wc_off, wc_tmp, keys, partial;
  DBuf<uint32_t> pbits, wc_vals, wc_used, wc_ctr, wc_cnt, wc_pos;
  DBuf<uint32_t> starts, woff, msym, mlen, tok, wstart, wlen, wfreq, dirty, ctr;
  DBuf<unsigned long long> err;  // [0] != 0: a walk's chain broke, [1] words walked
  DBuf<int64_t> vals;
  DBuf<Best> d_best;
  uint32_t cap = 0;  // of the pair table in keys / vals
  uint64_t n_tok_room = 0;

  ~ctok_wp_trainer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (h_best) (void)hipHostFree(h_best);
    if (h_pat) (void)hipHostFree(h_pat);
    if (pretok) ctok_destroy(pretok);
    if (s) (void)hipStreamDestroy(s);
  }

  void ensure_device() {
    HIPT(hipSetDevice(device));
    if (!s) HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev)
      if (!e) HIPT(hipEventCreate(&e));
    if (!h_best) HIPT(hipHostMalloc((void**)&h_best, sizeof(Best), hipHostMallocDefault));
  }

  void ensure_pretok() {
    if (pretok) return;
    const std::string j = byte_level_nfc_json();
    if (ctok_create_from_buffer(j.data(), j.size(), &pretok) != CTOK_OK)
      throw_error(CTOK_E_DEVICE, std::string("WordPiece trainer normaliser: ") + ctok_last_error());
  }

  // *into += the span between two events (both complete: the stream was synchronised)
  void add_ms(int e0, double* into) {
    float ms = 0;
    HIPT(hipEventElapsedTime(&ms, ev[e0], ev[e0 + 1]));
    *into += ms;
  }

  // ---- pretokenize (:79-89) and the word counts ------------------------------------------------------
  // The texts go to the device in text-aligned chunks of about CTOK_TRAIN_CHUNK_BYTES (a longer
  // text is a chunk by itself), as in ctok_trainer_count.
  void count(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    counts.clear();
    st.chunks = st.host_chunks = st.rerun_chunks = st.lowered_chunks = 0;
    st.ms_count = 0;
    ensure_device();
    ensure_pretok();
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    uint64_t chunk = 256ull << 20;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_CHUNK_BYTES")) chunk = std::max<uint64_t>(1, *e);
    std::vector<uint64_t> coff;
    for (uint64_t d0 = 0; d0 < n;) {
      uint64_t d1 = d0 + 1;  // at least one text per chunk
      while (d1 < n && off[d1 + 1] - off[d0] <= chunk) d1++;
      if (off[d1] - off[d0] >= 0xA0000000ull) throw_error(CTOK_E_CAPACITY, "a text of 2.5 GiB or more");
      coff.resize(d1 - d0 + 1);
      for (uint64_t i = d0; i <= d1; i++) coff[i - d0] = off[i] - off[d0];
      st.chunks++;
      count_chunk(utf8 + off[d0], coff.data(), d1 - d0);
      d0 = d1;
    }
  }

  // a drained "word" that is a run of whitespace is dropped; the others are added up
  void add_word(const char* p, uint64_t len, uint32_t c) {
    if (!len || wsplit::ws_at((const uint8_t*)p, len, 0)) return;
    counts[std::string(p, len)] += c;
  }

  // One chunk: NFC, Lowercase and the split on the device, then the counting of the BPE trainer's
  // count_chunk_device (same table sizes, same second attempt); a chunk whose table overflows or
  // cannot be allocated is split by a host walk over the device's lower-cased text.
  void count_chunk(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    if (!off[n]) return;
    uint64_t slot_cap = 1ull << 31;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_COUNT_SLOTS")) slot_cap = std::max<uint64_t>(2, std::min<uint64_t>(slot_cap, *e));
    auto pow2_in_cap = [&](uint64_t want) {
      uint64_t c = 1024;
      while (c < want && c < (1ull << 31)) c <<= 1;
      while (c > slot_cap) c >>= 1;
      return c;
    };
    ctok_host::pretokenize_device(pretok, device, utf8, off, n, [&](const ctok_host::DevicePretok& r) {
      hipStream_t q = (hipStream_t)r.stream;
      if (!r.n_bytes) return;
      HIPT(hipEventRecord(ev[0], q));
      const Lowered L = lower_device(lower, r.text, r.n_bytes, r.doc_off, r.n_docs, q);
      if (L.changed) st.lowered_chunks++;
      if (L.n_bytes >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a chunk of 4 GiB or more");
      const uint64_t nb = L.n_bytes;
      const uint32_t n_words = (uint32_t)((nb + 31) / 32);
      pbits.ensure(n_words);
      wc_ctr.ensure(ctok_wc::kNumCtr);
      HIPT(hipMemsetAsync(wc_ctr.p, 0, ctok_wc::kNumCtr * 4, q));
      const ctok_wc::Text x{L.text, pbits.p, (uint32_t)nb, n_words};
      uint32_t c[ctok_wc::kNumCtr] = {0, 0, 0, 0};
      HIPT(ctok_bpe::launch_ws_bits(L.text, (uint32_t)nb, L.doc_off, r.n_docs, pbits.p, q));
      HIPT(ctok_wc::launch_pieces(x, wc_ctr.p, q));
      HIPT(hipEventRecord(ev[1], q));
      HIPT(hipMemcpyAsync(c, wc_ctr.p, ctok_wc::kNumCtr * 4, hipMemcpyDeviceToHost, q));
      HIPT(hipStreamSynchronize(q));
      add_ms(0, &st.ms_count);
      const uint64_t pieces = c[ctok_wc::kCtrPieces];
      uint64_t tcap = pow2_in_cap(pieces / 2);
      for (int attempt = 0; attempt < 2; attempt++) {
        if (!wc_keys.try_ensure(tcap) || !wc_vals.try_ensure(tcap) || !wc_used.try_ensure(tcap)) break;
        HIPT(hipEventRecord(ev[0], q));
        HIPT(hipMemsetAsync(wc_keys.p, 0xFF, tcap * 8, q));
        HIPT(hipMemsetAsync(wc_vals.p, 0, tcap * 4, q));
        HIPT(hipMemsetAsync(wc_ctr.p, 0, ctok_wc::kNumCtr * 4, q));
        const ctok_wc::Table T{wc_keys.p, wc_vals.p, (uint32_t)(tcap - 1), wc_used.p, wc_ctr.p};
        HIPT(ctok_wc::launch_count(x, T, 1, q));
        HIPT(hipEventRecord(ev[1], q));
        HIPT(hipMemcpyAsync(c, wc_ctr.p, ctok_wc::kNumCtr * 4, hipMemcpyDeviceToHost, q));
        HIPT(hipStreamSynchronize(q));
        add_ms(0, &st.ms_count);
        if (!c[ctok_wc::kCtrOverflow]) {
          drain_chunk(x, T, c[ctok_wc::kCtrUsed], q);
          return;
        }
        const uint64_t larger = pow2_in_cap(2 * pieces);
        if (attempt == 1 || larger <= tcap) break;
        tcap = larger;
        st.rerun_chunks++;
      }
      // the host walk, text by text, by the kernel's rule (ws_split_hd.h)
      st.host_chunks++;
      std::vector<uint8_t> h_text(nb);
      std::vector<uint64_t> h_off(r.n_docs + 1);
      HIPT(hipMemcpyAsync(h_text.data(), L.text, nb, hipMemcpyDeviceToHost, q));
      HIPT(hipMemcpyAsync(h_off.data(), L.doc_off, h_off.size() * 8, hipMemcpyDeviceToHost, q));
      HIPT(hipStreamSynchronize(q));
      for (uint64_t d = 0; d < r.n_docs; d++) {
        if (h_off[d] > h_off[d + 1] || h_off[d + 1] > nb) throw_error(CTOK_E_DEVICE, "lowercase: offsets out of order");
        const uint8_t* t = h_text.data() + h_off[d];
        const uint64_t len = h_off[d + 1] - h_off[d];
        for (uint64_t p = 0; p < len;) {
          uint64_t e = p + 1;
          while (e < len && !wsplit::run_start(t, len, e)) e++;
          add_word((const char*)t + p, e - p, 1);
          p = e;
        }
      }
    });
  }

  void drain_chunk(const ctok_wc::Text& x, const ctok_wc::Table& T, uint32_t n_used, hipStream_t q) {
    if (!n_used) return;
    wc_off.ensure((uint64_t)n_used + 1);
    wc_cnt.ensure(n_used);
    wc_pos.ensure(n_used);
    wc_tmp.ensure(ctok_wc::drain_tmp_elems(n_used));
    wc_bytes.ensure(x.n_bytes);  // distinct words' first occurrences are disjoint pieces of the text
    HIPT(hipEventRecord(ev[0], q));
    HIPT(ctok_wc::launch_drain(x, T, n_used, wc_bytes.p, wc_off.p, wc_cnt.p, wc_pos.p, wc_tmp.p, wc_tmp.cap, q));
    HIPT(hipEventRecord(ev[1], q));
    std::vector<uint64_t> h_off((size_t)n_used + 1);
    std::vector<uint32_t> h_cnt(n_used);
    HIPT(hipMemcpyAsync(h_off.data(), wc_off.p, h_off.size() * 8, hipMemcpyDeviceToHost, q));
    HIPT(hipMemcpyAsync(h_cnt.data(), wc_cnt.p, h_cnt.size() * 4, hipMemcpyDeviceToHost, q));
    HIPT(hipStreamSynchronize(q));
    add_ms(0, &st.ms_count);
    const uint64_t nb = h_off[n_used];
    if (nb > x.n_bytes) throw_error(CTOK_E_DEVICE, "word counting: drained more bytes than the text holds");
    std::vector<char> h_bytes(nb);
    if (nb) HIPT(hipMemcpyAsync(h_bytes.data(), wc_bytes.p, nb, hipMemcpyDeviceToHost, q));
    HIPT(hipStreamSynchronize(q));
    for (uint32_t i = 0; i < n_used; i++) {
      if (h_off[i] > h_off[i + 1] || h_off[i + 1] > nb) throw_error(CTOK_E_DEVICE, "word counting: drained offsets out of order");
      add_word(h_bytes.data() + h_off[i], h_off[i + 1] - h_off[i], h_cnt[i]);
    }
  }

  // ---- train_from_word_freqs (:130-225) --------------------------------------------------------------
  // A training that fails leaves the vocab as it was before the call (merges and words are empty
  // then, as after any failed call).
  void train(const std::unordered_map<std::string, uint32_t>& word_freqs) {
    const std::unordered_map<std::string, uint32_t> before = vocab;
    try {
      train_steps(word_freqs);
    } catch (...) {
      vocab = before;
      merges.clear();
      words.clear();
      key_str.clear();
      cap = 0;
      throw;
    }
  }

  void train_steps(const std::unordered_map<std::string, uint32_t>& word_freqs) {
    const double t_start = now_ms();
    struct Stop {  // (ms_host also when a step throws)
      ctok_wp_trainer_info& i;
      double t0;
      ~Stop() { i.ms_host = now_ms() - t0; }
    } stop{st, t_start};
    merges.clear();
    words.clear();
    key_str.clear();
    st.words = st.unique_words = st.initial_vocab = st.merges = st.table_capacity = st.rebuilds = st.walked_words = 0;
    st.ms_match = st.ms_pairs = st.ms_add = st.ms_walk = st.ms_best = 0;
    cap = 0;
    ensure_device();
    const ctok_rt::BpeTrainKnobs knobs;
    const bool recount = ctok_rt::WpTrainKnobs().recount;

    // the words counted min_frequency times or more (:132-135), in byte order (the reference's
    // order is HashMap order; results do not depend on it)
    std::vector<std::pair<std::string, uint32_t>> wf;
    for (const auto& kv : word_freqs)
      if (kv.second >= min_frequency && !kv.first.empty()) wf.push_back(kv);
    std::sort(wf.begin(), wf.end());

    // the specials (:138-142: a repeated one overwrites its id, next_id still moves on), then the
    // chars in ascending code point order (:145-159)
    uint64_t next_id = 0;
    for (const auto& t : specials) vocab[t] = (uint32_t)next_id++;
    std::vector<std::vector<uint32_t>> wchars(wf.size());
    std::set<uint32_t> chars, later;  // later: chars that follow another in a word
    uint64_t n_chars = 0, n_wbytes = 0;
    for (size_t i = 0; i < wf.size(); i++) {
      wchars[i] = chars_of(wf[i].first, "a word");
      chars.insert(wchars[i].begin(), wchars[i].end());
      later.insert(wchars[i].begin() + 1, wchars[i].end());
      n_chars += wchars[i].size();
      n_wbytes += wf[i].first.size();
      st.words += wf[i].second;
    }
    st.unique_words = wf.size();
    for (uint32_t c : chars) {
      const std::string t = utf8_of(c);
      if (!vocab.count(t)) vocab[t] = (uint32_t)next_id++;
    }
    if (n_wbytes >= 0xFFFFFF00ull || n_chars >= 0xFFFFFFF0ull) throw_error(CTOK_E_CAPACITY, "4 GiB or more of unique words");
    st.initial_vocab = vocab.size();

    // the tokens' keys (include/ctok_wordpiece.h)
    std::unordered_map<std::string, uint32_t> str_key;
    std::set<uint32_t> taken;
    uint64_t spill = kKeySpill;
    auto give_key = [&](const std::string& t, uint32_t id) {
      if (id >= kKeyChar) throw_error(CTOK_E_ARG, "a vocab id of 2^31 or more");
      uint32_t k = id;
      if (!taken.insert(k).second) {
        if (spill >= 0xFFFFFFFEull) throw_error(CTOK_E_CAPACITY, "no free token key is left");
        k = (uint32_t)spill++;
        taken.insert(k);
      }
      str_key[t] = k;
      key_str[k] = t;
      return k;
    };
    {
      std::vector<std::pair<uint32_t, std::string>> by_id;
      for (const auto& kv : vocab) by_id.emplace_back(kv.second, kv.first);
      std::sort(by_id.begin(), by_id.end());
      for (const auto& e : by_id) give_key(e.second, e.first);
    }

    // the string table of the whole training: the current vocab, and prefix + char for every char
    // behind a word's first (tokenize_for_training's fallback, whether or not it is a key)
    std::vector<wptab::Pattern> pats;
    std::vector<std::string> fallback;  // (storage of the patterns that are no vocab strings)
    for (const auto& kv : vocab) add_patterns(pats, kv.first, prefix, str_key.at(kv.first));
    fallback.reserve(later.size());
    for (uint32_t c : later) {
      const std::string t = prefix + utf8_of(c);
      if (vocab.count(t)) continue;
      key_str[kKeyChar + c] = t;
      fallback.push_back(utf8_of(c));
      pats.push_back(wptab::Pattern{(const uint8_t*)fallback.back().data(), (uint32_t)fallback.back().size(), 1, kKeyChar + c});
    }
    table.upload(pats, s);

    // the words on the device: their bytes behind each other with a start bit per word, and the
    // CSR of their tokens with room for a token per char
    const uint64_t W = wf.size();
    {
      std::vector<uint8_t> h_bytes;
      std::vector<uint32_t> h_woff{0}, h_start{0}, h_freq, h_bits((n_wbytes + 31) / 32 + 1, 0);
      h_bytes.reserve(n_wbytes + 16);
      for (size_t i = 0; i < W; i++) {
        h_bits[h_bytes.size() >> 5] |= 1u << (h_bytes.size() & 31);
        h_bytes.insert(h_bytes.end(), wf[i].first.begin(), wf[i].first.end());
        h_woff.push_back((uint32_t)h_bytes.size());
        h_start.push_back(h_start.back() + (uint32_t)wchars[i].size());
        h_freq.push_back(wf[i].second);
        words.push_back(wf[i].first);
      }
      h_bytes.resize(n_wbytes + 16, 0);
      wchars.clear();
      wchars.shrink_to_fit();
      wbytes.ensure(n_wbytes + 16);
      starts.ensure(h_bits.size());
      woff.ensure(W + 1);
      msym.ensure(n_wbytes + 1);
      mlen.ensure(n_wbytes + 1);
      tok.ensure(n_chars + 1);
      wstart.ensure(W + 1);
      wlen.ensure(W + 1);
      wfreq.ensure(W + 1);
      dirty.ensure(W + 1);
      err.ensure(2);
      ctr.ensure(ctok_bpe::kNumCtr);
      partial.ensure(2 * ctok_bpe::kBestBlocks);
      d_best.ensure(1);
      HIPT(hipMemcpyAsync(wbytes.p, h_bytes.data(), h_bytes.size(), hipMemcpyHostToDevice, s));
      HIPT(hipMemcpyAsync(starts.p, h_bits.data(), h_bits.size() * 4, hipMemcpyHostToDevice, s));
      HIPT(hipMemcpyAsync(woff.p, h_woff.data(), (W + 1) * 4, hipMemcpyHostToDevice, s));
      HIPT(hipMemcpyAsync(wstart.p, h_start.data(), (W + 1) * 4, hipMemcpyHostToDevice, s));
      if (W) HIPT(hipMemcpyAsync(wfreq.p, h_freq.data(), W * 4, hipMemcpyHostToDevice, s));
      HIPT(hipMemsetAsync(wlen.p, 0, (W + 1) * 4, s));
      HIPT(hipMemsetAsync(dirty.p, 0, (W + 1) * 4, s));
      HIPT(hipMemsetAsync(err.p, 0, 16, s));
      HIPT(hipStreamSynchronize(s));  // (the host vectors go out of use)
    }
    n_tok_room = n_chars;
    const Text X{wbytes.p, starts.p, (uint32_t)n_wbytes};
    const Matches M{msym.p, mlen.p};
    const Words Wd{tok.p, wstart.p, wlen.p, wfreq.p, (uint32_t)W};

    enum { kEvMatch = 0, kEvBest = 2, kEvAdd = 4, kEvWalk = 6, kEvPairs = 8 };
    // every position's longest match and every word's tokens, once
    HIPT(hipEventRecord(ev[kEvMatch], s));
    HIPT(launch_match(X, table.view, false, M, s));
    HIPT(launch_walk_train(woff.p, M, Wd, nullptr, dirty.p, true, err.p, s));
    HIPT(hipEventRecord(ev[kEvMatch + 1], s));
    HIPT(hipStreamSynchronize(s));
    add_ms(kEvMatch, &st.ms_match);

    // The pair table, its rebuild and grow rules and the search: those of the BPE trainer
    // (bpe_train_host.cpp), on its kernels.
    const uint64_t cap_limit = std::max<uint64_t>(1, std::min<uint64_t>(1ull << 30, knobs.slots.value_or(1ull << 30)));
    const uint64_t n_sym = key_str.size();
    const uint64_t max_pairs = std::min<uint64_t>(n_chars, n_sym * n_sym);
    uint64_t want_cap = 64;
    while (want_cap < 2 * max_pairs && want_cap < (1ull << 22)) want_cap <<= 1;
    want_cap = std::min(want_cap, cap_limit);

    bool add_pending = false, pairs_pending = false;
    auto ptable = [&] { return Table{keys.p, vals.p, cap, ctr.p}; };
    auto rebuild = [&] {
      keys.ensure(want_cap);
      vals.ensure(want_cap);
      cap = (uint32_t)want_cap;
      HIPT(hipMemsetAsync(keys.p, 0xFF, (size_t)cap * 8, s));
      HIPT(hipMemsetAsync(vals.p, 0, (size_t)cap * 8, s));
      HIPT(hipMemsetAsync(ctr.p, 0, ctok_bpe::kNumCtr * 4, s));
      HIPT(hipEventRecord(ev[kEvPairs], s));
      HIPT(ctok_bpe::launch_pair_count(Wd, ptable(), s));
      HIPT(hipEventRecord(ev[kEvPairs + 1], s));
      pairs_pending = true;
    };
    auto search = [&]() -> Best {
      HIPT(hipEventRecord(ev[kEvBest], s));
      HIPT(ctok_bpe::launch_pair_best(ptable(), partial.p, d_best.p, s));
      HIPT(hipEventRecord(ev[kEvBest + 1], s));
      HIPT(hipMemcpyAsync(h_best, d_best.p, sizeof(Best), hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      add_ms(kEvBest, &st.ms_best);
      if (add_pending) add_ms(kEvAdd, &st.ms_add), add_ms(kEvWalk, &st.ms_walk);
      if (pairs_pending) add_ms(kEvPairs, &st.ms_pairs);
      add_pending = pairs_pending = false;
      return *h_best;
    };

    bool need_rebuild = true;
    uint64_t n_builds = 0, threshold = 0;
    while (vocab.size() < vocab_size) {
      const bool rebuilt = need_rebuild || recount;
      if (rebuilt) {
        rebuild();
        n_builds++;
        need_rebuild = false;
      }
      const Best r = search();
      if (r.overflow) {  // (each turn of this branch either rebuilds once or grows the table, so it ends)
        if (rebuilt) {
          if (cap >= cap_limit)
            throw_error(CTOK_E_ARG, "the pair table of " + std::to_string(cap) +
                                        " slots (CTOK_BPE_TRAIN_SLOTS) cannot hold the training's live pairs");
          want_cap = std::min<uint64_t>(cap_limit, (uint64_t)cap * 4);
        }
        need_rebuild = true;
        continue;
      }
      if (rebuilt) {  // r.taken = the live pairs
        if (r.taken * 2 > cap && cap < cap_limit) {
          want_cap = std::min<uint64_t>(cap_limit, std::max<uint64_t>((uint64_t)cap * 2, r.taken * 4));
          need_rebuild = true;
        }
        threshold = r.taken * 2 > cap ? cap : cap / 2;
      } else if (r.taken > threshold) {
        need_rebuild = true;
      }
      if (r.count <= 0) break;  // pair_freqs.is_empty()
      if ((uint64_t)r.count >= (1ull << 32))
        throw_error(CTOK_E_ARG, "a pair count of " + std::to_string(r.count) + " does not fit the reference's u32 counts");
      const auto ia = key_str.find((uint32_t)(r.key >> 32)), ib = key_str.find((uint32_t)r.key);
      if (ia == key_str.end() || ib == key_str.end()) throw_error(CTOK_E_DEVICE, "pair search returned an unknown token");
      const std::string a = ia->second, b = ib->second;
      const std::string merged = a + (starts_with(b, prefix) ? b.substr(prefix.size()) : b);  // :204-208
      if (vocab.count(merged))
        throw_error(CTOK_E_ARG, "the merged string of a round is already in the vocab (the reference would not end)");
      if (next_id >= kKeyChar) throw_error(CTOK_E_ARG, "a vocab id of 2^31 or more");
      vocab[merged] = (uint32_t)next_id;
      const uint32_t sym = give_key(merged, (uint32_t)next_id);
      next_id++;
      merges.emplace_back(a, b);
      // the new string's two patterns, then the words it changed
      const uint32_t len0 = (uint32_t)merged.size();
      const uint32_t skip = starts_with(merged, prefix) && merged.size() > prefix.size() ? (uint32_t)prefix.size() : len0;
      const uint32_t len1 = len0 - skip;  // (0: no pattern in form 1)
      if (len0 + 16 > h_pat_cap) {
        if (h_pat) (void)hipHostFree(h_pat);
        h_pat = nullptr;
        h_pat_cap = 0;
        HIPT(hipHostMalloc((void**)&h_pat, 2 * (size_t)len0 + 64, hipHostMallocDefault));
        h_pat_cap = 2 * (size_t)len0 + 64;
        d_pat.ensure(h_pat_cap);
      }
      std::memcpy(h_pat, merged.data(), len0);  // (the round before is complete: search() synchronised)
      HIPT(hipMemcpyAsync(d_pat.p, h_pat, len0, hipMemcpyHostToDevice, s));
      HIPT(hipEventRecord(ev[kEvAdd], s));
      // merged = prefix + one char: the positions that hold that char's fallback token (the same
      // string, which was no key until now) take the new key; the fallback symbol goes out of use
      uint32_t relabel = wptab::kNone;
      if (len1) {
        const std::vector<uint32_t> rest = chars_of(merged.substr(skip), "a merged string");
        if (rest.size() == 1 && key_str.count(kKeyChar + rest[0])) relabel = kKeyChar + rest[0];
      }
      HIPT(launch_add(X, d_pat.p, len0, d_pat.p + skip, len1, sym, relabel, M, woff.p, (uint32_t)W, dirty.p, s));
      HIPT(hipEventRecord(ev[kEvAdd + 1], s));
      HIPT(hipEventRecord(ev[kEvWalk], s));
      const Table T = ptable();
      HIPT(launch_walk_train(woff.p, M, Wd, recount ? nullptr : &T, dirty.p, recount, err.p, s));
      HIPT(hipEventRecord(ev[kEvWalk + 1], s));
      if (relabel != wptab::kNone) key_str.erase(relabel);  // (the walk leaves no token and no live pair with it)
      add_pending = true;
    }
    // (recount: the last round's walk came after the last count; the table handed to pair_counts
    // is that of the final words in either mode)
    if (recount && add_pending && cap) rebuild(), n_builds++;
    unsigned long long h_err[2] = {0, 0};
    HIPT(hipMemcpyAsync(h_err, err.p, 16, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (add_pending) add_ms(kEvAdd, &st.ms_add), add_ms(kEvWalk, &st.ms_walk);
    if (pairs_pending) add_ms(kEvPairs, &st.ms_pairs);
    if (h_err[0]) throw_error(CTOK_E_DEVICE, "a word's matches do not end at its end");
    st.merges = merges.size();
    st.table_capacity = cap;
    st.rebuilds = n_builds ? n_builds - 1 : 0;
    st.walked_words = h_err[1] - W;  // (without the first walk of every word)
  }
};

// ======================================================================================= the model

struct ctok_wp_model {
  std::unordered_map<std::string, uint32_t> vocab;
  std::string prefix, unk;
  uint64_t max_chars = 100;
  int device = 0;
  bool has_unk = false;
  uint32_t unk_id = 0;
  bool on_device = false;
  hipStream_t s = nullptr;
  DevTable table;
  DBuf<uint8_t> text;
  DBuf<uint64_t> doc_off, tok_off;
  DBuf<uint32_t> pbits, msym, mlen, cnt, pos, tmp, ids;
  std::vector<uint32_t> h_ids;
  std::vector<uint64_t> h_tok_off;

  ~ctok_wp_model() {
    if (s) (void)hipStreamDestroy(s);
  }

  void ensure_device() {
    HIPT(hipSetDevice(device));
    if (!s) HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (on_device) return;
    std::vector<wptab::Pattern> pats;
    for (const auto& kv : vocab) add_patterns(pats, kv.first, prefix, kv.second);
    table.upload(pats, s);
    on_device = true;
  }

  void encode(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    ensure_device();
    h_ids.clear();
    h_tok_off.assign(n + 1, 0);
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
    const uint64_t nb = off[n];
    if (!nb) return;
    if (nb >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a batch of 4 GiB or more");
    const uint32_t n_words = (uint32_t)((nb + 31) / 32);
    text.ensure(nb + 16);
    doc_off.ensure(n + 1);
    tok_off.ensure(n + 1);
    pbits.ensure(n_words);
    msym.ensure(nb);
    mlen.ensure(nb);
    cnt.ensure(nb + 1);
    pos.ensure(nb + 1);
    tmp.ensure(ctok_dev::scan_tmp_elems(nb + 1) + 64);
    HIPT(hipMemcpyAsync(text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(doc_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    const Text X{text.p, pbits.p, (uint32_t)nb};
    const Matches M{msym.p, mlen.p};
    HIPT(ctok_bpe::launch_ws_bits(text.p, (uint32_t)nb, doc_off.p, n, pbits.p, s));
    HIPT(launch_match(X, table.view, true, M, s));
    HIPT(launch_model_count(X, M, max_chars, has_unk ? 1u : 0u, cnt.p, s));
    HIPT(ctok_dev::scan_u32(cnt.p, pos.p, nb, nullptr, tmp.p, tmp.cap, s));  // pos[nb] = the total
    uint32_t total = 0;
    HIPT(hipMemcpyAsync(&total, pos.p + nb, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (total > nb) throw_error(CTOK_E_DEVICE, "WordPiece encode: more ids than bytes");
    ids.ensure((uint64_t)total + 1);
    HIPT(launch_model_emit(X, M, max_chars, has_unk ? 1u : 0u, unk_id, pos.p, ids.p, doc_off.p, n, tok_off.p, s));
    h_ids.resize(total);
    if (total) HIPT(hipMemcpyAsync(h_ids.data(), ids.p, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(h_tok_off.data(), tok_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
  }
};

// =========================================================================================== C ABI

extern "C" {

int ctok_wp_trainer_create(const ctok_wp_trainer_config* cfg, ctok_wp_trainer** out) {
  if (!cfg || !out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    auto tr = std::make_unique<ctok_wp_trainer>();
    tr->vocab_size = cfg->vocab_size;
    tr->min_frequency = cfg->min_frequency;
    tr->max_chars = cfg->max_input_chars_per_word;
    tr->device = cfg->device;
    if (!cfg->continuing_subword_prefix) throw_error(CTOK_E_ARG, "null continuing_subword_prefix");
    tr->prefix = cfg->continuing_subword_prefix;
    (void)chars_of(tr->prefix, "continuing_subword_prefix");
    if (cfg->n_special && !cfg->special_off) throw_error(CTOK_E_ARG, "null special_off");
    if (cfg->n_special && cfg->special_off[cfg->n_special] && !cfg->special) throw_error(CTOK_E_ARG, "null special");
    for (uint64_t i = 0; i < cfg->n_special; i++) {
      tr->specials.emplace_back(cfg->special + cfg->special_off[i], cfg->special_off[i + 1] - cfg->special_off[i]);
      (void)chars_of(tr->specials.back(), "a special token");
    }
    *out = tr.release();
  });
}

void ctok_wp_trainer_destroy(ctok_wp_trainer* tr) { delete tr; }

int ctok_wp_trainer_count(ctok_wp_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    tr->count(utf8, off, n_texts);
  });
}

int ctok_wp_trainer_train(ctok_wp_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    tr->count(utf8, off, n_texts);
    tr->train(tr->counts);
  });
}

int ctok_wp_trainer_train_words(ctok_wp_trainer* tr, const uint8_t* words, const uint64_t* word_off,
                                const uint32_t* freqs, uint64_t n_words) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_words && (!word_off || !freqs || (word_off[n_words] && !words)))) throw_error(CTOK_E_ARG, "null argument");
    std::unordered_map<std::string, uint32_t> m;
    for (uint64_t i = 0; i < n_words; i++) {
      if (word_off[i] > word_off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      uint32_t& c = m[std::string((const char*)words + word_off[i], word_off[i + 1] - word_off[i])];
      if ((uint64_t)c + freqs[i] > 0xFFFFFFFFull) throw_error(CTOK_E_ARG, "a word's frequencies add up past u32");
      c += freqs[i];
    }
    tr->train(m);
  });
}

uint64_t ctok_wp_trainer_vocab_size(const ctok_wp_trainer* tr) { return tr ? tr->vocab.size() : 0; }

int ctok_wp_trainer_result(ctok_wp_trainer* tr, ctok_bpe_strings* vocab, const uint32_t** vocab_id,
                           ctok_bpe_strings* merges) {
  return ctok_host::run_guarded([&] {
    if (!tr || !vocab || !vocab_id || !merges) throw_error(CTOK_E_ARG, "null argument");
    std::vector<std::pair<std::string, uint32_t>> v(tr->vocab.begin(), tr->vocab.end());
    std::sort(v.begin(), v.end());
    tr->v_vocab.clear();
    tr->v_vocab_id.clear();
    for (const auto& kv : v) {
      tr->v_vocab.add(kv.first);
      tr->v_vocab_id.push_back(kv.second);
    }
    tr->v_merges.clear();
    for (const auto& m : tr->merges) {
      tr->v_merges.add(m.first);
      tr->v_merges.add(m.second);
    }
    tr->v_vocab.view(vocab);
    *vocab_id = tr->v_vocab_id.data();
    tr->v_merges.view(merges);
  });
}

int ctok_wp_trainer_word_counts(ctok_wp_trainer* tr, ctok_bpe_strings* words, const uint32_t** freqs) {
  return ctok_host::run_guarded([&] {
    if (!tr || !words || !freqs) throw_error(CTOK_E_ARG, "null argument");
    std::vector<std::pair<std::string, uint32_t>> v(tr->counts.begin(), tr->counts.end());
    std::sort(v.begin(), v.end());
    tr->v_words.clear();
    tr->v_freqs.clear();
    for (const auto& kv : v) {
      tr->v_words.add(kv.first);
      tr->v_freqs.push_back(kv.second);
    }
    tr->v_words.view(words);
    *freqs = tr->v_freqs.data();
  });
}

int ctok_wp_trainer_tokens(ctok_wp_trainer* tr, ctok_bpe_strings* words, ctok_bpe_strings* tokens,
                           const uint64_t** tok_off) {
  return ctok_host::run_guarded([&] {
    if (!tr || !words || !tokens || !tok_off) throw_error(CTOK_E_ARG, "null argument");
    tr->v_words.clear();
    tr->v_tokens.clear();
    tr->v_tok_off.assign(1, 0);
    const size_t W = tr->words.size();
    if (W) {
      HIPT(hipSetDevice(tr->device));
      std::vector<uint32_t> h_tok(tr->n_tok_room + 1), h_start(W + 1), h_len(W);
      HIPT(hipMemcpyAsync(h_tok.data(), tr->tok.p, h_tok.size() * 4, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipMemcpyAsync(h_start.data(), tr->wstart.p, (W + 1) * 4, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipMemcpyAsync(h_len.data(), tr->wlen.p, W * 4, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipStreamSynchronize(tr->s));
      for (size_t w = 0; w < W; w++) {
        tr->v_words.add(tr->words[w]);
        if (h_len[w] > h_start[w + 1] - h_start[w]) throw_error(CTOK_E_DEVICE, "a word has more tokens than chars");
        for (uint32_t i = 0; i < h_len[w]; i++) {
          const auto it = tr->key_str.find(h_tok[h_start[w] + i]);
          if (it == tr->key_str.end()) throw_error(CTOK_E_DEVICE, "a word holds an unknown token");
          tr->v_tokens.add(it->second);
        }
        tr->v_tok_off.push_back(tr->v_tokens.off.size() - 1);
      }
    }
    tr->v_words.view(words);
    tr->v_tokens.view(tokens);
    *tok_off = tr->v_tok_off.data();
  });
}

int ctok_wp_trainer_stats(const ctok_wp_trainer* tr, ctok_wp_trainer_info* out) {
  return ctok_host::run_guarded([&] {
    if (!tr || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = tr->st;
  });
}

int ctok_wp_trainer_pair_counts(ctok_wp_trainer* tr, ctok_bpe_strings* first, ctok_bpe_strings* second,
                                const int64_t** count) {
  return ctok_host::run_guarded([&] {
    if (!tr || !first || !second || !count) throw_error(CTOK_E_ARG, "null argument");
    tr->v_first.clear();
    tr->v_second.clear();
    tr->v_pc.clear();
    if (tr->cap) {
      HIPT(hipSetDevice(tr->device));
      std::vector<uint64_t> k(tr->cap);
      std::vector<int64_t> v(tr->cap);
      HIPT(hipMemcpyAsync(k.data(), tr->keys.p, (size_t)tr->cap * 8, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipMemcpyAsync(v.data(), tr->vals.p, (size_t)tr->cap * 8, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipStreamSynchronize(tr->s));
      for (uint32_t i = 0; i < tr->cap; i++) {
        if (k[i] == ctok_bpe::kEmptyKey || !v[i]) continue;
        const auto ia = tr->key_str.find((uint32_t)(k[i] >> 32)), ib = tr->key_str.find((uint32_t)k[i]);
        if (ia == tr->key_str.end() || ib == tr->key_str.end()) throw_error(CTOK_E_DEVICE, "the pair table holds an unknown token");
        tr->v_first.add(ia->second);
        tr->v_second.add(ib->second);
        tr->v_pc.push_back(v[i]);
      }
    }
    tr->v_first.view(first);
    tr->v_second.view(second);
    *count = tr->v_pc.data();
  });
}

int ctok_wp_model_create(const uint8_t* vocab_bytes, const uint64_t* vocab_off, const uint32_t* vocab_id, uint64_t n,
                         const char* continuing_subword_prefix, const char* unk_token,
                         uint64_t max_input_chars_per_word, int device, ctok_wp_model** out) {
  if (!out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    if (!continuing_subword_prefix || !unk_token || (n && (!vocab_off || !vocab_id || (vocab_off[n] && !vocab_bytes))))
      throw_error(CTOK_E_ARG, "null argument");
    auto m = std::make_unique<ctok_wp_model>();
    m->prefix = continuing_subword_prefix;
    m->unk = unk_token;
    m->max_chars = max_input_chars_per_word;
    m->device = device;
    (void)chars_of(m->prefix, "continuing_subword_prefix");
    for (uint64_t i = 0; i < n; i++) {
      if (vocab_off[i] > vocab_off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      std::string t((const char*)vocab_bytes + vocab_off[i], vocab_off[i + 1] - vocab_off[i]);
      (void)chars_of(t, "a vocab string");
      if (vocab_id[i] == wptab::kNone) throw_error(CTOK_E_ARG, "the vocab id 2^32 - 1 is not supported");
      if (!m->vocab.emplace(std::move(t), vocab_id[i]).second) throw_error(CTOK_E_ARG, "a vocab string is given twice");
    }
    const auto it = m->vocab.find(m->unk);
    m->has_unk = it != m->vocab.end();
    m->unk_id = m->has_unk ? it->second : 0;
    *out = m.release();
  });
}

void ctok_wp_model_destroy(ctok_wp_model* m) { delete m; }
uint64_t ctok_wp_model_vocab_size(const ctok_wp_model* m) { return m ? m->vocab.size() : 0; }

int ctok_wp_model_encode_batch(ctok_wp_model* m, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts,
                               const uint32_t** ids, const uint64_t** tok_off) {
  return ctok_host::run_guarded([&] {
    if (!m || !ids || !tok_off || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    m->encode(utf8, off, n_texts);
    *ids = m->h_ids.data();
    *tok_off = m->h_tok_off.data();
  });
}

int ctok_lowercase(const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, int device, uint8_t* out,
                   uint64_t out_cap, uint64_t* out_off) {
  return ctok_host::run_guarded([&] {
    if (!out_off || (n_texts && (!off || (off[n_texts] && (!utf8 || !out))))) throw_error(CTOK_E_ARG, "null argument");
    out_off[0] = 0;
    if (!n_texts) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    for (uint64_t i = 0; i < n_texts; i++) {
      if (off[i] > off[i + 1]) throw_error(CTOK_E_ARG, "offsets must not decrease");
      (void)chars_of(std::string((const char*)utf8 + off[i], off[i + 1] - off[i]), "a text");
    }
    const uint64_t nb = off[n_texts];
    if (!nb) {
      for (uint64_t i = 0; i <= n_texts; i++) out_off[i] = 0;
      return;
    }
    HIPT(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct Close {
      hipStream_t s;
      ~Close() { (void)hipStreamDestroy(s); }
    } close{s};
    LowerBufs b;
    DBuf<uint8_t> text;
    DBuf<uint64_t> doc_off;
    text.ensure(nb + 16);
    doc_off.ensure(n_texts + 1);
    HIPT(hipMemcpyAsync(text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(doc_off.p, off, (n_texts + 1) * 8, hipMemcpyHostToDevice, s));
    const Lowered L = lower_device(b, text.p, nb, doc_off.p, n_texts, s);
    if (L.n_bytes > out_cap) {
      HIPT(hipStreamSynchronize(s));
      throw_error(CTOK_E_CAPACITY, "ctok_lowercase: the output needs " + std::to_string(L.n_bytes) + " bytes");
    }
    HIPT(hipMemcpyAsync(out, L.text, L.n_bytes, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(out_off, L.doc_off, (n_texts + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
  });
}

}  // extern "C"
