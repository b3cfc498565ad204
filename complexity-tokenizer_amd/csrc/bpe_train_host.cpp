// Host runtime of the classic frequency-BPE trainer behind include/ctok_bpe_trainer.h.
//
// Reference: BpeTrainer, src/bpe_trainer.rs (Complexity-ML/complexity-tokenizer v0.3.3).  This file
// restates its control flow step by step; the O(corpus) and O(words) work runs on the GPU:
//   build_word_frequencies (:240-273)  the White_Space split as a piece-start bitmap (bpe_train.hip
//                                      k_ws_bits), the words counted per chunk in the INL trainer's
//                                      device hash table (wordcount.hip, unchanged); the host drops
//                                      the whitespace runs and merges the chunks.  A chunk that
//                                      overflows the largest table allowed is split by a host walk
//                                      with the same rule (ws_split_hd.h)
//   build_initial_vocab (:276-320)     host
//   split_word (:323-338)              host: the words as a CSR of symbol ids
//   count_pairs (:341-375)             k_pair_count into the resident pair table
//   the loop (:143-180)                k_pair_best (two launches) + one 32-byte readback, the string
//                                      and vocab work on the host, then k_bpe_merge
// Symbols are strings in the reference; here a symbol is a dense id of its string (sym_str), so
// equal strings are one symbol.  The two orders the reference leaves to hash iteration are fixed as
// include/ctok_bpe_trainer.h states them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ctok_bpe_trainer.h"
#include "bpe_train_internal.h"
#include "host_common.h"
#include "knobs.h"
#include "pair_best_hd.h"
#include "train_host_common.h"
#include "wordcount_internal.h"
#include "ws_split_hd.h"

using namespace ctok_bpe;
using ctok_host::throw_error;
using ctok_train_host::DBuf;
using ctok_train_host::now_ms;
using ctok_train_host::utf8_of;

namespace {

// the chars of a UTF-8 word (str::chars); a word that is not UTF-8 is an argument error
std::vector<uint32_t> chars_of(const std::string& w) {
  std::vector<uint32_t> out;
  const size_t n = w.size();
  for (size_t i = 0; i < n;) {
    const uint8_t b = (uint8_t)w[i];
    const int len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 0;
    if (!len || i + len > n) throw_error(CTOK_E_ARG, "a word is not valid UTF-8");
    uint32_t c = len == 1 ? b : b & (0xFFu >> (len + 1));
    for (int j = 1; j < len; j++) {
      if (!wsplit::is_cont((uint8_t)w[i + j])) throw_error(CTOK_E_ARG, "a word is not valid UTF-8");
      c = (c << 6) | ((uint8_t)w[i + j] & 63u);
    }
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

}  // namespace

struct ctok_bpe_trainer {
  // BpeTrainerConfig (src/bpe_trainer.rs:14-51)
  uint64_t vocab_size = 30000;
  uint32_t min_frequency = 2;
  std::vector<std::string> specials;
  bool has_suffix = false, has_prefix = false;
  std::string suffix, prefix;
  int device = 0;
  // the last counting and the last training
  std::unordered_map<std::string, uint32_t> counts;
  std::unordered_map<std::string, uint32_t> vocab;
  std::vector<std::pair<std::string, std::string>> merges;
  std::vector<std::string> sym_str;
  std::unordered_map<std::string, uint32_t> sym_id;
  ctok_bpe_trainer_info st{};
  // views handed out
  Strings v_vocab, v_merges, v_words, v_syms;
  std::vector<uint32_t> v_vocab_id, v_freqs, v_pa, v_pb;
  std::vector<int64_t> v_pc;
  // device state
  hipStream_t s = nullptr;
  hipEvent_t ev[8] = {};
  Best* h_best = nullptr;  // pinned
  DBuf<uint8_t> text, wc_bytes;
  DBuf<uint64_t> doc_off, wc_keys, wc_off, wc_tmp, keys, partial;
  DBuf<uint32_t> pbits, wc_vals, wc_used, wc_ctr, wc_cnt, wc_pos, tok, wstart, wlen, wfreq, ctr;
  DBuf<int64_t> vals;
  DBuf<Best> d_best;
  uint32_t cap = 0;  // of the pair table in keys / vals

  ~ctok_bpe_trainer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (h_best) (void)hipHostFree(h_best);
    if (s) (void)hipStreamDestroy(s);
  }

  void ensure_device() {
    HIPT(hipSetDevice(device));
    if (!s) HIPT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev)
      if (!e) HIPT(hipEventCreate(&e));
    if (!h_best) HIPT(hipHostMalloc((void**)&h_best, sizeof(Best), hipHostMallocDefault));
  }

  // *into += the span between two events (both complete: the stream was synchronised)
  void add_ms(int e0, double* into) {
    float ms = 0;
    HIPT(hipEventElapsedTime(&ms, ev[e0], ev[e0 + 1]));
    *into += ms;
  }

  // ---- build_word_frequencies (:240-273), without the suffix ----------------------------------------
  // The texts go to the device in text-aligned chunks of about CTOK_TRAIN_CHUNK_BYTES (a longer
  // text is a chunk by itself), as in ctok_trainer_count: a chunk's table lives for that chunk and
  // the host adds the chunks up.
  void count(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    counts.clear();
    st.chunks = st.host_chunks = st.rerun_chunks = 0;
    st.ms_count = 0;
    ensure_device();
    if (!n) return;
    if (off[0] != 0) throw_error(CTOK_E_ARG, "offsets[0] must be 0");
    uint64_t chunk = 256ull << 20;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_CHUNK_BYTES")) chunk = std::max<uint64_t>(1, *e);
    std::vector<uint64_t> coff;
    for (uint64_t d0 = 0; d0 < n;) {
      uint64_t d1 = d0 + 1;  // at least one text per chunk
      while (d1 < n && off[d1 + 1] - off[d0] <= chunk) d1++;
      if (off[d1] - off[d0] >= 0xFFFFFF00ull) throw_error(CTOK_E_CAPACITY, "a text of 4 GiB or more");
      coff.resize(d1 - d0 + 1);
      for (uint64_t i = d0; i <= d1; i++) coff[i - d0] = off[i] - off[d0];
      st.chunks++;
      if (!count_chunk_device(utf8 + off[d0], coff.data(), d1 - d0)) {
        st.host_chunks++;
        count_chunk_host(utf8 + off[d0], coff.data(), d1 - d0);
      }
      d0 = d1;
    }
  }

  // a drained "word" that is a run of whitespace is dropped; the others are added up
  void add_word(const char* p, uint64_t len, uint32_t c) {
    if (!len || wsplit::ws_at((const uint8_t*)p, len, 0)) return;
    counts[std::string(p, len)] += c;
  }

  // One chunk on the device.  Table capacity, the second attempt with a larger table and the
  // `false` for "count it on the host" are those of the INL trainer's count_chunk_device.
  bool count_chunk_device(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    const uint64_t nb = off[n];
    if (!nb) return true;
    uint64_t slot_cap = 1ull << 31;
    if (auto e = ctok_rt::env_u64("CTOK_TRAIN_COUNT_SLOTS")) slot_cap = std::max<uint64_t>(2, std::min<uint64_t>(slot_cap, *e));
    auto pow2_in_cap = [&](uint64_t want) {
      uint64_t c = 1024;
      while (c < want && c < (1ull << 31)) c <<= 1;
      while (c > slot_cap) c >>= 1;
      return c;
    };
    const uint32_t n_words = (uint32_t)((nb + 31) / 32);
    // (the counting kernels read whole dwords up to 7 bytes past a word: 16 zero bytes behind the text)
    text.ensure(nb + 16);
    doc_off.ensure(n + 1);
    pbits.ensure(n_words);
    wc_ctr.ensure(ctok_wc::kNumCtr);
    HIPT(hipMemcpyAsync(text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(doc_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(wc_ctr.p, 0, ctok_wc::kNumCtr * 4, s));
    const ctok_wc::Text x{text.p, pbits.p, (uint32_t)nb, n_words};
    uint32_t c[ctok_wc::kNumCtr] = {0, 0, 0, 0};
    HIPT(hipEventRecord(ev[0], s));
    HIPT(launch_ws_bits(text.p, (uint32_t)nb, doc_off.p, n, pbits.p, s));
    HIPT(ctok_wc::launch_pieces(x, wc_ctr.p, s));
    HIPT(hipEventRecord(ev[1], s));
    HIPT(hipMemcpyAsync(c, wc_ctr.p, ctok_wc::kNumCtr * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    add_ms(0, &st.ms_count);
    const uint64_t pieces = c[ctok_wc::kCtrPieces];
    uint64_t tcap = pow2_in_cap(pieces / 2);
    for (int attempt = 0; attempt < 2; attempt++) {
      if (!wc_keys.try_ensure(tcap) || !wc_vals.try_ensure(tcap) || !wc_used.try_ensure(tcap)) return false;
      HIPT(hipEventRecord(ev[0], s));
      HIPT(hipMemsetAsync(wc_keys.p, 0xFF, tcap * 8, s));
      HIPT(hipMemsetAsync(wc_vals.p, 0, tcap * 4, s));
      HIPT(hipMemsetAsync(wc_ctr.p, 0, ctok_wc::kNumCtr * 4, s));
      const ctok_wc::Table T{wc_keys.p, wc_vals.p, (uint32_t)(tcap - 1), wc_used.p, wc_ctr.p};
      HIPT(ctok_wc::launch_count(x, T, 1, s));
      HIPT(hipEventRecord(ev[1], s));
      HIPT(hipMemcpyAsync(c, wc_ctr.p, ctok_wc::kNumCtr * 4, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      add_ms(0, &st.ms_count);
      if (!c[ctok_wc::kCtrOverflow]) {
        drain_chunk(x, T, c[ctok_wc::kCtrUsed]);
        return true;
      }
      const uint64_t larger = pow2_in_cap(2 * pieces);
      if (attempt == 1 || larger <= tcap) return false;
      tcap = larger;
      st.rerun_chunks++;
    }
    return false;
  }

  void drain_chunk(const ctok_wc::Text& x, const ctok_wc::Table& T, uint32_t n_used) {
    if (!n_used) return;
    wc_off.ensure((uint64_t)n_used + 1);
    wc_cnt.ensure(n_used);
    wc_pos.ensure(n_used);
    wc_tmp.ensure(ctok_wc::drain_tmp_elems(n_used));
    wc_bytes.ensure(x.n_bytes);  // distinct words' first occurrences are disjoint pieces of the text
    HIPT(hipEventRecord(ev[0], s));
    HIPT(ctok_wc::launch_drain(x, T, n_used, wc_bytes.p, wc_off.p, wc_cnt.p, wc_pos.p, wc_tmp.p, wc_tmp.cap, s));
    HIPT(hipEventRecord(ev[1], s));
    std::vector<uint64_t> h_off((size_t)n_used + 1);
    std::vector<uint32_t> h_cnt(n_used);
    HIPT(hipMemcpyAsync(h_off.data(), wc_off.p, h_off.size() * 8, hipMemcpyDeviceToHost, s));
    HIPT(hipMemcpyAsync(h_cnt.data(), wc_cnt.p, h_cnt.size() * 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    add_ms(0, &st.ms_count);
    const uint64_t nb = h_off[n_used];
    if (nb > x.n_bytes) throw_error(CTOK_E_DEVICE, "word counting: drained more bytes than the text holds");
    std::vector<char> h_bytes(nb);
    if (nb) HIPT(hipMemcpyAsync(h_bytes.data(), wc_bytes.p, nb, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n_used; i++) {
      if (h_off[i] > h_off[i + 1] || h_off[i + 1] > nb) throw_error(CTOK_E_DEVICE, "word counting: drained offsets out of order");
      add_word(h_bytes.data() + h_off[i], h_off[i + 1] - h_off[i], h_cnt[i]);
    }
  }

  // One chunk split on the host by the kernel's rule (its device table overflowed or could not be
  // allocated): every text by itself.
  void count_chunk_host(const uint8_t* utf8, const uint64_t* off, uint64_t n) {
    for (uint64_t d = 0; d < n; d++) {
      const uint8_t* t = utf8 + off[d];
      const uint64_t len = off[d + 1] - off[d];
      for (uint64_t p = 0; p < len;) {
        uint64_t q = p + 1;
        while (q < len && !wsplit::run_start(t, len, q)) q++;
        add_word((const char*)t + p, q - p, 1);
        p = q;
      }
    }
  }

  uint32_t sym_of(const std::string& str) {
    auto it = sym_id.find(str);
    if (it != sym_id.end()) return it->second;
    if (sym_str.size() >= 0xFFFFFFFEull) throw_error(CTOK_E_CAPACITY, "more than 2^32 symbols");
    const uint32_t id = (uint32_t)sym_str.size();
    sym_str.push_back(str);
    sym_id.emplace(str, id);
    return id;
  }

  // ---- train (:100-228) on word frequencies (the suffix already appended) ---------------------------
  void train(const std::vector<std::pair<std::string, uint32_t>>& wf) {
    const double t_start = now_ms();
    struct Stop {  // (ms_host also when a step throws)
      ctok_bpe_trainer_info& i;
      double t0;
      ~Stop() { i.ms_host = now_ms() - t0; }
    } stop{st, t_start};
    vocab.clear();
    merges.clear();
    sym_str.clear();
    sym_id.clear();
    st.words = st.unique_words = st.initial_symbols = st.merges = st.table_capacity = st.rebuilds = 0;
    st.ms_pairs = st.ms_best = st.ms_merges = 0;
    cap = 0;
    ensure_device();
    const ctok_rt::BpeTrainKnobs knobs;

    // build_initial_vocab (:276-320): the specials (a repeated one overwrites its id and next_id
    // still moves on), then the chars by total frequency, ties in ascending code point order
    uint32_t next_id = 0;
    for (const auto& t : specials) vocab[t] = next_id++;
    std::vector<std::vector<uint32_t>> wchars(wf.size());
    std::map<uint32_t, uint64_t> char_freq;  // ascending code point
    std::map<uint32_t, bool> follows;        // chars that follow another in a word
    for (size_t i = 0; i < wf.size(); i++) {
      wchars[i] = chars_of(wf[i].first);
      for (uint32_t c : wchars[i]) char_freq[c] += wf[i].second;
      if (has_prefix)
        for (size_t j = 1; j < wchars[i].size(); j++) follows[wchars[i][j]] = true;
      st.words += wf[i].second;
    }
    st.unique_words = wf.size();
    std::vector<std::pair<uint32_t, uint64_t>> order(char_freq.begin(), char_freq.end());
    std::stable_sort(order.begin(), order.end(), [](const auto& x, const auto& y) { return x.second > y.second; });
    std::unordered_map<uint32_t, uint32_t> plain_sym, prefixed_sym;
    for (const auto& cf : order) {
      const std::string t = utf8_of(cf.first);
      if (!vocab.count(t)) vocab[t] = next_id++;
      plain_sym[cf.first] = sym_of(t);
    }
    for (const auto& kv : follows) prefixed_sym[kv.first] = sym_of(prefix + utf8_of(kv.first));
    st.initial_symbols = sym_str.size();

    // split_word (:323-338): the CSR of symbol ids
    std::vector<uint32_t> h_tok, h_start{0}, h_len, h_freq;
    for (size_t i = 0; i < wf.size(); i++) {
      const auto& ch = wchars[i];
      for (size_t j = 0; j < ch.size(); j++) h_tok.push_back(has_prefix && j > 0 ? prefixed_sym.at(ch[j]) : plain_sym.at(ch[j]));
      if (h_tok.size() >= 0xFFFFFFF0ull) throw_error(CTOK_E_CAPACITY, "more than 2^32 word symbols");
      h_len.push_back((uint32_t)ch.size());
      h_start.push_back((uint32_t)h_tok.size());
      h_freq.push_back(wf[i].second);
    }
    wchars.clear();
    wchars.shrink_to_fit();
    const uint64_t T = h_tok.size(), W = wf.size();
    tok.ensure(T + 1);
    wstart.ensure(W + 1);
    wlen.ensure(W + 1);
    wfreq.ensure(W + 1);
    ctr.ensure(kNumCtr);
    partial.ensure(2 * kBestBlocks);
    d_best.ensure(1);
    if (T) HIPT(hipMemcpyAsync(tok.p, h_tok.data(), T * 4, hipMemcpyHostToDevice, s));
    HIPT(hipMemcpyAsync(wstart.p, h_start.data(), (W + 1) * 4, hipMemcpyHostToDevice, s));
    if (W) HIPT(hipMemcpyAsync(wlen.p, h_len.data(), W * 4, hipMemcpyHostToDevice, s));
    if (W) HIPT(hipMemcpyAsync(wfreq.p, h_freq.data(), W * 4, hipMemcpyHostToDevice, s));
    HIPT(hipStreamSynchronize(s));  // (the host vectors go out of use)
    const Words Wd{tok.p, wstart.p, wlen.p, wfreq.p, (uint32_t)W};

    // The pair table: at most half full after a rebuild where the cap allows it.  Every search
    // reads the whole table, so it starts no larger than the pairs the initial symbols can form
    // (distinct pairs <= min(T, symbols^2)); merges bring new symbols and new pairs, and a table
    // that is half full of live pairs after a rebuild grows.
    const uint64_t cap_limit = std::max<uint64_t>(1, std::min<uint64_t>(1ull << 30, knobs.slots.value_or(1ull << 30)));
    const uint64_t n_sym = sym_str.size();
    const uint64_t max_pairs = std::min<uint64_t>(T, n_sym * n_sym);
    uint64_t want_cap = 64;
    while (want_cap < 2 * max_pairs && want_cap < (1ull << 22)) want_cap <<= 1;
    want_cap = std::min(want_cap, cap_limit);

    enum { kEvBest = 2, kEvMerge = 4, kEvPairs = 6 };
    bool merge_pending = false, pairs_pending = false;
    auto table = [&] { return Table{keys.p, vals.p, cap, ctr.p}; };
    // count_pairs (:341-375) into an empty table of want_cap slots
    auto rebuild = [&] {
      keys.ensure(want_cap);
      vals.ensure(want_cap);
      cap = (uint32_t)want_cap;
      HIPT(hipMemsetAsync(keys.p, 0xFF, (size_t)cap * 8, s));
      HIPT(hipMemsetAsync(vals.p, 0, (size_t)cap * 8, s));
      HIPT(hipMemsetAsync(ctr.p, 0, kNumCtr * 4, s));
      HIPT(hipEventRecord(ev[kEvPairs], s));
      HIPT(launch_pair_count(Wd, table(), s));
      HIPT(hipEventRecord(ev[kEvPairs + 1], s));
      pairs_pending = true;
    };
    // k_pair_best and the one synchronised readback of a merge
    auto search = [&]() -> Best {
      HIPT(hipEventRecord(ev[kEvBest], s));
      HIPT(launch_pair_best(table(), partial.p, d_best.p, s));
      HIPT(hipEventRecord(ev[kEvBest + 1], s));
      HIPT(hipMemcpyAsync(h_best, d_best.p, sizeof(Best), hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
      add_ms(kEvBest, &st.ms_best);
      if (merge_pending) add_ms(kEvMerge, &st.ms_merges);
      if (pairs_pending) add_ms(kEvPairs, &st.ms_pairs);
      merge_pending = pairs_pending = false;
      return *h_best;
    };

    bool need_rebuild = true, first = true;
    uint64_t n_builds = 0, threshold = 0;
    while (vocab.size() < vocab_size) {
      const bool rebuilt = need_rebuild || knobs.recount;
      if (rebuilt) {
        rebuild();
        n_builds++;
        need_rebuild = false;
      }
      const Best r = search();
      if (r.overflow) {
        // an add found no slot.  After merges: slots of dead pairs fill the table, count again.
        // Straight after a count: the live pairs do not fit, so grow, or give up at the cap --
        // each turn of this branch either rebuilds once or grows the table, so it ends.
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
        if (r.taken * 2 > cap && cap < cap_limit) {  // (the counts are exact all the same: use them, grow after the merge)
          want_cap = std::min<uint64_t>(cap_limit, std::max<uint64_t>((uint64_t)cap * 2, r.taken * 4));
          need_rebuild = true;
        }
        // at the cap and more than half full: only an overflow rebuilds (not every merge)
        threshold = r.taken * 2 > cap ? cap : cap / 2;
      } else if (r.taken > threshold) {
        need_rebuild = true;
      }
      if (r.count <= 0) break;  // pair_freqs.is_empty()
      if (first && (uint64_t)r.count >= (1ull << 32))
        throw_error(CTOK_E_ARG, "a pair count of " + std::to_string(r.count) + " does not fit the reference's u32 counts");
      first = false;
      if ((uint64_t)r.count < min_frequency) break;
      const uint32_t a = (uint32_t)(r.key >> 32), b = (uint32_t)r.key;
      if (a >= sym_str.size() || b >= sym_str.size()) throw_error(CTOK_E_DEVICE, "pair search returned an unknown symbol");
      const std::string first_s = sym_str[a], second_s = sym_str[b];
      const std::string merged = first_s + second_s;
      const uint32_t vid = (uint32_t)vocab.size();
      vocab[merged] = vid;  // (a string already there gets the new id and the vocab does not grow)
      merges.emplace_back(first_s, second_s);
      const uint32_t nid = sym_of(merged);
      HIPT(hipEventRecord(ev[kEvMerge], s));
      HIPT(launch_merge(Wd, table(), a, b, nid, s));
      HIPT(hipEventRecord(ev[kEvMerge + 1], s));
      merge_pending = true;
    }
    HIPT(hipStreamSynchronize(s));
    if (merge_pending) add_ms(kEvMerge, &st.ms_merges);
    if (pairs_pending) add_ms(kEvPairs, &st.ms_pairs);
    st.merges = merges.size();
    st.table_capacity = cap;
    st.rebuilds = n_builds ? n_builds - 1 : 0;
  }

  std::vector<std::pair<std::string, uint32_t>> with_suffix(const std::unordered_map<std::string, uint32_t>& m) const {
    std::vector<std::pair<std::string, uint32_t>> v;
    v.reserve(m.size());
    for (const auto& kv : m) v.emplace_back(has_suffix ? kv.first + suffix : kv.first, kv.second);
    std::sort(v.begin(), v.end());  // (the reference's order is HashMap order; results do not depend on it)
    return v;
  }
};

extern "C" {

int ctok_bpe_trainer_create(const ctok_bpe_trainer_config* cfg, ctok_bpe_trainer** out) {
  if (!cfg || !out) return ctok_host::run_guarded([] { throw_error(CTOK_E_ARG, "null argument"); });
  *out = nullptr;
  return ctok_host::run_guarded([&] {
    auto tr = std::make_unique<ctok_bpe_trainer>();
    tr->vocab_size = cfg->vocab_size;
    tr->min_frequency = cfg->min_frequency;
    tr->device = cfg->device;
    if (cfg->n_special && !cfg->special_off) throw_error(CTOK_E_ARG, "null special_off");
    if (cfg->n_special && cfg->special_off[cfg->n_special] && !cfg->special) throw_error(CTOK_E_ARG, "null special");
    for (uint64_t i = 0; i < cfg->n_special; i++)
      tr->specials.emplace_back(cfg->special + cfg->special_off[i], cfg->special_off[i + 1] - cfg->special_off[i]);
    if (cfg->end_of_word_suffix) {
      tr->has_suffix = true;
      tr->suffix = cfg->end_of_word_suffix;
    }
    if (cfg->continuing_subword_prefix) {
      tr->has_prefix = true;
      tr->prefix = cfg->continuing_subword_prefix;
    }
    *out = tr.release();
  });
}

void ctok_bpe_trainer_destroy(ctok_bpe_trainer* tr) { delete tr; }

int ctok_bpe_trainer_count(ctok_bpe_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    tr->count(utf8, off, n_texts);
  });
}

int ctok_bpe_trainer_train(ctok_bpe_trainer* tr, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    tr->count(utf8, off, n_texts);
    tr->train(tr->with_suffix(tr->counts));
  });
}

int ctok_bpe_trainer_train_words(ctok_bpe_trainer* tr, const uint8_t* words, const uint64_t* word_off,
                                 const uint32_t* freqs, uint64_t n_words) {
  return ctok_host::run_guarded([&] {
    if (!tr || (n_words && (!word_off || !freqs || (word_off[n_words] && !words)))) throw_error(CTOK_E_ARG, "null argument");
    std::unordered_map<std::string, uint32_t> m;
    for (uint64_t i = 0; i < n_words; i++) {
      uint32_t& c = m[std::string((const char*)words + word_off[i], word_off[i + 1] - word_off[i])];
      if ((uint64_t)c + freqs[i] > 0xFFFFFFFFull) throw_error(CTOK_E_ARG, "a word's frequencies add up past u32");
      c += freqs[i];
    }
    tr->train(tr->with_suffix(m));
  });
}

uint64_t ctok_bpe_trainer_vocab_size(const ctok_bpe_trainer* tr) { return tr ? tr->vocab.size() : 0; }
uint64_t ctok_bpe_trainer_num_merges(const ctok_bpe_trainer* tr) { return tr ? tr->merges.size() : 0; }

int ctok_bpe_trainer_result(ctok_bpe_trainer* tr, ctok_bpe_strings* vocab, const uint32_t** vocab_id,
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

int ctok_bpe_trainer_word_counts(ctok_bpe_trainer* tr, ctok_bpe_strings* words, const uint32_t** freqs) {
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

int ctok_bpe_trainer_stats(const ctok_bpe_trainer* tr, ctok_bpe_trainer_info* out) {
  return ctok_host::run_guarded([&] {
    if (!tr || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = tr->st;
  });
}

int ctok_bpe_trainer_symbols(ctok_bpe_trainer* tr, ctok_bpe_strings* symbols) {
  return ctok_host::run_guarded([&] {
    if (!tr || !symbols) throw_error(CTOK_E_ARG, "null argument");
    tr->v_syms.clear();
    for (const auto& x : tr->sym_str) tr->v_syms.add(x);
    tr->v_syms.view(symbols);
  });
}

int ctok_bpe_trainer_pair_counts(ctok_bpe_trainer* tr, const uint32_t** a, const uint32_t** b, const int64_t** count,
                                 uint64_t* n) {
  return ctok_host::run_guarded([&] {
    if (!tr || !a || !b || !count || !n) throw_error(CTOK_E_ARG, "null argument");
    tr->v_pa.clear();
    tr->v_pb.clear();
    tr->v_pc.clear();
    if (tr->cap) {
      HIPT(hipSetDevice(tr->device));
      std::vector<uint64_t> k(tr->cap);
      std::vector<int64_t> v(tr->cap);
      HIPT(hipMemcpyAsync(k.data(), tr->keys.p, (size_t)tr->cap * 8, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipMemcpyAsync(v.data(), tr->vals.p, (size_t)tr->cap * 8, hipMemcpyDeviceToHost, tr->s));
      HIPT(hipStreamSynchronize(tr->s));
      for (uint32_t i = 0; i < tr->cap; i++) {
        if (k[i] == kEmptyKey) continue;
        tr->v_pa.push_back((uint32_t)(k[i] >> 32));
        tr->v_pb.push_back((uint32_t)k[i]);
        tr->v_pc.push_back(v[i]);
      }
    }
    *a = tr->v_pa.data();
    *b = tr->v_pb.data();
    *count = tr->v_pc.data();
    *n = tr->v_pa.size();
  });
}

}  // extern "C"
