// Internals of the host runtime shared by its translation units: error plumbing, the tokenizer
// object, the per-device state and the few functions that cross files.  Not part of the C ABI
// (hidden visibility: libctok.so exports the C functions of include/ctok.h only).
//   bpe_model.cpp    tokenizer.json's model as a BpeModel (HIP-free, table_compile.h)
//   table_compile.cpp  the BpeModel into the device tables, CompiledTables (HIP-free, table_compile.h)
//   ctok_load.cpp    the rest of the tokenizer.json loader, the getters that read only struct ctok
//   ctok_encode.cpp  device state (table upload), encode_device and the NFC splice
//   ctok_host.cpp    decode, host-buffer pipeline, padded encode, offsets, pretokenize, C ABI
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ctok.h"
#include "ctok_internal.h"
#include "host_common.h"
#include "json.hpp"
#include "table_compile.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {
using namespace ctok_dev;

// ----------------------------------------------------------------------------- errors
extern thread_local std::string g_err;  // ctok_last_error's message (ctok_host.cpp)

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// (CtokError and throw_err: table_compile.h)
#define HIPTRY(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) throw_err(CTOK_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// f's CtokError (or other exception) as the C ABI's return code and ctok_last_error message
int run(const std::function<void()>& f);

// A worker thread whose exception the parent rethrows: join() waits for it (a no-op for a thread
// never started), then rethrows what f threw.  The destructor joins without rethrowing.
class CatchThread {
 public:
  CatchThread() = default;
  template <class F>
  explicit CatchThread(F f) : th_([this, f] {
    try { f(); } catch (...) { ex_ = std::current_exception(); }
  }) {}
  CatchThread(const CatchThread&) = delete;
  ~CatchThread() { if (th_.joinable()) th_.join(); }
  template <class F>
  void start(F f) {
    th_ = std::thread([this, f] {
      try { f(); } catch (...) { ex_ = std::current_exception(); }
    });
  }
  void join() {
    if (th_.joinable()) th_.join();
    if (ex_) std::rethrow_exception(std::exchange(ex_, nullptr));
  }

 private:
  std::exception_ptr ex_;
  std::thread th_;
};

// ----------------------------------------------------------------------------- device state

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  void ensure(size_t n) {
    if (n <= cap && p) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    size_t want = std::max<size_t>(n + n / 16, 1024);  // (grow-only; a little slack for the next call)
    HIPTRY(hipMalloc((void**)&p, want * sizeof(T)));
    cap = want;
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
};

// Pinned (page-locked) host buffer: the landing side of the 16-bit id copies.
template <typename T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  void ensure(size_t n) {
    if (n <= cap && p) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    size_t want = std::max<size_t>(n + n / 8, 1024);
    HIPTRY(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
    cap = want;
  }
  ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// Double-buffered host-buffer pipeline of one device (ctok_encode_batch): chunk c's text is
// copied from the caller's buffer to d_in[c & 1] on the up stream while chunk c - 1 is encoded;
// its ids come back from d_ids[c & 1] into the caller's buffer while chunk c + 1 is encoded.
struct HostPipe {
  hipStream_t up = nullptr, down = nullptr;  // H2D and D2H copy streams (both directions at once)
  hipEvent_t ev_h2d[2] = {}, ev_enc[2] = {}, ev_d2h[2] = {};
  hipEvent_t ev_t[4] = {};  // timing of the first chunk's H2D and the last chunk's D2H
  DevBuf<uint16_t> d_ids16[2];    // 16-bit wire format (ids16 tokenizers): ids, and tok_off as u32
  DevBuf<uint32_t> d_toff32[2];
  PinBuf<uint16_t> pin_ids16[2];
  PinBuf<uint32_t> pin_toff32[2];
  DevBuf<uint8_t> d_in[2];
  DevBuf<uint64_t> d_off[2], d_tokoff[2];
  DevBuf<uint32_t> d_ids[2];
};

// Timing events of an encode call (DeviceState::ev), recorded by the kernels' own dispatches (Lx)
enum Ev {
  kEvStart,        // k_clear's start (a marker when normalising work precedes it)
  kEvSegmentEnd,   // k_segment's end
  kEvShortEnd,     // k_bpe_short's end
  kEvScanStart,    // the tile scan's start
  kEvUnused4,
  kEvDroppedStart, // the dropped-byte pass's start
  kEvTokoffEnd,    // k_tokoff's end
  kEvTilefirstEnd, // k_tilefirst's end
  kEvMidStart,     // the 17..32 B pass
  kEvC3End,        // the 33..64 B pass's end (register or sparse)
  kEvMidEnd,
  kEvSpliceEnd,    // a marker after the NFC splice
  kEvCount
};

// The pinned host words (DeviceState::host, 4096 bytes), as u64 word offsets
constexpr size_t kPinBytes = 4096;
constexpr size_t kPinNtok = 0;      // the token count (k_tokoff writes host_res[0], then the counters from [1])
constexpr size_t kPinFinal = 1;     // the final counters (k_tokoff, or copied): kNumCounters u32
constexpr size_t kPinReport = 64;   // the report (k_report / k_bpe_short): kNumCounters u32, then the sequence number
constexpr size_t kPinLongTot = 96;  // the long pieces' totals: ids, global-memory state words (2 u32)
constexpr size_t kPinSplice = 100;  // nfc_splice: sub-batch bytes, flagged docs (2 u64)
constexpr size_t kPinScratch = 102; // any other small readback between syncs (3 u64): NFC doc count,
                                    // normalised size, the decode and pad counters, the window total
static_assert(kPinFinal == kPinNtok + 1, "k_tokoff writes the counters right after the token count");
static_assert(kPinFinal * 8 + kNumCounters * 4 <= kPinReport * 8, "final counters run into the report");
static_assert(kPinReport * 8 + (kNumCounters + 1) * 4 <= kPinLongTot * 8, "report runs into the long totals");
static_assert(kPinLongTot * 8 + 2 * 4 <= kPinSplice * 8, "long totals run into the splice words");
static_assert(kPinSplice + 2 <= kPinScratch, "splice words run into the scratch slot");
static_assert((kPinScratch + 3) * 8 <= kPinBytes, "pinned words outgrow their block");

struct DeviceState {
  int device = -1;
  uint32_t n_cus = 1;
  std::recursive_mutex mu;  // serialises calls on this device; recursive: ctok_encode_padded holds it
                            // across its nested ctok_encode_padded_device call
  hipStream_t stream = nullptr;
  hipEvent_t ev[kEvCount] = {};
  hipEvent_t ev_sync = nullptr;   // spin-waited completion marker (no blocking-wait wakeup latency)
  hipStream_t side = nullptr;     // long-piece pass, overlapped with the short merge passes
  hipEvent_t ev_tot = nullptr;    // the long pieces' totals are in the host words
  hipEvent_t ev_join = nullptr;   // the side stream's long tiers are done
  uint32_t seq = 0;               // encode calls (attempts) on this device: Work::seq
  uint64_t* host = nullptr;       // pinned host words for small device->host readbacks
  uint64_t* host_dev = nullptr;   // the same words as a device pointer (k_tokoff writes the results there)
  // tables
  DevBuf<uint64_t> merge_tab, lds_image, lds16_image, merge16;
  DevBuf<uint32_t> pair0;
  DevBuf<uint32_t> piece_tab;
  DevBuf<uint32_t> rank_newid, eager, wmeta;
  DevBuf<int32_t> byte2id;
  DevBuf<uint8_t> cls_s1, cls_s2, nfc_s1, alnum, at_bytes, at_flags, cls_bmp;
  DevBuf<uint16_t> nfc_s2, decomp_off;
  DevBuf<uint32_t> decomp_cp, decomp_data, comp_val, at_off, at_id;
  DevBuf<uint64_t> comp_key;
  Tables t{};
  // workspace
  DevBuf<uint32_t> tfirst, pbits, tile_np, tile_tok, tile_doc, tcls, list0, list1, list2, list3, tcnt, scratch, counters;
  DevBuf<uint16_t> prec;  // piece records (u16, or pairs of them as u32)
  DevBuf<uint32_t> mrec, pdoc;
  DevBuf<uint32_t> lids, lw, long_pos, lw_pos, lwn, rend, cps;
  DevBuf<uint64_t> tregion;
  DevBuf<uint64_t> stamps;  // diagnostic builds (CTOK_SEG_STAMPS) with CTOK_STAMPS=1
  DevBuf<uint64_t> wgrec;   // diagnostic: CTOK_WGREC=1
  DevBuf<uint16_t> wpref;
  DevBuf<uint32_t> long_cnt, long_ord, long_hist, c3q, c3pre;
  DevBuf<uint64_t> long_list, mid_list, scan_tmp, scan_tmp2;
  DevBuf<uint32_t> doc_flag, ncp;
  // NFC splice (nfc_splice): flagged-doc ranks / sub-batch positions, the speculative pass's
  // output, the sub-batch and its output
  DevBuf<uint32_t> spl_rank, spl_ids, sub_ids;
  DevBuf<uint64_t> spl_pos, spl_toff, sub_off, sub_toff;
  DevBuf<uint8_t> sub_text;
  DevBuf<uint32_t> nfc_bits;  // k_segment's NFC word flags (speculative passes)
  DevBuf<uint64_t> norm_off;
  DevBuf<uint8_t> norm_text;
  bool last_norm = false;  // the last encode ran on norm_text / norm_off (last_B bytes)
  uint64_t last_B = 0;
  int last_rec16 = -1, last_wire16 = -1;  // diagnostics (ctok_get_table_props): the last encode's piece records / wire format
  // decode: tables (uploaded on first use), workspace, events
  bool dec_ready = false;
  DevBuf<uint32_t> dec_ent;
  DevBuf<uint8_t> dec_bytes;
  DevBuf<uint32_t> dec_chunk, dec_del, dec_tile, dec_cnt;
  DevBuf<uint8_t> dec_raw, dec_out;
  DevBuf<uint64_t> dec_rawoff, dec_outoff, dec_tokoff;
  DevBuf<uint32_t> dec_ids;
  hipEvent_t dev_ev[8] = {};
  // host-API staging
  std::unique_ptr<HostPipe> pipe;
  // padded encode: encoded ids, special ids, counters; host-API input / outputs
  DevBuf<uint32_t> pad_ids, pad_special, pad_ctr, pad_out[4];
  DevBuf<uint64_t> pad_tokoff, pad_rowlen, pad_in_off;
  // its overflowing windows (ctok_encode_windows): per-window records, per-row first windows
  DevBuf<uint64_t> win_len, win_start, win_rowwin;
  DevBuf<uint32_t> win_row, win_tokenless;
  DevBuf<uint8_t> pad_in_text;
  // bytes of device memory held for encode calls (the workspace, not the tokenizer tables)
  uint64_t workspace_bytes() const {
    uint64_t b = 0;
    auto add = [&](const auto& x) { b += (uint64_t)x.cap * sizeof(*x.p); };
    add(tfirst), add(pbits), add(tile_np), add(tile_tok), add(tile_doc), add(tcls), add(list0), add(list1);
    add(list2), add(list3), add(tcnt), add(prec), add(mrec), add(pdoc), add(scratch), add(counters), add(lids), add(lw), add(tregion), add(rend);
    add(wpref), add(long_cnt), add(long_ord), add(long_hist), add(long_pos), add(lw_pos), add(lwn), add(long_list), add(c3q), add(c3pre);
    add(mid_list), add(scan_tmp), add(scan_tmp2), add(cps);
    add(doc_flag), add(ncp), add(norm_off), add(norm_text);
    add(nfc_bits), add(spl_rank), add(spl_ids), add(sub_ids), add(spl_pos), add(spl_toff), add(sub_off), add(sub_toff), add(sub_text);
    return b;
  }
  ~DeviceState() {
    if (device >= 0) {
      (void)hipSetDevice(device);
      if (pipe) {
        for (int i = 0; i < 2; i++) {
          if (pipe->ev_h2d[i]) (void)hipEventDestroy(pipe->ev_h2d[i]);
          if (pipe->ev_enc[i]) (void)hipEventDestroy(pipe->ev_enc[i]);
          if (pipe->ev_d2h[i]) (void)hipEventDestroy(pipe->ev_d2h[i]);
        }
        for (auto& e : pipe->ev_t) if (e) (void)hipEventDestroy(e);
        if (pipe->up) (void)hipStreamDestroy(pipe->up);
        if (pipe->down) (void)hipStreamDestroy(pipe->down);
        pipe.reset();
      }
      for (auto& e : ev) if (e) (void)hipEventDestroy(e);
      for (auto& e : dev_ev) if (e) (void)hipEventDestroy(e);
      if (ev_sync) (void)hipEventDestroy(ev_sync);
      if (ev_join) (void)hipEventDestroy(ev_join);
      if (side) (void)hipStreamDestroy(side);
      if (ev_tot) (void)hipEventDestroy(ev_tot);
      if (host) (void)hipHostFree(host);
      if (stream) (void)hipStreamDestroy(stream);
    }
  }
};

}  // namespace ctok_rt

// ----------------------------------------------------------------------------- tokenizer

// (the compiled tables: its CompiledTables base, table_compile.h)
struct ctok : ctok_rt::CompiledTables {
  // host-side model (immutable after load)
  std::unordered_map<std::string, uint32_t> vocab;          // model.vocab
  std::unordered_map<uint32_t, std::string> id_to_token;    // Vocab::id_to_token
  std::vector<std::pair<std::string, uint32_t>> special;    // special added tokens
  bool nfc = true;
  bool add_prefix_space = false;
  // decode (src/huggingface/mod.rs:710-747): decoder kind, per-id decoded bytes
  int decoder = 1;                  // 1 ByteLevel, 0 raw concatenation (unknown decoder type), -1 unsupported
  std::string decoder_name;         // for the unsupported message
  std::vector<uint32_t> dec_ent;    // 2 u32 per id: byte offset, length | kDecNonAscii | kDecSpecial
  std::vector<uint8_t> dec_bytes;   // each id's bytes, 4-byte aligned, + 8 bytes of padding
  // post-processor, compiled to the items of PostProcessor::process(ids, None)
  // (src/postprocessors.rs:34-55): kPadItemA = the row's ids, else one special id
  bool has_pp = false;
  std::vector<uint32_t> pp_items;
  int pp_kind = 0;                   // 1 TemplateProcessing, 2 RobertaProcessing, 3 BertProcessing
  std::string pp_single, pp_pair;    // template strings (num_special_tokens_to_add)
  bool pp_has_pair = false;
  uint64_t model_max_length = 512;  // from_file / from_str: src/huggingface/mod.rs:243-245
  // per device
  std::mutex dev_mu;
  std::map<int, std::unique_ptr<ctok_rt::DeviceState>> devs;
  // (out of line, ctok_encode.cpp: destroying devs frees device memory, and the loader makes no HIP call)
  __attribute__((visibility("hidden"))) ctok();
  __attribute__((visibility("hidden"))) ~ctok();
};

namespace ctok_rt __attribute__((visibility("hidden"))) {

// ---- ctok_load.cpp
std::string encode_utf8(const std::vector<uint32_t>& cps, size_t a, size_t b);
bool is_white_space(uint32_t c);
void load(ctok* t, const char* buf, size_t len);
void load_root(ctok* t, const ctj::Value& root, const TableOptions& opt, LoadTimer& timer);

// ---- ctok_encode.cpp
double now_ms();
DeviceState* device_state(ctok* t, int device);
void spin_sync(DeviceState* ds, hipStream_t s);
// the pinned host words from u64 word `word` on (kPin*), read as T after a sync or a poll
template <class T>
volatile T* pinned(DeviceState* ds, size_t word) {
  return (volatile T*)(ds->host + word);
}

template <typename T>
void upload(DevBuf<T>& b, const T* src, size_t n, hipStream_t s) {
  b.ensure(n ? n : 1);
  if (n) HIPTRY(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
}

// What an encode call produces besides the piece starts, the normalised text and the tile state
enum class EncodeMode {
  Ids,          // ids and tok_off
  SegmentOnly,  // pre-tokenization only (the trainer's word counting): pbits of the text
  KeepFirst,    // ids, and k_emit leaves every piece's first id within its tile in tcnt (offsets)
};

// One encode_device call on device-resident buffers
struct EncodeCall {
  const uint8_t* text = nullptr;    // 16-byte aligned (a caller's pointer: checked at the C entry), 16 readable bytes past n_bytes, their content ignored
  const uint64_t* doc_off = nullptr;  // [n_docs + 1]
  uint64_t n_docs = 0, n_bytes = 0;
  uint32_t* ids = nullptr;          // output (null with SegmentOnly)
  uint64_t ids_cap = 0;
  uint64_t* tok_off = nullptr;      // [n_docs + 1] output
  hipStream_t stream = nullptr;
  bool timing = false;              // fill the ms_* fields of stats
  ctok_stats* stats = nullptr;
  // false: encode_to_encoding's words go straight to BpeTokenizer::encode, with no added-token
  // split (src/huggingface/mod.rs:395-420)
  bool split_added = true;
  EncodeMode mode = EncodeMode::Ids;
  bool all_nfc = false;  // every doc is normalised, unchecked (nfc_splice's sub-batch of flagged docs)
};
// The pipeline on device-resident buffers.  Returns the token count.
uint64_t encode_device(ctok* t, DeviceState* ds, const EncodeCall& call);

}  // namespace ctok_rt
