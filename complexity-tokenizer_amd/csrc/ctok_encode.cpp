// The encode side of the host runtime: per-device state (table upload and the filling of Tables)
// and the stream-ordered encode pipeline on device-resident buffers, encode_device, with the NFC
// splice.  The call's numeric decisions are in call_plan.h, its environment variables in knobs.h.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "call_plan.h"
#include "gen/unicode_data.h"
#include "host_internal.h"
#include "knobs.h"

ctok::ctok() = default;
ctok::~ctok() = default;

namespace ctok_rt __attribute__((visibility("hidden"))) {

// Tables::cp_fast: every code point of cp_range_class's ranges has the class it gives and no NFC
// flag in the generated tables (gen/unicode_data.h), so k_segment may skip their lookups.
bool cp_fast_ok() {
  static const bool ok = [] {
    if (process_knobs().no_cp_ranges) return false;
    for (uint32_t cp = 0x3000; cp < 0x1F700; cp++) {
      const int rc = cp_range_class(cp);
      if (rc < 0) continue;
      const int cl = (ct_cls_stage2[ct_cls_stage1[cp >> 8] * 64 + ((cp & 255) >> 2)] >> ((cp & 3) * 2)) & 3;
      if (cl != rc || ct_nfc_stage2[ct_nfc_stage1[cp >> 8] * 256 + (cp & 255)] != 0) return false;
    }
    return true;
  }();
  return ok;
}

DeviceState* device_state(ctok* t, int device) {
  std::lock_guard<std::mutex> lk(t->dev_mu);
  auto it = t->devs.find(device);
  if (it != t->devs.end()) return it->second.get();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw_err(CTOK_E_DEVICE, "no HIP device visible (the encode path has no CPU fallback)");
  if (device < 0 || device >= n) throw_err(CTOK_E_ARG, "device ordinal out of range");
  HIPTRY(hipSetDevice(device));
  auto ds = std::make_unique<DeviceState>();
  ds->device = device;
  HIPTRY(hipStreamCreateWithFlags(&ds->stream, hipStreamNonBlocking));
  {
    int cus = 0;
    HIPTRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    ds->n_cus = cus > 0 ? (uint32_t)cus : 1u;
  }
  for (auto& e : ds->ev) HIPTRY(hipEventCreate(&e));
  for (auto& e : ds->dev_ev) HIPTRY(hipEventCreate(&e));
  HIPTRY(hipEventCreateWithFlags(&ds->ev_sync, hipEventDisableTiming));
  HIPTRY(hipEventCreateWithFlags(&ds->ev_join, hipEventDisableTiming));
  HIPTRY(hipStreamCreateWithFlags(&ds->side, hipStreamNonBlocking));
  HIPTRY(hipEventCreateWithFlags(&ds->ev_tot, hipEventDisableTiming));
  // (coherent: the host polls words k_report writes while the call runs -- Work::report)
  HIPTRY(hipHostMalloc((void**)&ds->host, kPinBytes, hipHostMallocCoherent));
  HIPTRY(hipHostGetDevicePointer((void**)&ds->host_dev, ds->host, 0));
  hipStream_t s = ds->stream;
  upload(ds->merge_tab, t->merge_tab.data(), t->merge_tab.size(), s);
  upload(ds->lds_image, t->lds_image.data(), t->lds_image.size(), s);
  if (t->narrow) {
    upload(ds->lds16_image, t->lds16_image.data(), t->lds16_image.size(), s);
    upload(ds->merge16, t->merge16.data(), t->merge16.size(), s);
  }
  upload(ds->pair0, t->pair0.data(), t->pair0.size(), s);
  upload(ds->rank_newid, t->rank_newid.data(), t->rank_newid.size(), s);
  upload(ds->eager, t->eager_bits.data(), t->eager_bits.size(), s);
  if (t->window) upload(ds->wmeta, t->wmeta.data(), t->wmeta.size(), s);
  upload(ds->piece_tab, t->piece_tab.data(), t->piece_tab.size(), s);
  upload(ds->byte2id, t->byte2id, 256, s);
  upload(ds->cls_s1, ct_cls_stage1, sizeof(ct_cls_stage1), s);
  upload(ds->cls_s2, ct_cls_stage2, sizeof(ct_cls_stage2), s);
  upload(ds->nfc_s1, ct_nfc_stage1, sizeof(ct_nfc_stage1), s);
  upload(ds->nfc_s2, ct_nfc_stage2, sizeof(ct_nfc_stage2) / 2, s);
  {  // the BMP's classes and NFC flags as one direct table: a nibble per code point
    static const std::vector<uint8_t> bmp = [] {
      std::vector<uint8_t> b(32768, 0);
      for (uint32_t cp = 0; cp < 0x10000; cp++) {
        const uint32_t cl = (ct_cls_stage2[ct_cls_stage1[cp >> 8] * 64 + ((cp & 255) >> 2)] >> ((cp & 3) * 2)) & 3;
        const uint32_t nf = ct_nfc_stage2[ct_nfc_stage1[cp >> 8] * 256 + (cp & 255)] != 0 ? 4u : 0u;
        b[cp >> 1] |= (uint8_t)((cl | nf) << ((cp & 1) * 4));
      }
      return b;
    }();
    upload(ds->cls_bmp, bmp.data(), bmp.size(), s);
  }
  upload(ds->decomp_cp, ct_decomp_cp, CT_DECOMP_N, s);
  upload(ds->decomp_off, ct_decomp_off, CT_DECOMP_N + 1, s);
  upload(ds->decomp_data, ct_decomp_data, CT_DECOMP_DATA_N, s);
  upload(ds->comp_key, (const uint64_t*)ct_comp_key, CT_COMP_N, s);
  upload(ds->comp_val, ct_comp_val, CT_COMP_N, s);
  upload(ds->alnum, ct_bytemap_alnum, 256, s);
  upload(ds->at_bytes, (const uint8_t*)t->at_bytes.data(), t->at_bytes.size(), s);
  upload(ds->at_off, t->at_off.data(), t->at_off.size(), s);
  upload(ds->at_id, t->at_id.data(), t->at_id.size(), s);
  upload(ds->at_flags, t->at_flags.data(), t->at_flags.size(), s);
  HIPTRY(hipStreamSynchronize(s));
  Tables& tb = ds->t;
  tb.merge_tab = ds->merge_tab.p;
  tb.merge_mask = t->merge_mask;
  tb.lds_image = (const uint4*)ds->lds_image.p;
  tb.pair0 = ds->pair0.p;
  tb.lds16_image = (const uint4*)ds->lds16_image.p;
  tb.merge16 = ds->merge16.p;
  tb.merge16_mask = t->merge16_mask;
  tb.piece_tab = (const uint4*)ds->piece_tab.p;
  tb.piece_mask = t->piece_mask;
  tb.rank_newid = ds->rank_newid.p;
  tb.eager = ds->eager.p;
  tb.wmeta = ds->wmeta.p;
  tb.window = t->window ? 1 : 0;
  tb.n_ranks = (uint32_t)t->rank_newid.size();
  tb.byte2id = ds->byte2id.p;
  tb.cls_s1 = ds->cls_s1.p;
  tb.cls_s2 = ds->cls_s2.p;
  tb.nfc_s1 = ds->nfc_s1.p;
  tb.nfc_s2 = ds->nfc_s2.p;
  tb.cls_bmp = ds->cls_bmp.p;
  tb.cp_fast = cp_fast_ok() ? 1u : 0u;
  tb.decomp_cp = ds->decomp_cp.p;
  tb.decomp_off = ds->decomp_off.p;
  tb.decomp_data = ds->decomp_data.p;
  tb.n_decomp = CT_DECOMP_N;
  tb.comp_key = ds->comp_key.p;
  tb.comp_val = ds->comp_val.p;
  tb.n_comp = CT_COMP_N;
  tb.bytemap_alnum = ds->alnum.p;
  tb.at_bytes = ds->at_bytes.p;
  tb.at_off = ds->at_off.p;
  tb.at_id = ds->at_id.p;
  tb.at_flags = ds->at_flags.p;
  tb.n_at = (uint32_t)t->at_id.size();
  const UploadKnobs knobs;
  tb.proper = (t->proper && !knobs.force_improper) ? 1 : 0;
  tb.compact = t->compact ? 1 : 0;
  tb.narrow = (t->narrow && !knobs.force_wide_slots) ? 1 : 0;
  // CTOK_SHORT_PACKED=0: the 16 + 16 register tier on every table (A/B arm; the tests run both)
  tb.short_packed = (tb.narrow && t->short_packed && knobs.short_packed != 0) ? 1 : 0;
  {  // CTOK_MID_PACKED: the 17..32 B pass of tables with the property (Tables::mid_packed; A/B arms, the
     // tests run all three).  The third pass of k_bpe_short belongs to its packed instance: with
     // CTOK_SHORT_PACKED=0, 2 is 1.
    const int want = knobs.mid_packed;
    uint32_t v = (tb.narrow && tb.compact && t->short_packed && want > 0) ? (want >= 2 ? 2u : 1u) : 0u;
    if (v == 2 && !tb.short_packed) v = 1;
    tb.mid_packed = v;
  }
  tb.all_bytes = std::all_of(t->byte2id, t->byte2id + 256, [](int32_t v) { return v >= 0; }) ? 1 : 0;
  tb.dbg = knobs.dbg_mode;
  DeviceState* r = ds.get();
  t->devs[device] = std::move(ds);
  return r;
}

#define STEP(name, x)                                                                    \
  do {                                                                                   \
    HIPTRY(x);                                                                           \
    if (process_knobs().debug_sync) {                                                    \
      fprintf(stderr, "[ctok] %s launched\n", name);                                     \
      HIPTRY(hipStreamSynchronize(s));                                                   \
      fprintf(stderr, "[ctok] %s done\n", name);                                         \
    }                                                                                    \
  } while (0)

// Wait for all work on s by spinning on an event: a blocking stream synchronise can add
// hundreds of microseconds of wake-up latency per call on this path's few sync points.
// (idle: called between polls -- the timed calls read their event pairs there, see Laps)
template <class Idle>
void spin_sync(DeviceState* ds, hipStream_t s, Idle idle) {
  HIPTRY(hipEventRecord(ds->ev_sync, s));
  for (;;) {
    hipError_t e = hipEventQuery(ds->ev_sync);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) throw_err(CTOK_E_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(e));
    idle();
  }
}
void spin_sync(DeviceState* ds, hipStream_t s) {
  spin_sync(ds, s, [] {});
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The elapsed times of a timed call's event pairs, each read as soon as its later event has
// completed, while the host waits for the rest of the call: a read costs a few microseconds, and
// the ten of an encode call, read after its final wait, added ~40 us to every timed call
// (C4S8 1.20 -> 1.16 ms untimed, profiles/r06).
struct Laps {
  struct Lap {
    hipEvent_t a, b;
    double v;
    bool done;
  };
  Lap l[12];
  int n = 0;
  // the pairs of an encode call (add_laps; -1: not timed)
  int pretok = -1, segment = -1, lo = -1, mid = -1, c3 = -1, to_short = -1, to_mid = -1, to_c3 = -1, to_tail = -1,
      emit = -1, device = -1;
  int add(hipEvent_t a, hipEvent_t b) {
    l[n] = {a, b, 0.0, false};
    return n++;
  }
  void read(Lap& p) {
    float v = 0;
    HIPTRY(hipEventElapsedTime(&v, p.a, p.b));
    p.v = v;
    p.done = true;
  }
  void poll() {  // reads the first pair whose events have both completed, if any
    for (int k = 0; k < n; k++) {
      if (l[k].done) continue;
      // (both: the events can be on two streams, the "later" one done first)
      if (!done(l[k].b) || !done(l[k].a)) continue;
      read(l[k]);
      return;
    }
  }
  static bool done(hipEvent_t ev) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipErrorNotReady) return false;
    if (e != hipSuccess) throw_err(CTOK_E_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(e));
    return true;
  }
  void finish() {
    for (int k = 0; k < n; k++)
      if (!l[k].done) read(l[k]);
  }
  double ms(int k) const { return k < 0 ? 0.0 : l[k].v; }
};

// Waits for k_report's report of this call (Work::report: the counters, then the sequence number);
// a device error, or the stream running dry without it, ends the wait
void wait_report(hipStream_t s, volatile uint32_t* rep, uint32_t seq) {
  for (uint32_t i = 1;; i++) {
    if (rep[kNumCounters] == seq) return;
    if ((i & 4095) == 0) {
      const hipError_t e = hipStreamQuery(s);
      if (e == hipSuccess && rep[kNumCounters] != seq) throw_err(CTOK_E_DEVICE, "k_report: the call's report never came");
      if (e != hipSuccess && e != hipErrorNotReady)
        throw_err(CTOK_E_DEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(e));
    }
  }
}

// ----------------------------------------------------------------------------- diagnostics
// (off the call's path: each prints to stderr when its variable is set)

// CTOK_HOSTPROF=1: host time at points of the call, printed at its end
enum HpMark { kHpEntry, kHpPrep, kHpSegLaunched, kHpShortLaunched, kHpReport, kHpAllLaunched, kHpSynced, kHpLaps, kHpEnd, kHpCount };
struct HostProf {
  bool on = process_knobs().hostprof;
  double t[kHpCount] = {};
  void mark(HpMark i) {
    if (on) t[i] = now_ms();
  }
  void print() const {
    if (!on) return;
    auto us = [&](HpMark i) { return (t[i] - t[kHpEntry]) * 1e3; };
    fprintf(stderr, "[ctok hostprof] us from entry: prep %.1f  clear..segment launched %.1f  short launched %.1f  report %.1f  "
            "all launched %.1f  synced %.1f  laps %.1f  end %.1f\n", us(kHpPrep), us(kHpSegLaunched), us(kHpShortLaunched),
            us(kHpReport), us(kHpAllLaunched), us(kHpSynced), us(kHpLaps), us(kHpEnd));
  }
};

// CTOK_WGREC=1 (dev_common.h WgRec), per kernel: workgroups, distinct CUs, start / end spread (us from the first start)
void print_wgrec(const uint64_t* d_wgrec) {
  std::vector<uint64_t> r(kWgRecWords);
  HIPTRY(hipMemcpy(r.data(), d_wgrec, kWgRecWords * 8, hipMemcpyDeviceToHost));
  uint64_t t0 = ~0ull;
  for (size_t i = 0; i < kWgRecWords; i += 4)
    if (r[i]) t0 = std::min(t0, r[i]);
  static const char* names[4] = {"k_bpe_short", "k_bpe_mid<2>", "k_bpe_mid<3>", "k_bpe_sparse"};
  for (int k = 0; k < 4; k++) {
    std::vector<uint64_t> cus;
    double s0 = 1e30, s1 = 0, e0 = 1e30, e1 = 0;
    int n = 0, busy = 0;
    for (int b = 0; b < 1024; b++) {
      const uint64_t* q = &r[((size_t)k * 1024 + b) * 4];
      if (!q[0] || !q[1]) continue;
      n++;
      busy += q[3] != 0;
      cus.push_back(q[2]);
      const double a = (q[0] - t0) / 100.0, e = (q[1] - t0) / 100.0;  // (100 MHz clock)
      s0 = std::min(s0, a), s1 = std::max(s1, a), e0 = std::min(e0, e), e1 = std::max(e1, e);
    }
    if (!n) continue;
    std::sort(cus.begin(), cus.end());
    const size_t ncu = std::unique(cus.begin(), cus.end()) - cus.begin();
    fprintf(stderr, "[ctok wgrec] %-13s wgs %4d (working %4d) on %3zu CUs  start %8.1f .. %8.1f  end %8.1f .. %8.1f us\n",
            names[k], n, busy, ncu, s0, s1, e0, e1);
  }
}

// CTOK_STAMPS=1 in a -DCTOK_SEG_STAMPS build: k_segment's mean cycles per phase over the tiles that stamped
void print_stamps(const uint64_t* d_stamps, size_t n_tiles) {
  std::vector<uint64_t> st8(n_tiles * 8);
  HIPTRY(hipMemcpy(st8.data(), d_stamps, st8.size() * 8, hipMemcpyDeviceToHost));
  double acc[6] = {0, 0, 0, 0, 0, 0}, np_sum = 0;
  uint64_t n = 0;
  for (size_t i = 0; i < n_tiles; i++) {
    const uint64_t* r = &st8[i * 8];
    if (!r[0] || !r[5]) continue;
    for (int k = 0; k < 5; k++) acc[k] += (double)(r[k + 1] - r[k]);
    acc[5] += (double)(r[5] - r[0]);
    np_sum += (double)r[6];
    n++;
  }
  if (n)
    fprintf(stderr, "[ctok stamps] k_segment cycles per tile (mean of %llu): loads %.0f  non-ascii %.0f  starts %.0f  "
            "routing %.0f  tail %.0f  total %.0f  pieces %.1f\n", (unsigned long long)n, acc[0] / n, acc[1] / n,
            acc[2] / n, acc[3] / n, acc[4] / n, acc[5] / n, np_sum / n);
}

// ----------------------------------------------------------------------------- NFC splice

// NFC splice: the speculative pass over the raw text finished but flagged a code point NFC may
// change (src/normalizers.rs:45-47 normalises every document).  Only the documents holding such
// code points (k_nfc_check's flags, a superset of those NFC changes) are gathered into a
// sub-batch, encoded normalised, and their ids replace the pass's in c.ids / c.tok_off; the
// others' ids are already right (NFC leaves them unchanged, and pieces never cross documents).
// Returns the token count; *n_flagged = the flagged documents.
uint64_t nfc_splice(ctok* t, DeviceState* ds, const EncodeCall& c, uint64_t ntok_main, uint64_t* n_flagged) {
  const uint64_t n_docs = c.n_docs;
  hipStream_t s = c.stream;
  ds->doc_flag.ensure(n_docs + 1);
  HIPTRY(launch_flag_docs(c.doc_off, n_docs, ds->nfc_bits.p, ds->doc_flag.p, s));
  // ranks of the flagged docs, their places in the sub-batch
  ds->spl_rank.ensure(n_docs + 1);
  ds->spl_pos.ensure(n_docs + 1);
  ds->scan_tmp.ensure(scan_tmp_elems(n_docs + 1) + 64);
  HIPTRY(scan_u32(ds->doc_flag.p, ds->spl_rank.p, n_docs, nullptr, (uint32_t*)ds->scan_tmp.p, ds->scan_tmp.cap * 2, s));
  HIPTRY(launch_flag_len(c.doc_off, ds->doc_flag.p, n_docs, ds->spl_pos.p, s));
  HIPTRY(scan_u64(ds->spl_pos.p, n_docs, ds->scan_tmp.p, ds->scan_tmp.cap, s));
  volatile uint64_t* h = pinned<uint64_t>(ds, kPinSplice);
  HIPTRY(hipMemcpyAsync((void*)h, ds->spl_pos.p + n_docs, 8, hipMemcpyDeviceToHost, s));
  HIPTRY(hipMemcpyAsync((void*)(h + 1), ds->spl_rank.p + n_docs, 4, hipMemcpyDeviceToHost, s));
  spin_sync(ds, s);
  const uint64_t SB = h[0], F = (uint32_t)h[1];
  *n_flagged = F;
  if (F == 0) return ntok_main;
  // the flagged docs' raw text as a sub-batch (16-byte aligned, zero padded)
  ds->sub_text.ensure(SB + 16);
  ds->sub_off.ensure(F + 1);
  HIPTRY(launch_gather_flagged(c.text, c.doc_off, ds->spl_rank.p, ds->spl_pos.p, n_docs, ds->sub_text.p, ds->sub_off.p, s));
  HIPTRY(hipMemcpyAsync(ds->sub_off.p + F, ds->spl_pos.p + n_docs, 8, hipMemcpyDeviceToDevice, s));
  HIPTRY(hipMemsetAsync(ds->sub_text.p + SB, 0, 16, s));
  // the pass's output, read by the splice
  ds->spl_ids.ensure(ntok_main + 1);
  ds->spl_toff.ensure(n_docs + 1);
  if (ntok_main) HIPTRY(hipMemcpyAsync(ds->spl_ids.p, c.ids, ntok_main * 4, hipMemcpyDeviceToDevice, s));
  HIPTRY(hipMemcpyAsync(ds->spl_toff.p, c.tok_off, (n_docs + 1) * 8, hipMemcpyDeviceToDevice, s));
  // the sub-batch: normalise + encode (no speculation and no check: every doc in it is flagged),
  // with the outer call's added-token rule
  ds->sub_ids.ensure(ctok_ids_bound(t, SB, F));
  ds->sub_toff.ensure(F + 1);
  EncodeCall sub;
  sub.text = ds->sub_text.p, sub.doc_off = ds->sub_off.p, sub.n_docs = F, sub.n_bytes = SB;
  sub.ids = ds->sub_ids.p, sub.ids_cap = ds->sub_ids.cap, sub.tok_off = ds->sub_toff.p;
  sub.stream = s;
  sub.split_added = c.split_added;
  sub.all_nfc = true;
  encode_device(t, ds, sub);
  ds->scan_tmp.ensure(scan_tmp_elems(n_docs + 1) + 64);
  HIPTRY(launch_splice(ds->spl_rank.p, ds->spl_toff.p, ds->spl_ids.p, ds->sub_toff.p, ds->sub_ids.p, n_docs, c.ids,
                       c.ids_cap, c.tok_off, ds->scan_tmp.p, ds->scan_tmp.cap, s));
  HIPTRY(hipMemcpyAsync((void*)h, c.tok_off + n_docs, 8, hipMemcpyDeviceToHost, s));
  spin_sync(ds, s);
  return h[0];
}

// ----------------------------------------------------------------------------- encode_device

// One encode_device call: what its attempts share
struct Enc {
  ctok* t;
  DeviceState* ds;
  const EncodeCall& c;
  Tables tb;  // the device's tables; n_at = 0 without the added-token split
  // a flagged pass is finished and only its flagged docs are encoded again (nfc_splice), except
  // where the whole batch's pass state is read afterwards (offsets, the trainer's pre-tokenizer)
  bool splice;
  CallKnobs knobs;
  HostProf hp;
};

// One run of the pipeline.  The call starts speculating on NFC where it can, with lean list
// capacities; an attempt's outcome can turn either off for the next.
struct Attempt {
  // NFC speculation: when NFC is the only normalisation, run the pipeline on the raw text and let
  // k_segment flag any code point that NFC might change (NFC_QC != Yes or a non-zero combining
  // class; ASCII never is).  Only a flagged batch pays for the check + normalise passes.
  bool speculate;
  bool safe;  // the safe list capacities (Capacities)
  // normalise
  bool ev0_marker = false;  // kEvStart is a marker before the normalising work, not k_clear's start
  bool ctr_zeroed = false;  // (else launch_docstart zeroes the counters, in the bitmap's clearing launch)
  bool norm = false;        // the pipeline runs on norm_text / norm_off
  const uint8_t* text = nullptr;
  const uint64_t* off = nullptr;
  uint64_t B = 0;           // bytes of text
  uint64_t nfc_docs = 0;
  // workspace
  Capacities cap{};
  Work w{};
  // passes
  bool tm = false;  // the launches record timing events
  PassPlan plan{};
  Laps laps;
  // results
  uint64_t ntok = 0;
  uint32_t cnt[kNumCounters] = {};  // the final counters
};

// The text the pipeline runs on: the call's, or norm_text / norm_off after the NFC check (without
// speculation) and k_norm (NFC and / or the prefix space).
void normalise(Enc& e, Attempt& a) {
  ctok* t = e.t;
  DeviceState* ds = e.ds;
  const EncodeCall& c = e.c;
  hipStream_t s = c.stream;
  const uint64_t n_docs = c.n_docs;
  const bool nfc = t->nfc && c.n_bytes;
  a.ev0_marker = c.timing && (t->add_prefix_space || (nfc && (c.all_nfc || !a.speculate)));
  if (a.ev0_marker) HIPTRY(hipEventRecord(ds->ev[kEvStart], s));
  ds->counters.ensure(kCounterWords);
  a.text = c.text, a.off = c.doc_off, a.B = c.n_bytes;
  a.norm = t->add_prefix_space;
  if (nfc && c.all_nfc) {
    ds->doc_flag.ensure(n_docs + 1);
    HIPTRY(hipMemsetD32Async((hipDeviceptr_t)ds->doc_flag.p, 1, n_docs + 1, s));
    a.nfc_docs = n_docs;
    a.norm = true;
  } else if (nfc && !a.speculate) {
    ds->doc_flag.ensure(n_docs + 1);
    HIPTRY(hipMemsetAsync(ds->doc_flag.p, 0, (n_docs + 1) * 4, s));
    HIPTRY(hipMemsetAsync(ds->counters.p, 0, kCounterWords * 4, s));
    a.ctr_zeroed = true;
    STEP("nfc_check", launch_nfc_check(c.text, c.n_bytes, c.doc_off, (uint32_t)n_docs, e.tb, ds->doc_flag.p,
                                       ds->counters.p + kCtrNfcDocs, s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, ds->counters.p + kCtrNfcDocs, 4, hipMemcpyDeviceToHost, s));
    spin_sync(ds, s);
    a.nfc_docs = *pinned<uint32_t>(ds, kPinScratch);
    if (a.nfc_docs) a.norm = true;
  }
  if (a.norm) {
    const int do_nfc = t->nfc && a.nfc_docs;
    ds->doc_flag.ensure(n_docs + 1);
    if (!t->nfc) HIPTRY(hipMemsetAsync(ds->doc_flag.p, 0, (n_docs + 1) * 4, s));
    ds->ncp.ensure(n_docs + 1);
    ds->norm_off.ensure(n_docs + 2);
    ds->cps.ensure(4 * c.n_bytes + 64);
    STEP("norm0", launch_norm(c.text, c.doc_off, (uint32_t)n_docs, ds->doc_flag.p, t->add_prefix_space, do_nfc, e.tb,
                              ds->cps.p, ds->ncp.p, ds->norm_off.p, nullptr, 0, s));
    ds->scan_tmp.ensure(scan_tmp_elems(n_docs + 1) + 64);
    HIPTRY(scan_u64(ds->norm_off.p, n_docs, ds->scan_tmp.p, ds->scan_tmp.cap, s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, ds->norm_off.p + n_docs, 8, hipMemcpyDeviceToHost, s));
    spin_sync(ds, s);
    const uint64_t nb = *pinned<uint64_t>(ds, kPinScratch);
    if (nb >= 0xF0000000ull) throw_err(CTOK_E_ARG, "normalised batch exceeds 3.75 GiB; split the batch");
    // (16 readable bytes after the text, like every text buffer; k_norm writes exactly nb bytes and
    // what an earlier call left behind them is ignored -- include/ctok.h, tests/test_gpu_text_tail.py)
    ds->norm_text.ensure(nb + 16);
    STEP("norm1", launch_norm(c.text, c.doc_off, (uint32_t)n_docs, ds->doc_flag.p, t->add_prefix_space, do_nfc, e.tb,
                              ds->cps.p, ds->ncp.p, ds->norm_off.p, ds->norm_text.p, 1, s));
    a.text = ds->norm_text.p, a.off = ds->norm_off.p, a.B = nb;
  }
  ds->last_norm = a.norm;
  ds->last_B = a.B;
}

// b grown to n elements, and the Work field that points at it
template <class T, class P>
void bind(DevBuf<T>& b, size_t n, P*& field) {
  b.ensure(n);
  field = (P*)b.p;
}

// Work for the attempt's text: the workspace buffers grown to what plan_capacities says, each bound
// to its field.  (The long pieces' buffers are sized from the report and from launch_long_prep's
// totals: bind_long_prep, bind_long_ids.)
void size_workspace(Enc& e, Attempt& a) {
  DeviceState* ds = e.ds;
  const ProcessKnobs& pk = process_knobs();
  Work& w = a.w;
  w.text = a.text;
  w.n_bytes = (uint32_t)a.B;
  w.doc_off = a.off;
  w.n_docs = (uint32_t)e.c.n_docs;
  w.n_words = (uint32_t)((a.B + 31) / 32);
  w.n_tiles = (uint32_t)((a.B + kTile - 1) / kTile);
  w.n_cus = ds->n_cus;
  w.nfc_watch = a.speculate ? (e.splice ? 2u : 1u) : 0u;
  w.keep_first = e.c.mode == EncodeMode::KeepFirst ? 1u : 0u;
  w.short_wgs = e.knobs.short_wgs;
  w.chunk_sort = e.knobs.chunk_sort;
  const size_t nt = w.n_tiles;
  a.cap = plan_capacities(a.B, nt, a.safe, e.tb.n_at, pk.unit, e.knobs.c3_sparse);
  w.k0 = a.cap.k0;
  w.unit = a.cap.unit;
  w.long_cap = a.cap.long_cap;
  w.mid_cap = a.cap.mid_cap;
  w.c3_max = a.cap.c3_max;
  // piece records: u16 when every id a whole-piece probe can return is below 0xFFFF
  w.rec16 = (e.t->narrow && !pk.rec32) ? 1u : 0u;
  ds->last_rec16 = (int)w.rec16;

  if (w.nfc_watch == 2) bind(ds->nfc_bits, nfc_bits_words(a.B), w.nfc_bits);  // (zeroed by launch_docstart)
  bind(ds->tfirst, nt + 8, w.tfirst);
  bind(ds->pbits, w.n_words + 8, w.pbits);
  bind(ds->wpref, nt * 64 + 8, w.wpref);
  bind(ds->tile_np, nt + 8, w.tile_np);
  bind(ds->tile_tok, nt + 8, w.tile_tok);
  bind(ds->tile_doc, nt + 8, w.tile_doc);
  bind(ds->tcls, kNumClasses * nt + 8, w.tcls);
  bind(ds->list0, nt * w.k0 + 8, w.list0);
  bind(ds->rend, kNumClasses * nt + 8, w.rend);
  if (e.tb.n_at == 0) {
    ds->list1.ensure(nt * kCap1 + 8);
    ds->list2.ensure(nt * kCap2 + 8);
    ds->list3.ensure(nt * kCap3 + 8);
  }
  w.list1 = ds->list1.p, w.list2 = ds->list2.p, w.list3 = ds->list3.p;  // (unused with added tokens: list0 holds every piece)
  bind(ds->tcnt, nt * kTileSlots + 8, w.tcnt);
  bind(ds->prec, nt * kTileSlots * (w.rec16 ? 1 : 2) + 16, w.prec);
  bind(ds->mrec, nt * kTileSlots + 8, w.mrec);
  bind(ds->pdoc, nt * (kTileSlots / 32) + 8, w.pdoc);
  bind(ds->scratch, nt * kTileSlots + 8, w.scratch);  // per tile: the class regions of the register passes
  bind(ds->tregion, nt + 8, w.tregion);
  bind(ds->long_list, w.long_cap + 8, w.long_list);
  bind(ds->long_cnt, w.long_cap + 8, w.long_cnt);
  bind(ds->long_ord, w.long_cap + 8, w.long_ord);
  bind(ds->long_hist, kLhWords, w.long_hist);
  bind(ds->mid_list, w.mid_cap + 8, w.mid_list);
  bind(ds->scan_tmp, std::max(scan_tmp_elems(std::max<uint64_t>(nt + 1, e.c.n_docs + 1)), tile_scan_tmp_elems(nt)) + 64,
       w.scan_tmp);
  w.scan_tmp_cap = ds->scan_tmp.cap * 2;
  w.counters = ds->counters.p;  // (grown by normalise, which may zero them)
  if (w.c3_max) {
    bind(ds->c3q, w.c3_max + 8, w.c3q);
    bind(ds->c3pre, kC3Shards + 8, w.c3pre);
  }
  // the pinned host words the kernels write: the report, and k_tokoff's results (CTOK_COPY_RESULTS: copied instead)
  w.report = (uint32_t*)(ds->host_dev + kPinReport);
  w.host_res = pk.copy_results ? nullptr : ds->host_dev + kPinNtok;
  hipStream_t s = e.c.stream;
#ifdef CTOK_CHECK
  // (range-checking build: every merged record starts out of range, so one no pass wrote traps)
  HIPTRY(hipMemsetAsync(ds->mrec.p, 0xFF, (size_t)nt * kTileSlots * 4, s));
#endif
  if (pk.wgrec) {  // diagnostic: per-workgroup records of the merge passes (dev_common.h WgRec)
    bind(ds->wgrec, kWgRecWords, w.wgrec);
    HIPTRY(hipMemsetAsync(ds->wgrec.p, 0, kWgRecWords * 8, s));
  }
  if (pk.stamps && nt) {  // (k_segment writes them only in a -DCTOK_SEG_STAMPS build)
    bind(ds->stamps, nt * 8 + 8, w.stamps);
    HIPTRY(hipMemsetAsync(ds->stamps.p, 0, nt * 8 * 8, s));
  }
}
void bind_long_prep(DeviceState* ds, Work& w, uint32_t n_long) {
  bind(ds->long_pos, n_long + 8, w.long_pos);
  bind(ds->lw_pos, n_long + 8, w.lw_pos);
  ds->lwn.ensure(n_long + 8);
  ds->scan_tmp2.ensure(scan_tmp_elems(n_long + 1) + 64);
}
void bind_long_ids(DeviceState* ds, Work& w, uint32_t n_ids, uint32_t n_gmem_bytes) {
  bind(ds->lids, (uint64_t)n_ids + 64, w.lids);
  bind(ds->lw, 4 * (uint64_t)n_gmem_bytes + 64, w.lw);
}

// The launch options of a timed attempt: start event a, stop event b (-1: none)
Lx lx(const Enc& e, const Attempt& a, int start, int stop) {
  Lx x;
  if (a.tm && start >= 0) x.start = e.ds->ev[start];
  if (a.tm && stop >= 0) x.stop = e.ds->ev[stop];
  return x;
}

// Streams and ordering.  The main stream s runs k_clear, k_tilefirst, k_segment, k_bpe_short,
// whose first wave writes the report the host polls (k_segment's counters, the class-3 count
// among them, into pinned host words, then the call's sequence number; k_report does it when
// k_bpe_short does not run).  Having seen it, the host knows k_segment has completed, so it
// launches what reads k_segment's output on the side stream with no fork event: the 17..32 B
// pass when the call has no long pieces (its workgroups take the CUs k_bpe_short's free at its
// end, beside the 33..64 B pass -- register or sparse -- on the main stream), else the
// long-piece preparation and tiers; one join before the tail (dropped-byte pass, tile scan,
// k_emit, k_tokoff).  The round-5 flow forked the side stream with an event after k_segment
// (the counter copy and, in round 6's first build, the class-3 list there), and the sparse pass
// waited for the list's event: ~3 us per event marker on the main stream and ~10 us per
// cross-stream wait (tools/queue_gaps.hip, profiles/r06).  Any-order packets
// (hipExtAnyOrderLaunch) do not help here: one starts when the previous kernel's first
// workgroup retires, and k_bpe_short's persistent workgroups retire together at its end
// (tools/anyorder_check.hip).
// Timing (stats): events recorded by the kernels' own dispatches (Lx, enum Ev), no marker
// packets, and none on the launches the device waits for at the call's start (an event costs the
// host ~3 us per launch there; later launches run ahead of the device).

// k_clear, k_tilefirst, k_segment
void launch_pretok(Enc& e, Attempt& a) {
  hipStream_t s = e.c.stream;
  a.tm = e.c.timing && e.c.stats && a.w.n_tiles;  // (no tiles: no merge pass to time)
  e.hp.mark(kHpPrep);
  STEP("docstart", launch_docstart(a.w, s, !a.ctr_zeroed, lx(e, a, a.ev0_marker ? -1 : kEvStart, -1), lx(e, a, -1, kEvTilefirstEnd)));
  STEP("segment", launch_segment(a.w, e.tb, s, lx(e, a, -1, kEvSegmentEnd)));
}

// Pre-tokenization only: the attempt ends after k_segment (no list is read, so no overflow matters)
Outcome finish_segment_only(Enc& e, Attempt& a) {
  DeviceState* ds = e.ds;
  HIPTRY(hipMemcpyAsync(ds->host + kPinFinal, ds->counters.p, kNumCounters * 4, hipMemcpyDeviceToHost, e.c.stream));
  spin_sync(ds, e.c.stream);
  return a.speculate && pinned<uint32_t>(ds, kPinFinal)[kCtrNfcFlag] ? Outcome::RerunNormalised : Outcome::Done;
}

// k_bpe_short, then -- by the report's plan -- the other merge passes and the long pieces, on the
// main and the side stream, and the join
void launch_merges(Enc& e, Attempt& a) {
  DeviceState* ds = e.ds;
  const Tables& tb = e.tb;
  Work& w = a.w;
  hipStream_t s = e.c.stream;
  if (++ds->seq == 0) ds->seq = 1;
  w.seq = ds->seq;
  // (k_bpe_short's first wave writes the report; without it -- added tokens, no tiles -- k_report)
  e.hp.mark(kHpSegLaunched);
  if (tb.n_at != 0 || !w.n_tiles) STEP("report", launch_report(w, s));
  STEP("bpe_short", launch_bpe_class(w, tb, 0, s, lx(e, a, -1, kEvShortEnd)));
  e.hp.mark(kHpShortLaunched);
  volatile uint32_t* report = pinned<uint32_t>(ds, kPinReport);
  wait_report(s, report, w.seq);
  e.hp.mark(kHpReport);
  uint32_t rep[kNumCounters];
  for (int i = 0; i < kNumCounters; i++) rep[i] = report[i];
  const PassPlan& p = a.plan = plan_passes(tb, rep, a.cap, w.nfc_watch, e.knobs.overlap, e.knobs.mid512, w.n_tiles);
  w.mid_wide = p.mid_wide;
  // long pieces: their lengths, order and places first (side stream, before the host waits for
  // anything else: the long tiers after them are the side stream's critical path on C5 / C3);
  // lids / lw are sized from the totals read back below, once the merge passes are launched
  volatile uint32_t* tot = pinned<uint32_t>(ds, kPinLongTot);
  if (p.n_long) {
    bind_long_prep(ds, w, p.n_long);
    STEP("long_prep", launch_long_prep(w, tb, ds->side, p.n_long, ds->lwn.p, (uint32_t*)ds->scan_tmp2.p,
                                       ds->scan_tmp2.cap * 2));
    HIPTRY(hipMemcpyAsync((void*)tot, ds->long_pos.p + p.n_long, 4, hipMemcpyDeviceToHost, ds->side));
    HIPTRY(hipMemcpyAsync((void*)(tot + 1), ds->lw_pos.p + p.n_long, 4, hipMemcpyDeviceToHost, ds->side));
    HIPTRY(hipEventRecord(ds->ev_tot, ds->side));
  }
  // Without long pieces the side stream is idle: the 17..32 B pass goes there (CTOK_OVERLAP=0: on
  // the main stream after k_bpe_short), so its workgroups take the CUs k_bpe_short's free at its
  // end, beside the 33..64 B pass on the main stream (the classes' pieces, regions and records are
  // disjoint); no fork event -- the report orders it after k_segment --, one join before the tail
  if (!p.folded) STEP("bpe_mid", launch_bpe_class(w, tb, 2, p.mid_side ? ds->side : s, lx(e, a, kEvMidStart, kEvMidEnd)));
  // With the class folded the side stream is idle again: the 33..64 B pass -- register or sparse --
  // goes there and takes the CUs k_bpe_short's workgroups free as they end, instead of starting
  // after the last of them (C4: 0.05 ms, profiles/mid32_packed/ab_summary.txt; CTOK_OVERLAP=0: main)
  hipStream_t c3s = p.c3_side ? ds->side : s;
  if (p.c3_sparse) STEP("bpe_c3_sparse", launch_c3_sparse(w, tb, p.c3n, c3s, lx(e, a, -1, kEvC3End)));
  else STEP("bpe_c3", launch_bpe_class(w, tb, 4, c3s, lx(e, a, -1, kEvC3End)));
  if (p.n_long) {
    for (;;) {  // the long pieces' totals (launch_long_prep above)
      const hipError_t err = hipEventQuery(ds->ev_tot);
      if (err == hipSuccess) break;
      if (err != hipErrorNotReady) throw_err(CTOK_E_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(err));
    }
    const bool any_gmem = tot[1] != 0;  // a long piece for the global-memory tier (its state words reserved)
    bind_long_ids(ds, w, tot[0], tot[1]);
    STEP("bpe_long", launch_bpe_long(w, tb, ds->side, p.n_long, p.c3_long_side, any_gmem));
  }
  if (p.join) {
    HIPTRY(hipEventRecord(ds->ev_join, ds->side));
    HIPTRY(hipStreamWaitEvent(s, ds->ev_join, 0));
  }
}

// The pairs of events a timed attempt reports (fill_stats)
void add_laps(const Enc& e, Attempt& a, bool dropped_pass) {
  const hipEvent_t* ev = e.ds->ev;
  const PassPlan& p = a.plan;
  Laps& l = a.laps;
  const bool passes = e.tb.n_at == 0;  // (with added tokens one kernel merges every <= 32 B piece)
  l.pretok = l.add(ev[kEvStart], ev[kEvSegmentEnd]);
  l.segment = l.add(ev[kEvTilefirstEnd], ev[kEvSegmentEnd]);
  l.lo = l.add(ev[kEvSegmentEnd], ev[kEvShortEnd]);  // <= 16 B pass (from k_segment's end)
  // class 2; on the side stream its events span the wait for k_bpe_short's CUs, so the time it
  // adds after k_bpe_short's end is reported
  // (nothing when k_bpe_short took it: lo then contains the class)
  l.mid = !passes || p.folded ? -1 : l.add(ev[p.mid_side ? kEvShortEnd : kEvMidStart], ev[kEvMidEnd]);
  l.c3 = passes ? l.add(ev[kEvShortEnd], ev[kEvC3End]) : -1;  // class 3 (register or sparse pass; after k_bpe_short)
  l.to_short = l.add(ev[kEvSegmentEnd], ev[kEvShortEnd]);  // k_segment's end to the merge passes' ends
  l.to_mid = passes && !p.folded ? l.add(ev[kEvSegmentEnd], ev[kEvMidEnd]) : -1;
  l.to_c3 = passes ? l.add(ev[kEvSegmentEnd], ev[kEvC3End]) : -1;
  l.to_tail = l.add(ev[kEvSegmentEnd], ev[dropped_pass ? kEvDroppedStart : kEvScanStart]);  // ... to the tail's start
  l.emit = l.add(ev[kEvScanStart], ev[kEvTokoffEnd]);  // tile scan + emit
  l.device = l.add(ev[kEvStart], ev[kEvTokoffEnd]);
}

// The tail on the main stream: dropped-byte pass, tile scan, k_emit, k_tokoff
void launch_tail(Enc& e, Attempt& a) {
  DeviceState* ds = e.ds;
  const EncodeCall& c = e.c;
  const Work& w = a.w;
  hipStream_t s = c.stream;
  const bool dropped_pass = e.tb.n_at == 0 && !e.tb.all_bytes;
  STEP("bpe_dropped", launch_bpe_class(w, e.tb, 3, s, lx(e, a, kEvDroppedStart, -1)));
  // the token count and the counters: written by k_tokoff straight into the pinned host words
  // (two copy launches fewer at the end of every call), or copied
  const bool empty_docs = pinned<uint32_t>(ds, kPinReport)[kCtrEmptyDocs] != 0;
  STEP("emit", launch_emit(w, c.ids, c.ids_cap, c.tok_off, s, c.stats != nullptr, empty_docs, lx(e, a, kEvScanStart, -1),
                           lx(e, a, -1, kEvTokoffEnd)));
  if (!w.host_res) {
    HIPTRY(hipMemcpyAsync(ds->host + kPinNtok, c.tok_off + c.n_docs, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinFinal, ds->counters.p, kNumCounters * 4, hipMemcpyDeviceToHost, s));
  }
  if (a.tm) add_laps(e, a, dropped_pass);
  e.hp.mark(kHpAllLaunched);
}

// Waits for the attempt; its token count, final counters and event times
void read_results(Enc& e, Attempt& a) {
  DeviceState* ds = e.ds;
  spin_sync(ds, e.c.stream, [&] { a.laps.poll(); });
  e.hp.mark(kHpSynced);
  a.laps.finish();
  e.hp.mark(kHpLaps);
  a.ntok = *pinned<uint64_t>(ds, kPinNtok);
  if (a.w.wgrec) print_wgrec(a.w.wgrec);
  if (a.w.stamps) print_stamps(a.w.stamps, a.w.n_tiles);
  for (int i = 0; i < kNumCounters; i++) a.cnt[i] = pinned<uint32_t>(ds, kPinFinal)[i];
}

Outcome run_attempt(Enc& e, Attempt& a) {
  normalise(e, a);
  size_workspace(e, a);
  launch_pretok(e, a);
  if (e.c.mode == EncodeMode::SegmentOnly) return finish_segment_only(e, a);
  launch_merges(e, a);
  launch_tail(e, a);
  read_results(e, a);
  const Outcome o = call_outcome(a.cnt, a.ntok, e.c.ids_cap, a.w.nfc_watch, a.safe, a.w.long_cap);
  if (o == Outcome::ErrOverflow)
    throw_err(CTOK_E_DEVICE, "a piece list overflowed its safe capacity: the call's ids were not written");
  if (o == Outcome::ErrPanic)
    throw_err(CTOK_E_PANIC, "index out of bounds: a merge rank points past the list of valid merges (reference src/bpe.rs:141 panics)");
  if (o == Outcome::ErrCapacity) throw_err(CTOK_E_CAPACITY, "ids_cap too small: tok_off[n_docs] holds the number of ids needed");
  return o;
}

// The flagged docs of a finished speculative attempt, encoded again normalised
void splice_flagged(Enc& e, Attempt& a) {
  const EncodeCall& c = e.c;
  a.ntok = nfc_splice(e.t, e.ds, c, a.ntok, &a.nfc_docs);
  if (c.timing) {
    HIPTRY(hipEventRecord(e.ds->ev[kEvSpliceEnd], c.stream));
    HIPTRY(hipEventSynchronize(e.ds->ev[kEvSpliceEnd]));
  }
  if (a.ntok > c.ids_cap) throw_err(CTOK_E_CAPACITY, "ids_cap too small: tok_off[n_docs] holds the number of ids needed");
}

void fill_stats(const Enc& e, const Attempt& a, bool spliced) {
  ctok_stats* st = e.c.stats;
  if (!st) return;
  const uint32_t* cnt = a.cnt;
  st->bytes_in = e.c.n_bytes;
  st->bytes_norm = a.B;
  st->docs = e.c.n_docs;
  st->pieces = a.w.n_tiles ? cnt[kCtrPieces] : 0;
  st->long_pieces = cnt[kCtrLong];
  st->tokens = a.ntok;
  st->workspace_bytes = e.ds->workspace_bytes();
  st->long_rounds = cnt[kCtrRounds];
  st->nfc_docs = a.nfc_docs;
  for (int c = 0; c < kNumClasses; c++) {
    st->class_bytes[c] = cnt[ctr_stat(c)];
    st->class_ids[c] = cnt[ctr_stat(c) + 1];
  }
  if (!a.tm) return;
  const Laps& l = a.laps;
  st->ms_pretok = l.ms(l.pretok);
  st->ms_segment = l.ms(l.segment);
  st->ms_bpe_lo = l.ms(l.lo);
  st->ms_bpe_hi = std::max(0.0, l.ms(l.mid));
  st->ms_bpe_med = l.ms(l.c3);
  // the merge passes (k_segment's end to the last one's end) and the side stream's long tiers
  // past them (the tail's start waits for the join)
  st->ms_bpe_short = std::max(l.ms(l.to_short), std::max(l.ms(l.to_mid), l.ms(l.to_c3)));
  st->ms_bpe_long = std::max(0.0, l.ms(l.to_tail) - st->ms_bpe_short);
  st->ms_emit = l.ms(l.emit);
  st->ms_device = l.ms(l.device);
  if (spliced) {  // (the NFC splice ran after the main call: kEvSpliceEnd ends it)
    float v = 0;
    HIPTRY(hipEventElapsedTime(&v, e.ds->ev[kEvStart], e.ds->ev[kEvSpliceEnd]));
    st->ms_device = v;
  }
}

// The pipeline on device-resident buffers.  Returns the token count.
uint64_t encode_device(ctok* t, DeviceState* ds, const EncodeCall& c) {
  if (c.n_bytes >= 0xF0000000ull) throw_err(CTOK_E_ARG, "a single call is limited to < 3.75 GiB of text; split the batch");
  if (c.n_docs >= 0xF0000000ull) throw_err(CTOK_E_ARG, "too many documents in one call");
  Enc e{t, ds, c, ds->t, false, CallKnobs(), HostProf()};
  if (!c.split_added) e.tb.n_at = 0;
  e.splice = c.ids && c.mode == EncodeMode::Ids && !e.knobs.nfc_rerun;
  // all_nfc: no speculation and no check, every doc is normalised
  bool speculate = t->nfc && !t->add_prefix_space && c.n_bytes && !c.all_nfc && !e.knobs.no_nfc_speculation;
  // lean list capacities first; a call whose lists outgrow them runs again with the safe ones
  bool safe = process_knobs().safe_capacities;
  e.hp.mark(kHpEntry);
  for (;;) {
    Attempt a{speculate, safe};
    const Outcome o = run_attempt(e, a);
    if (o == Outcome::RerunNormalised) { speculate = false; continue; }
    if (o == Outcome::RerunSafe) { safe = true; continue; }
    if (c.mode == EncodeMode::SegmentOnly) return 0;
    if (o == Outcome::Splice) splice_flagged(e, a);
    fill_stats(e, a, o == Outcome::Splice);
    e.hp.mark(kHpEnd);
    e.hp.print();
    return a.ntok;
  }
}

}  // namespace ctok_rt

