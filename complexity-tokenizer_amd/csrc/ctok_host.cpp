// C++ host runtime behind the C ABI (include/ctok.h): the entry points on device and host
// buffers -- decode, the host-buffer encode pipeline, padded encode, offsets -- and the GPU
// pre-tokenizer for the trainer.  The loader is ctok_load.cpp (with bpe_model.cpp and
// table_compile.cpp), encode_device ctok_encode.cpp (host_internal.h).
//
// Reference counterparts (Complexity-ML/complexity-tokenizer v0.3.3):
//   decode            src/huggingface/mod.rs:698-785, src/decoders.rs:74-119, parsing.rs:272-364
#include <emmintrin.h>

#include <cstdio>
#include <cstring>
#include <string_view>

#include "host_internal.h"
#include "knobs.h"
#include "window_hd.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {

thread_local std::string g_err;

// ----------------------------------------------------------------------------- entry-point prologues

// Document (or token) offsets of a host batch: off[0] == 0 and off[0..n] non-decreasing
void check_offsets(const uint64_t* off, uint64_t n, const char* name) {
  if (off[0] != 0) throw_err(CTOK_E_ARG, std::string(name) + "[0] must be 0");
  for (uint64_t d = 0; d < n; d++)
    if (off[d + 1] < off[d]) throw_err(CTOK_E_ARG, std::string(name) + " must be non-decreasing");
}

// One call on a device, from its ctok_exec (null: device 0, the library's stream, no timing): the
// device's state with its mutex held and the device current on this thread until the scope ends
struct DeviceCall {
  int dev;
  DeviceState* ds;
  std::lock_guard<std::recursive_mutex> lock;
  hipStream_t s;
  bool timing;
  DeviceCall(ctok* t, const ctok_exec* exec)
      : dev(exec ? exec->device : 0), ds(device_state(t, dev)), lock(ds->mu),
        s(exec && exec->stream ? (hipStream_t)exec->stream : ds->stream), timing(exec && (exec->flags & CTOK_F_TIMING)) {
    HIPTRY(hipSetDevice(dev));
  }
  DeviceCall(ctok* t, int device) : dev(device), ds(device_state(t, dev)), lock(ds->mu), s(ds->stream), timing(false) {
    HIPTRY(hipSetDevice(dev));
  }
};

// The text and the ids of a device entry point (include/ctok.h, "Buffers of the device entry
// points"): refused at the entry, before the device is looked up, so that no kernel -- k_nfc_check
// and k_norm read the caller's text before the pipeline does -- runs on a misaligned pointer.  (The
// library's own text buffers, norm_text and sub_text among them, are allocations and so aligned.)
void check_device_text(const uint8_t* d_utf8, uint64_t n_bytes) {
  if (n_bytes && ((uintptr_t)d_utf8 & 15)) throw_err(CTOK_E_ARG, "device text buffer must be 16-byte aligned");
}
void check_device_ids(const uint32_t* d_ids, uint64_t n_ids) {
  if (n_ids && ((uintptr_t)d_ids & 3)) throw_err(CTOK_E_ARG, "device ids buffer must be 4-byte aligned");
}

// A host batch on the device, in pad_in_text (16 zero bytes after it) and pad_in_off
void stage_host_batch(DeviceState* ds, const uint8_t* utf8, const uint64_t* off, uint64_t n_docs, hipStream_t s) {
  const uint64_t B = off[n_docs];
  ds->pad_in_text.ensure(B + 16);
  ds->pad_in_off.ensure(n_docs + 1);
  if (B) HIPTRY(hipMemcpyAsync(ds->pad_in_text.p, utf8, B, hipMemcpyHostToDevice, s));
  HIPTRY(hipMemsetAsync(ds->pad_in_text.p + B, 0, 16, s));
  HIPTRY(hipMemcpyAsync(ds->pad_in_off.p, off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
}

// ----------------------------------------------------------------------------- decode

void ensure_decode_tables(ctok* t, DeviceState* ds, hipStream_t s) {
  if (ds->dec_ready) return;
  upload(ds->dec_ent, t->dec_ent.data(), t->dec_ent.size(), s);
  upload(ds->dec_bytes, t->dec_bytes.data(), t->dec_bytes.size(), s);
  HIPTRY(hipStreamSynchronize(s));
  ds->dec_ready = true;
}

// decode_batch_with_options on device-resident ids (src/huggingface/mod.rs:771-785).  Returns
// the output byte count; get_out(n) supplies an output buffer of >= n bytes (or throws).
uint64_t decode_device(ctok* t, DeviceState* ds, const uint32_t* d_ids, const uint64_t* d_tok_off, uint64_t n_docs,
                       uint64_t n_ids, uint32_t opts, const std::function<uint8_t*(uint64_t)>& get_out,
                       uint64_t* d_out_off, hipStream_t s, bool timing, ctok_decode_stats* st) {
  if (t->decoder < 0)
    throw_err(CTOK_E_UNSUPPORTED, "decoder " + t->decoder_name + " is outside the ByteLevel-BPE decode path");
  if (n_ids >= 0xF0000000ull || n_docs >= 0xF0000000ull)
    throw_err(CTOK_E_ARG, "a single decode call is limited to < 3.75 G ids and docs; split the batch");
  ensure_decode_tables(t, ds, s);
  DecTables tb{(const uint2*)ds->dec_ent.p, (uint32_t)(t->dec_ent.size() / 2), ds->dec_bytes.p};
  DecWork w{};
  w.ids = d_ids;
  w.n_ids = (uint32_t)n_ids;
  w.tok_off = d_tok_off;
  w.n_docs = (uint32_t)n_docs;
  w.opts = opts & (kDecOptSkipSpecial | kDecOptCleanup);
  w.n_chunks = (uint32_t)((n_ids + kDecChunk - 1) / kDecChunk);
  ds->dec_chunk.ensure(w.n_chunks + 8);
  ds->dec_cnt.ensure(8);
  ds->scan_tmp.ensure(scan_tmp_elems(w.n_chunks + 1) + 64);
  w.chunk_off = ds->dec_chunk.p;
  w.counters = ds->dec_cnt.p;
  if (timing) HIPTRY(hipEventRecord(ds->dev_ev[0], s));
  HIPTRY(hipMemsetAsync(ds->dec_cnt.p, 0, 32, s));
  HIPTRY(launch_dec_len(w, tb, (uint32_t*)ds->scan_tmp.p, ds->scan_tmp.cap * 2, s));
  if (timing) HIPTRY(hipEventRecord(ds->dev_ev[1], s));
  HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, ds->dec_cnt.p, 16, hipMemcpyDeviceToHost, s));
  spin_sync(ds, s);
  const uint32_t err = pinned<uint32_t>(ds, kPinScratch)[0], nonascii = pinned<uint32_t>(ds, kPinScratch)[1];
  const uint64_t R = pinned<uint64_t>(ds, kPinScratch)[1];
  if (err) throw_err(CTOK_E_ARG, "tok_off must start at 0, be non-decreasing and end at the number of ids");
  if (R >= 0xF0000000ull) throw_err(CTOK_E_ARG, "decoded batch exceeds 3.75 GiB; split the batch");
  const bool direct = !(w.opts & kDecOptCleanup) && !nonascii;
  uint64_t n_out = R;
  if (direct) {  // every unit is a valid ASCII byte and nothing is cleaned: the gather is the output
    uint8_t* d_out = get_out(R);
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[2], s));
    HIPTRY(launch_dec_gather(w, tb, d_out, d_out_off, s));
    if (!n_ids) HIPTRY(hipMemsetAsync(d_out_off, 0, (n_docs + 1) * 8, s));
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[3], s));
  } else {
    ds->dec_raw.ensure(R + 64);
    ds->dec_rawoff.ensure(n_docs + 1);
    w.raw = ds->dec_raw.p;
    w.n_raw = (uint32_t)R;
    w.raw_off = ds->dec_rawoff.p;
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[2], s));
    HIPTRY(launch_dec_gather(w, tb, w.raw, w.raw_off, s));
    if (!n_ids) HIPTRY(hipMemsetAsync(w.raw_off, 0, (n_docs + 1) * 8, s));
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[3], s));
    w.n_tiles = (uint32_t)((R + kDecTile - 1) / kDecTile);
    ds->dec_tile.ensure(w.n_tiles + 8);
    ds->dec_del.ensure(R / 32 + 8);
    ds->scan_tmp.ensure(scan_tmp_elems(w.n_tiles + 1) + 64);
    w.tile_cnt = ds->dec_tile.p;
    w.delbits = ds->dec_del.p;
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[4], s));
    if (w.opts & kDecOptCleanup) HIPTRY(hipMemsetAsync(w.delbits, 0, (R / 32 + 8) * 4, s));
    HIPTRY(launch_dec_prepare(w, s));
    HIPTRY(launch_dec_count(w, (uint32_t*)ds->scan_tmp.p, ds->scan_tmp.cap * 2, s));
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[5], s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, w.tile_cnt + w.n_tiles, 4, hipMemcpyDeviceToHost, s));
    spin_sync(ds, s);
    n_out = pinned<uint32_t>(ds, kPinScratch)[0];
    uint8_t* d_out = get_out(n_out);
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[6], s));
    HIPTRY(launch_dec_write(w, d_out, d_out_off, s));
    if (!R) HIPTRY(hipMemsetAsync(d_out_off, 0, (n_docs + 1) * 8, s));
    if (timing) HIPTRY(hipEventRecord(ds->dev_ev[7], s));
  }
  if (st) {
    st->ids = n_ids;
    st->docs = n_docs;
    st->bytes_raw = R;
    st->bytes_out = n_out;
    st->direct = direct ? 1 : 0;
    if (timing) {
      HIPTRY(hipEventSynchronize(ds->dev_ev[direct ? 3 : 7]));
      auto el = [&](int i, int j) {
        float v = 0;
        HIPTRY(hipEventElapsedTime(&v, ds->dev_ev[i], ds->dev_ev[j]));
        return (double)v;
      };
      st->ms_len = el(0, 1);
      st->ms_gather = el(2, 3);
      st->ms_clean = direct ? 0.0 : el(4, 5) + el(6, 7);
      st->ms_device = st->ms_len + st->ms_gather + st->ms_clean;
    }
  }
  return n_out;
}

// ----------------------------------------------------------------------------- host-buffer pipeline
//
// ctok_encode_batch on host memory.  The batch is cut into chunks of about `chunk` text bytes
// (whole documents); per chunk c (slot c & 1):
//   stage   the up stream copies the chunk's text from the caller's buffer to d_in and its
//           offsets to d_off, made chunk-relative on the device                  (ev_h2d)
//   encode  the encode stream waits for ev_h2d (and for the D2H of chunk c - 2, which used the
//           same d_ids), runs encode_device, adds the running token base to tok_off (ev_enc)
//   drain   the down stream copies ids / tok_off straight into the caller's ids (at the running
//           token base) and tok_off                                              (ev_d2h)
// stage(c + 1) and drain(c - 1) run on helper threads while encode(c) runs, so PCIe traffic in
// both directions overlaps the kernels.  The copies touch the caller's pageable memory directly:
// the runtime pins it in place at the link's rate (56-57 GB/s each way on the MI355X box, the same
// as from hipHostMalloc memory; profiles/r03/pcie_probe.txt), so staging through pinned buffers
// only added two host memcpys per byte (round 2: 16.3 GB/s E2E on C2).

// dst[i] = src[i] for i < n, with non-temporal 16-byte stores (the caller's ids are written once
// and not read back here: no read-for-ownership of their lines)
void widen16(uint32_t* dst, const uint16_t* src, size_t n) {
  size_t i = 0;
  for (; i < n && ((uintptr_t)(dst + i) & 15u); i++) dst[i] = src[i];
  const __m128i z = _mm_setzero_si128();
  for (; i + 8 <= n; i += 8) {
    const __m128i v = _mm_loadu_si128((const __m128i*)(src + i));
    _mm_stream_si128((__m128i*)(dst + i), _mm_unpacklo_epi16(v, z));
    _mm_stream_si128((__m128i*)(dst + i + 4), _mm_unpackhi_epi16(v, z));
  }
  for (; i < n; i++) dst[i] = src[i];
  _mm_sfence();
}

HostPipe* host_pipe(DeviceState* ds) {
  if (ds->pipe) return ds->pipe.get();
  auto p = std::make_unique<HostPipe>();
  HIPTRY(hipStreamCreateWithFlags(&p->up, hipStreamNonBlocking));
  HIPTRY(hipStreamCreateWithFlags(&p->down, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    HIPTRY(hipEventCreateWithFlags(&p->ev_h2d[i], hipEventDisableTiming));
    HIPTRY(hipEventCreateWithFlags(&p->ev_enc[i], hipEventDisableTiming));
    HIPTRY(hipEventCreateWithFlags(&p->ev_d2h[i], hipEventDisableTiming));
  }
  for (auto& e : p->ev_t) HIPTRY(hipEventCreate(&e));
  ds->pipe = std::move(p);
  return ds->pipe.get();
}

struct RangeOut {
  uint64_t ntok = 0;     // ids of the range
  bool overflow = false;  // ntok > cap: nothing past cap was written
};

// Encode docs [d0, d1) of a host batch on one device; ids go to ids[0, cap), tok_off[i] (i in
// [1, d1 - d0]) = ids of docs d0 .. d0 + i - 1 (tok_off[0] is not written: with several shards
// it is the previous shard's last entry).  The device lock is held by the caller.
RangeOut encode_host_range(ctok* t, DeviceState* ds, const uint8_t* text, const uint64_t* off, uint64_t d0,
                           uint64_t d1, uint32_t* ids, uint64_t cap, uint64_t* tok_off, uint64_t chunk,
                           unsigned nthreads, bool timing, ctok_stats* st) {
  RangeOut r;
  if (d1 <= d0) return r;
  HostPipe* P = host_pipe(ds);
  hipStream_t s = ds->stream;
  // chunk boundaries: whole docs, about `chunk` bytes each (a longer doc is a chunk by itself),
  // ramped: the first chunks grow from chunk / 8 and the last ones shrink to it, so the first
  // upload and the last download, which nothing overlaps, are short
  const bool no_ramp = process_knobs().no_chunk_ramp;
  const uint64_t c_min = std::max<uint64_t>(chunk / 8, 1u << 20);
  uint64_t want = no_ramp ? chunk : c_min;
  std::vector<uint64_t> cut{d0};
  while (cut.back() < d1) {
    const uint64_t a = cut.back(), left = off[d1] - off[a];
    uint64_t sz = no_ramp ? chunk : std::min(std::min(want, chunk), std::max(c_min, left / 2));
    if (left < sz + c_min) sz = left;  // no small remainder
    want = std::min(2 * want, chunk);
    const uint64_t* e = std::upper_bound(off + a + 1, off + d1 + 1, off[a] + sz);
    uint64_t b = (uint64_t)(e - off) - 1;  // last doc end <= off[a] + chunk
    if (b <= a) b = a + 1;
    cut.push_back(std::min(b, d1));
  }
  const size_t C = cut.size() - 1;
  std::vector<uint64_t> ntok(C, 0), base(C + 1, 0);
  double ms_h2d = 0, ms_d2h = 0, ms_dev = 0, ms_pre = 0, ms_bs = 0, ms_bl = 0, ms_em = 0, ms_seg = 0, ms_lo = 0, ms_hi = 0;
  double ms_med = 0;

  // stage / drain run on helper threads: each makes the shard's device current first (the HIP
  // current device is per thread).  Both copy straight between the caller's (pageable) buffers
  // and the device: the runtime pins the pages in place and copies at the link's rate, as fast as
  // from pinned memory (profiles/r03/pcie_probe.txt), so there is no staging copy on the host.
  const bool trace = process_knobs().pipe_trace;
  const double tr0 = now_ms();
  auto TR = [&](const char* what, size_t c) { if (trace) fprintf(stderr, "[pipe] %8.3f %s %zu\n", now_ms() - tr0, what, c); };
  auto stage = [&](size_t c) {
    TR("stage<", c);
    HIPTRY(hipSetDevice(ds->device));
    const int k = (int)(c & 1);
    const uint64_t a = cut[c], b = cut[c + 1], n = b - a, B = off[b] - off[a];
    // (d_in[k] / d_off[k] were last read by chunk c - 2's encode, which has returned)
    if (timing && c == 0) HIPTRY(hipEventRecord(P->ev_t[0], P->up));
    if (B) HIPTRY(hipMemcpyAsync(P->d_in[k].p, text + off[a], B, hipMemcpyHostToDevice, P->up));
    HIPTRY(hipMemsetAsync(P->d_in[k].p + B, 0, 16, P->up));
    HIPTRY(hipMemcpyAsync(P->d_off[k].p, off + a, (n + 1) * 8, hipMemcpyHostToDevice, P->up));
    HIPTRY(shift_u64(P->d_off[k].p, n + 1, (uint64_t)0 - off[a], P->up));  // chunk-relative offsets
    if (timing && c == 0) HIPTRY(hipEventRecord(P->ev_t[1], P->up));
    HIPTRY(hipEventRecord(P->ev_h2d[k], P->up));
    if (trace) { HIPTRY(hipEventSynchronize(P->ev_h2d[k])); TR("stage>", c); }
  };
  // ids16 tokenizers: the ids cross the link as u16 and tok_off as u32 (k_wire16), into pinned
  // buffers, and host threads widen them into the caller's buffers (which also first-touches
  // fresh output pages on several threads); the link is the E2E bound (56 GB/s for both
  // directions together), and this moves 2 B per id instead of 4
  const bool w16 = t->ids16 && !CallKnobs().wire32;
  ds->last_wire16 = w16 ? 1 : 0;
  auto drain = [&](size_t c) {
    HIPTRY(hipSetDevice(ds->device));
    const int k = (int)(c & 1);
    const uint64_t a = cut[c], n = cut[c + 1] - a;
    const uint64_t b0 = base[c], nt = ntok[c];
    const uint64_t nc = b0 < cap ? std::min(nt, cap - b0) : 0;  // ids that fit the caller's buffer
    uint64_t* dst_off = tok_off + (a - d0);
    HIPTRY(hipStreamWaitEvent(P->down, P->ev_enc[k], 0));  // chunk c's ids and tok_off
    if (timing && c + 1 == C) HIPTRY(hipEventRecord(P->ev_t[2], P->down));
    if (w16) {
      P->pin_ids16[k].ensure(nt + 8);
      P->pin_toff32[k].ensure(n + 1);
      if (nc) HIPTRY(hipMemcpyAsync(P->pin_ids16[k].p, P->d_ids16[k].p, nc * 2, hipMemcpyDeviceToHost, P->down));
      HIPTRY(hipMemcpyAsync(P->pin_toff32[k].p, P->d_toff32[k].p, (n + 1) * 4, hipMemcpyDeviceToHost, P->down));
    } else {
      if (nc) HIPTRY(hipMemcpyAsync(ids + b0, P->d_ids[k].p, nc * 4, hipMemcpyDeviceToHost, P->down));
      if (n) HIPTRY(hipMemcpyAsync(dst_off + 1, P->d_tokoff[k].p + 1, n * 8, hipMemcpyDeviceToHost, P->down));
    }
    if (timing && c + 1 == C) HIPTRY(hipEventRecord(P->ev_t[3], P->down));
    HIPTRY(hipEventRecord(P->ev_d2h[k], P->down));
    TR("drain<", c);
    HIPTRY(hipEventSynchronize(P->ev_d2h[k]));
    TR("d2h>", c);
  };
  // widen(c) (w16): chunk c's 16-bit ids / 32-bit tok_off from the pinned slot into the caller's
  // buffers, on up to nthreads threads.  Runs on its own thread, overlapping the next chunks'
  // copies; joined before the slot is drained into again (wid[c & 1]) and at the end.
  auto widen = [&](size_t c) {
    const int k = (int)(c & 1);
    const uint64_t a = cut[c], n = cut[c + 1] - a;
    const uint64_t b0 = base[c], nt = ntok[c];
    const uint64_t nc = b0 < cap ? std::min(nt, cap - b0) : 0;
    const uint16_t* src = P->pin_ids16[k].p;
    uint32_t* dst = ids + b0;
    const unsigned nw = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nthreads, nc >> 20));
    const uint64_t per = (nc + nw - 1) / nw;
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nw; i++)
      th.emplace_back([=] { const uint64_t lo = std::min(nc, i * per); widen16(dst + lo, src + lo, std::min(nc, lo + per) - lo); });
    widen16(dst, src, std::min(nc, per));
    const uint32_t* to = P->pin_toff32[k].p;
    uint64_t* dst_off = tok_off + (a - d0);
    for (uint64_t i = 1; i <= n; i++) dst_off[i] = b0 + to[i];
    for (auto& x : th) x.join();
    TR("widen>", c);
  };
  CatchThread wid[2];
  auto start_widen = [&](size_t c) { wid[c & 1].start([&, c] { widen(c); }); };
  auto join_widen = [&](int k) { wid[k].join(); };
  // device buffers sized for the largest chunk up front (no reallocation while copies are in flight)
  {
    uint64_t maxB = 0, maxD = 0;
    for (size_t c = 0; c < C; c++) {
      maxB = std::max(maxB, off[cut[c + 1]] - off[cut[c]]);
      maxD = std::max(maxD, cut[c + 1] - cut[c]);
    }
    for (int k = 0; k < 2; k++) {
      P->d_in[k].ensure(maxB + 16);
      P->d_off[k].ensure(maxD + 1);
      P->d_tokoff[k].ensure(maxD + 1);
      P->d_ids[k].ensure(ctok_ids_bound(t, maxB, maxD));
      if (w16) {
        P->d_ids16[k].ensure(ctok_ids_bound(t, maxB, maxD));
        P->d_toff32[k].ensure(maxD + 1);
      }
    }
  }
  stage(0);
  for (size_t c = 0; c < C; c++) {
    const int k = (int)(c & 1);
    const uint64_t a = cut[c], n = cut[c + 1] - a, B = off[cut[c + 1]] - off[a];
    // helper threads: chunk c + 1 goes up and chunk c - 1 comes down while chunk c is encoded;
    // an exception inside one is rethrown here after the join
    CatchThread th_stage, th_drain;
    if (c + 1 < C) th_stage.start([&, c] { stage(c + 1); });
    if (c >= 1) join_widen((int)((c - 1) & 1));  // (widen(c - 3) read the pinned slot drain(c - 1) fills)
    if (c >= 1) th_drain.start([&, c] { drain(c - 1); });
    HIPTRY(hipStreamWaitEvent(s, P->ev_h2d[k], 0));
    HIPTRY(hipStreamWaitEvent(s, P->ev_d2h[k], 0));  // chunk c - 2's ids have left d_ids[k]
    ctok_stats cs{};
    TR("enc<", c);
    EncodeCall call;
    call.text = P->d_in[k].p, call.doc_off = P->d_off[k].p, call.n_docs = n, call.n_bytes = B;
    call.ids = P->d_ids[k].p, call.ids_cap = P->d_ids[k].cap, call.tok_off = P->d_tokoff[k].p;
    call.stream = s, call.timing = timing, call.stats = &cs;
    ntok[c] = encode_device(t, ds, call);
    base[c + 1] = base[c] + ntok[c];
    TR("enc>", c);
    if (st) {
      st->pieces += cs.pieces;
      st->long_pieces += cs.long_pieces;
      st->long_rounds += cs.long_rounds;
      st->nfc_docs += cs.nfc_docs;
      st->workspace_bytes = std::max(st->workspace_bytes, cs.workspace_bytes);
      st->bytes_norm += cs.bytes_norm;
      for (int q = 0; q < kNumClasses; q++) {
        st->class_bytes[q] += cs.class_bytes[q];
        st->class_ids[q] += cs.class_ids[q];
      }
      ms_dev += cs.ms_device, ms_pre += cs.ms_pretok, ms_bs += cs.ms_bpe_short, ms_bl += cs.ms_bpe_long;
      ms_em += cs.ms_emit, ms_seg += cs.ms_segment, ms_lo += cs.ms_bpe_lo, ms_hi += cs.ms_bpe_hi;
      ms_med += cs.ms_bpe_med;
    }
    if (w16)
      HIPTRY(wire16(P->d_ids[k].p, ntok[c], P->d_ids16[k].p, P->d_tokoff[k].p, n + 1, P->d_toff32[k].p, s));
    else
      HIPTRY(shift_u64(P->d_tokoff[k].p + 1, n, base[c], s));  // batch-relative tok_off
    HIPTRY(hipEventRecord(P->ev_enc[k], s));
    th_drain.join();
    if (c >= 1 && w16) start_widen(c - 1);
    th_stage.join();
  }
  join_widen((int)((C - 1) & 1));
  drain(C - 1);
  if (w16) widen(C - 1);
  join_widen(0);
  join_widen(1);
  r.ntok = base[C];
  r.overflow = r.ntok > cap;
  if (st && timing) {
    float v = 0;
    HIPTRY(hipEventElapsedTime(&v, P->ev_t[0], P->ev_t[1]));
    ms_h2d = v;
    HIPTRY(hipEventElapsedTime(&v, P->ev_t[2], P->ev_t[3]));
    ms_d2h = v;
    st->ms_h2d += ms_h2d, st->ms_d2h += ms_d2h, st->ms_device += ms_dev, st->ms_pretok += ms_pre;
    st->ms_bpe_short += ms_bs, st->ms_bpe_long += ms_bl, st->ms_emit += ms_em, st->ms_segment += ms_seg;
    st->ms_bpe_lo += ms_lo, st->ms_bpe_hi += ms_hi, st->ms_bpe_med += ms_med;
  }
  return r;
}

int run(const std::function<void()>& f) {
  try {
    f();
    g_err.clear();
    return CTOK_OK;
  } catch (const CtokError& e) {
    return fail(e.code, e.msg);
  } catch (const std::bad_alloc&) {
    return fail(CTOK_E_DEVICE, "out of host memory");
  } catch (const std::exception& e) {
    return fail(CTOK_E_ARG, e.what());
  }
}

// NFC (when the tokenizer normalises) + ByteLevel pre-tokenization of a host batch on dc's device:
// what it leaves there (*norm: the text and offsets are the normalised ones, not the staged input)
ctok_host::DevicePretok pretokenize_staged(ctok* t, DeviceCall& dc, const uint8_t* utf8, const uint64_t* doc_off,
                                           uint64_t n_docs, bool* norm) {
  DeviceState* ds = dc.ds;
  stage_host_batch(ds, utf8, doc_off, n_docs, dc.s);
  EncodeCall call;
  call.text = ds->pad_in_text.p, call.doc_off = ds->pad_in_off.p, call.n_docs = n_docs, call.n_bytes = doc_off[n_docs];
  call.stream = dc.s;
  call.mode = EncodeMode::SegmentOnly;
  encode_device(t, ds, call);
  *norm = ds->last_norm;
  ctok_host::DevicePretok r;
  r.text = *norm ? ds->norm_text.p : ds->pad_in_text.p;
  r.doc_off = *norm ? ds->norm_off.p : ds->pad_in_off.p;
  r.pbits = ds->pbits.p;
  r.n_bytes = ds->last_B;
  r.n_docs = n_docs;
  r.stream = dc.s;
  return r;
}

void check_host_batch(const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, const char* name) {
  check_offsets(doc_off, n_docs, name);
  if (doc_off[n_docs] && !utf8) throw_err(CTOK_E_ARG, "null text");
}

}  // namespace ctok_rt

using namespace ctok_rt;

// ----------------------------------------------------------------------------- internal API
// for trainer_host.cpp (host_common.h): errors, and the GPU pre-tokenizer of a host batch

namespace ctok_host {
[[noreturn]] void throw_error(int code, const std::string& msg) { throw_err(code, msg); }
int run_guarded(const std::function<void()>& f) { return run(f); }
unsigned usable_cpus() { return usable_cpus_once(); }

// The text the pieces index (normalised when normalisation ran), its doc offsets, and the
// piece-start bitmap (bit g = a piece starts at byte g), copied back to the host.
void pretokenize(ctok* t, int dev, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                 std::vector<uint8_t>& text, std::vector<uint64_t>& off, std::vector<uint32_t>& pbits,
                 uint64_t* bytes_d2h) {
  check_host_batch(utf8, doc_off, n_docs, "offsets");
  DeviceCall dc(t, dev);
  bool norm;
  const DevicePretok r = pretokenize_staged(t, dc, utf8, doc_off, n_docs, &norm);
  const uint64_t B = r.n_bytes;
  pbits.assign((B + 31) / 32, 0);
  off.resize(n_docs + 1);
  text.resize(B);
  if (!pbits.empty()) HIPTRY(hipMemcpyAsync(pbits.data(), r.pbits, pbits.size() * 4, hipMemcpyDeviceToHost, dc.s));
  if (norm) {
    if (B) HIPTRY(hipMemcpyAsync(text.data(), r.text, B, hipMemcpyDeviceToHost, dc.s));
    HIPTRY(hipMemcpyAsync(off.data(), r.doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, dc.s));
  }
  HIPTRY(hipStreamSynchronize(dc.s));
  if (!norm) {
    if (B) std::memcpy(text.data(), utf8, B);
    std::memcpy(off.data(), doc_off, (n_docs + 1) * 8);
  }
  if (bytes_d2h) *bytes_d2h = pbits.size() * 4 + (norm ? B + (n_docs + 1) * 8 : 0);
}

// The same pre-tokenization with nothing copied back: `use` runs under the device's mutex with the
// device-resident text, doc offsets and piece-start bitmap, which stay valid until it returns.
void pretokenize_device(ctok* t, int dev, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                        const std::function<void(const DevicePretok&)>& use) {
  check_host_batch(utf8, doc_off, n_docs, "offsets");
  DeviceCall dc(t, dev);
  bool norm;
  use(pretokenize_staged(t, dc, utf8, doc_off, n_docs, &norm));
}
}  // namespace ctok_host

// ----------------------------------------------------------------------------- C ABI

extern "C" {

const char* ctok_last_error(void) { return g_err.c_str(); }
const char* ctok_version(void) { return "0.3.3+mi355x.1"; }

int ctok_get_table_props(const ctok* tc, int device, ctok_table_props* out) {
  if (!tc || !out) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  *out = ctok_table_props{t->narrow, t->compact, t->short_packed, t->ids16, -1, -1, -1, -1, -1};
  std::lock_guard<std::mutex> lk(t->dev_mu);
  auto it = t->devs.find(device);
  if (it != t->devs.end()) {
    const DeviceState& ds = *it->second;
    out->dev_narrow = (int)ds.t.narrow;
    out->dev_short_packed = (int)ds.t.short_packed;
    out->last_rec16 = ds.last_rec16;
    out->last_wire16 = ds.last_wire16;
    out->dev_mid_packed = (int)ds.t.mid_packed;
  }
  return CTOK_OK;
}

int ctok_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ctok_encode_batch_device(const ctok* tc, const uint8_t* d_utf8, const uint64_t* d_doc_off, uint64_t n_docs,
                             uint64_t n_bytes, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_tok_off,
                             uint64_t* n_tokens_out, const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !d_doc_off || !d_tok_off || (n_bytes && (!d_utf8 || !d_ids))) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    check_device_text(d_utf8, n_bytes);
    DeviceCall dc(t, exec);
    EncodeCall call;
    call.text = d_utf8, call.doc_off = d_doc_off, call.n_docs = n_docs, call.n_bytes = n_bytes;
    call.ids = d_ids, call.ids_cap = ids_cap, call.tok_off = d_tok_off;
    call.stream = dc.s, call.timing = dc.timing, call.stats = stats;
    uint64_t n = encode_device(t, dc.ds, call);
    if (n_tokens_out) *n_tokens_out = n;
    if (stats) stats->ms_total = now_ms() - t0;
  });
}

int ctok_decode_batch_device(const ctok* tc, const uint32_t* d_ids, const uint64_t* d_tok_off, uint64_t n_docs,
                             uint64_t n_ids, uint32_t options, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                             uint64_t* n_bytes_out, const ctok_exec* exec, ctok_decode_stats* stats) {
  if (!tc || !d_tok_off || !d_out_off || (n_ids && !d_ids)) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    check_device_ids(d_ids, n_ids);
    DeviceCall dc(t, exec);
    auto get_out = [&](uint64_t n) -> uint8_t* {
      if (n_bytes_out) *n_bytes_out = n;
      if (n > out_cap) throw_err(CTOK_E_CAPACITY, "out_cap too small: *n_bytes_out holds the number of bytes needed");
      if (n && !d_out) throw_err(CTOK_E_ARG, "null output buffer");
      return d_out;
    };
    uint64_t n = decode_device(t, dc.ds, d_ids, d_tok_off, n_docs, n_ids, options, get_out, d_out_off, dc.s, dc.timing, stats);
    if (n_bytes_out) *n_bytes_out = n;
    if (stats) stats->ms_total = now_ms() - t0;
  });
}

int ctok_decode_batch(const ctok* tc, const uint32_t* ids, const uint64_t* tok_off, uint64_t n_docs, uint32_t options,
                      uint8_t* out, uint64_t out_cap, uint64_t* out_off, const ctok_exec* exec,
                      ctok_decode_stats* stats) {
  if (!tc || !tok_off || !out_off) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    check_offsets(tok_off, n_docs, "tok_off");
    const uint64_t T = tok_off[n_docs];
    if (T && !ids) throw_err(CTOK_E_ARG, "null ids");
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    double h0 = now_ms();
    ds->dec_ids.ensure(T + 4);
    ds->dec_tokoff.ensure(n_docs + 1);
    ds->dec_outoff.ensure(n_docs + 1);
    if (T) HIPTRY(hipMemcpyAsync(ds->dec_ids.p, ids, T * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(ds->dec_tokoff.p, tok_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HIPTRY(hipStreamSynchronize(s));
    double h1 = now_ms();
    auto get_out = [&](uint64_t n) -> uint8_t* {
      ds->dec_out.ensure(n + 16);
      return ds->dec_out.p;
    };
    uint64_t n = decode_device(t, ds, ds->dec_ids.p, ds->dec_tokoff.p, n_docs, T, options, get_out, ds->dec_outoff.p,
                               s, dc.timing, stats);
    double d0 = now_ms();
    HIPTRY(hipMemcpyAsync(out_off, ds->dec_outoff.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n <= out_cap && n) HIPTRY(hipMemcpyAsync(out, ds->dec_out.p, n, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    if (n > out_cap) throw_err(CTOK_E_CAPACITY, "out_cap too small: out_off[n_docs] holds the number of bytes needed");
    if (stats) {
      stats->ms_h2d = h1 - h0;
      stats->ms_d2h = now_ms() - d0;
      stats->ms_total = now_ms() - t0;
    }
  });
}

int ctok_encode_batch(const ctok* tc, const uint8_t* utf8_in, const uint64_t* doc_off, uint64_t n_docs, uint32_t* ids,
                      uint64_t ids_cap, uint64_t* tok_off, const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !doc_off || !tok_off) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    check_host_batch(utf8_in, doc_off, n_docs, "doc_off");
    const uint64_t B = doc_off[n_docs];
    if (ids_cap && !ids) throw_err(CTOK_E_ARG, "null ids");
    std::vector<int> devs;
    if (exec && exec->devices && exec->n_devices > 0) devs.assign(exec->devices, exec->devices + exec->n_devices);
    else devs.push_back(exec ? exec->device : 0);
    const bool timing = exec && (exec->flags & CTOK_F_TIMING);
    const uint64_t chunk = (uint64_t)(exec && exec->chunk_mb ? exec->chunk_mb : 64u) << 20;
    const unsigned hw = usable_cpus_once();
    const unsigned nthr = exec && exec->host_threads ? exec->host_threads
                                                     : std::max(1u, std::min(8u, hw / (unsigned)devs.size()));  // (widening threads: 4 / 8 / 16 within run-to-run noise on C2, profiles/r03/v22_e2e_probe.txt, v27_*; 8 + the pipeline threads stay inside a 16-CPU quota)
    if (stats) *stats = ctok_stats{};
    // shards: contiguous doc ranges balanced by bytes (cut at the first doc start >= k * B / G)
    const size_t G = devs.size();
    std::vector<uint64_t> cut(G + 1, 0);
    for (size_t g = 1; g < G; g++) {
      const uint64_t target = B / G * g;
      cut[g] = (uint64_t)(std::lower_bound(doc_off, doc_off + n_docs, target) - doc_off);
      cut[g] = std::max(cut[g], cut[g - 1]);
    }
    cut[G] = n_docs;
    // output placement: shard g writes its ids at region[g] of the caller's buffer, sized for
    // ids <= bytes + docs (true unless NFC grows the text or a prefix space is added) when the
    // regions fit, else into a private buffer; a shard that outgrows its region runs again
    std::vector<uint64_t> region(G + 1, 0);
    for (size_t g = 0; g < G; g++)
      region[g + 1] = region[g] + (doc_off[cut[g + 1]] - doc_off[cut[g]]) + (cut[g + 1] - cut[g]);
    std::vector<std::unique_ptr<uint32_t[]>> priv(G);
    std::vector<RangeOut> res(G);
    std::vector<ctok_stats> sst(G);
    // one pass over all shards; in_place: shard g writes at region[g] of the caller's ids, else
    // into priv[g] of priv_size[g] ids
    auto attempt = [&](bool in_place, const std::vector<uint64_t>& priv_size) {
      auto shard = [&](size_t g) {
        DeviceCall dc(t, devs[g]);
        uint32_t* out = ids;
        uint64_t cap = ids_cap;
        if (G > 1) {
          if (in_place) {
            out = ids + region[g];
            cap = region[g + 1] - region[g];
          } else {
            priv[g].reset(new uint32_t[priv_size[g] + 1]);  // no zero fill: ids[0, ntok) are written
            out = priv[g].get();
            cap = priv_size[g] + 1;
          }
        }
        sst[g] = ctok_stats{};
        res[g] = encode_host_range(t, dc.ds, utf8_in, doc_off, cut[g], cut[g + 1], out, cap, tok_off + cut[g], chunk,
                                   nthr, timing, stats ? &sst[g] : nullptr);
      };
      if (G == 1) return shard(0);
      std::vector<CatchThread> th(G);
      for (size_t g = 0; g < G; g++) th[g].start([&, g] { shard(g); });
      for (auto& x : th) x.join();  // the error of the lowest shard (the vector's destructor joins the rest)
    };
    tok_off[0] = 0;
    bool in_place = G == 1 || region[G] <= ids_cap;
    {
      std::vector<uint64_t> sz(G);
      for (size_t g = 0; g < G; g++) sz[g] = region[g + 1] - region[g];
      attempt(in_place, sz);
    }
    uint64_t total = 0;
    bool overflow = false;
    for (size_t g = 0; g < G; g++) total += res[g].ntok, overflow |= res[g].overflow;
    if (G > 1 && overflow && total <= ids_cap) {
      // a shard outgrew its id bound region (NFC growth): again, into private buffers of the
      // now known sizes
      std::vector<uint64_t> sz(G);
      for (size_t g = 0; g < G; g++) sz[g] = res[g].ntok;
      in_place = false;
      attempt(false, sz);
    }
    if (G > 1) {
      // rebase: tok_off of shard g gets the ids of shards < g added; its ids move from
      // region[g] (or priv[g]) to that base.  In place, the regions start at or after their
      // destinations, so moving in shard order never overwrites ids not yet moved.
      uint64_t basev = 0;
      for (size_t g = 0; g < G; g++) {
        const uint64_t n = res[g].ntok;
        if (g > 0)
          for (uint64_t d = cut[g] + 1; d <= cut[g + 1]; d++) tok_off[d] += basev;
        if (total <= ids_cap && n) {
          if (in_place) {
            if (region[g] != basev) std::memmove(ids + basev, ids + region[g], n * 4);
          } else {
            std::memcpy(ids + basev, priv[g].get(), n * 4);
          }
        }
        basev += n;
      }
    }
    tok_off[n_docs] = total;
    if (total > ids_cap) throw_err(CTOK_E_CAPACITY, "ids_cap too small: tok_off[n_docs] holds the number of ids needed");
    if (stats) {
      for (size_t g = 0; g < G; g++) {
        const ctok_stats& q = sst[g];
        stats->pieces += q.pieces, stats->long_pieces += q.long_pieces, stats->nfc_docs += q.nfc_docs;
        stats->long_rounds += q.long_rounds;
        stats->workspace_bytes += q.workspace_bytes;  // (shards on one device report it once each)
        stats->bytes_norm += q.bytes_norm;
        for (int c = 0; c < kNumClasses; c++)
          stats->class_bytes[c] += q.class_bytes[c], stats->class_ids[c] += q.class_ids[c];
        // device times: the slowest shard
        stats->ms_device = std::max(stats->ms_device, q.ms_device);
        stats->ms_pretok = std::max(stats->ms_pretok, q.ms_pretok);
        stats->ms_segment = std::max(stats->ms_segment, q.ms_segment);
        stats->ms_bpe_short = std::max(stats->ms_bpe_short, q.ms_bpe_short);
        stats->ms_bpe_lo = std::max(stats->ms_bpe_lo, q.ms_bpe_lo);
        stats->ms_bpe_hi = std::max(stats->ms_bpe_hi, q.ms_bpe_hi);
        stats->ms_bpe_med = std::max(stats->ms_bpe_med, q.ms_bpe_med);
        stats->ms_bpe_long = std::max(stats->ms_bpe_long, q.ms_bpe_long);
        stats->ms_emit = std::max(stats->ms_emit, q.ms_emit);
        stats->ms_h2d = std::max(stats->ms_h2d, q.ms_h2d);
        stats->ms_d2h = std::max(stats->ms_d2h, q.ms_d2h);
      }
      stats->bytes_in = B;
      stats->docs = n_docs;
      stats->tokens = total;
      stats->ms_total = now_ms() - t0;
    }
  });
}

// The front of the padded and the windowed encode: the batch encoded into pad_ids / pad_tokoff,
// the sorted special ids and the zeroed counters on the device, and the rows described in a
// PadWork (outputs, width and row_len are the caller's to fill)
static PadWork pad_front(ctok* t, DeviceState* ds, hipStream_t s, bool timing, const uint8_t* d_utf8,
                         const uint64_t* d_doc_off, uint64_t n_docs, uint64_t n_bytes, const ctok_pad_opts* o,
                         uint64_t rows, ctok_stats* st) {
  const uint32_t f = o->flags;
  const bool pairs = f & CTOK_P_PAIRS;
  const bool add_special = f & CTOK_P_ADD_SPECIAL;
  // 1. encode (encode_to_encoding flavour: no added-token split)
  const uint64_t cap_ids = ctok_ids_bound(t, n_bytes, n_docs);
  ds->pad_ids.ensure(cap_ids);
  ds->pad_tokoff.ensure(n_docs + 1);
  EncodeCall call;
  call.text = d_utf8, call.doc_off = d_doc_off, call.n_docs = n_docs, call.n_bytes = n_bytes;
  call.ids = ds->pad_ids.p, call.ids_cap = ds->pad_ids.cap, call.tok_off = ds->pad_tokoff.p;
  call.stream = s, call.timing = timing, call.stats = st;
  call.split_added = !add_special;
  encode_device(t, ds, call);
  // 2. row lengths and the longest row
  std::vector<uint32_t> sp;
  for (const auto& e : t->special) sp.push_back(e.second);
  std::sort(sp.begin(), sp.end());
  sp.erase(std::unique(sp.begin(), sp.end()), sp.end());
  ds->pad_special.ensure(sp.size() + 1);
  if (!sp.empty()) HIPTRY(hipMemcpyAsync(ds->pad_special.p, sp.data(), sp.size() * 4, hipMemcpyHostToDevice, s));
  ds->pad_ctr.ensure(4);
  HIPTRY(hipMemsetAsync(ds->pad_ctr.p, 0, 16, s));
  PadWork w{};
  w.ids = ds->pad_ids.p;
  w.tok_off = ds->pad_tokoff.p;
  w.n_rows = (uint32_t)rows;
  w.pairs = pairs ? 1 : 0;
  w.use_tpl = (add_special && t->has_pp && !(f & CTOK_P_NO_POSTPROCESS)) ? 1 : 0;
  w.n_items = w.use_tpl ? (uint32_t)t->pp_items.size() : 0;
  for (uint32_t k = 0; k < w.n_items; k++) w.items[k] = t->pp_items[k];
  w.mark = (add_special && !(f & CTOK_P_NO_POSTPROCESS)) ? 1 : 0;
  w.special_ids = ds->pad_special.p;
  w.n_special = (uint32_t)sp.size();
  w.truncate = (f & CTOK_P_TRUNCATE) ? 1 : 0;
  w.max_len = o->max_length;
  w.target = 0;
  if (f & CTOK_P_PAD_TO_MAX) w.target = o->max_length;
  w.pad_left = (f & CTOK_P_PAD_LEFT) ? 1 : 0;
  w.pad_id = (f & CTOK_P_PAD_ID) ? o->pad_id : ctok_pad_id(t);
  w.counters = ds->pad_ctr.p;
  return w;
}

// rows of a padded call's batch, and the checks on its options that need no device
static uint64_t pad_rows_of(const ctok* t, const ctok_pad_opts* o, uint64_t n_docs) {
  const bool pairs = o->flags & CTOK_P_PAIRS;
  if (pairs && (n_docs & 1)) throw_err(CTOK_E_ARG, "CTOK_P_PAIRS needs an even number of documents");
  const uint64_t rows = pairs ? n_docs / 2 : n_docs;
  if (rows >= 0xFFFFFFFFull) throw_err(CTOK_E_ARG, "too many rows");
  if ((o->flags & CTOK_P_ADD_SPECIAL) && t->pp_items.size() > (size_t)kPadMaxItems)
    throw_err(CTOK_E_UNSUPPORTED, "post-processor template with more than 16 items");
  return rows;
}

int ctok_encode_padded_device(const ctok* tc, const uint8_t* d_utf8, const uint64_t* d_doc_off, uint64_t n_docs,
                              uint64_t n_bytes, const ctok_pad_opts* o, uint32_t* d_ids, uint32_t* d_attn,
                              uint32_t* d_type, uint32_t* d_special, uint64_t cap, uint64_t* d_row_len,
                              uint64_t* width_out, const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !o || !d_doc_off || !d_row_len || !width_out || (n_bytes && !d_utf8))
    return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    const uint32_t f = o->flags;
    const uint64_t rows = pad_rows_of(t, o, n_docs);
    check_device_text(d_utf8, n_bytes);
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    ctok_stats st{};
    PadWork w = pad_front(t, ds, s, dc.timing, d_utf8, d_doc_off, n_docs, n_bytes, o, rows, &st);
    w.row_len = d_row_len;
    HIPTRY(launch_pad_len(w, s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, ds->pad_ctr.p, 16, hipMemcpyDeviceToHost, s));
    spin_sync(ds, s);
    const uint64_t longest = pinned<uint64_t>(ds, kPinScratch)[0];
    const uint32_t dropped = pinned<uint32_t>(ds, kPinScratch)[2];
    if (w.use_tpl && dropped)
      throw_err(CTOK_E_PANIC, "attempt to subtract with overflow: the post-processor template drops ids (reference src/huggingface/mod.rs:378)");
    if ((f & CTOK_P_PAD_LONGEST) && !(f & CTOK_P_PAD_TO_MAX)) {
      w.target = longest;  // every row padded to the longest: row_len again
      HIPTRY(launch_pad_len(w, s));
    }
    const uint64_t width = std::max<uint64_t>(longest, w.target);
    *width_out = width;
    w.width = width;
    if (rows * width > cap) {
      HIPTRY(hipStreamSynchronize(s));
      throw_err(CTOK_E_CAPACITY, "cap too small: *width_out holds the row width needed");
    }
    if (rows * width && !d_ids) throw_err(CTOK_E_ARG, "null ids");
    w.out_ids = d_ids;
    w.out_attn = d_attn;
    w.out_type = d_type;
    w.out_special = d_special;
    HIPTRY(launch_pad_rows(w, s));
    spin_sync(ds, s);
    if (stats) {
      *stats = st;
      stats->ms_total = now_ms() - t0;
    }
  });
}

int ctok_encode_padded(const ctok* tc, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                       const ctok_pad_opts* o, uint32_t* ids, uint32_t* attn, uint32_t* type, uint32_t* special,
                       uint64_t cap, uint64_t* row_len, uint64_t* width_out, const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !o || !doc_off || !row_len || !width_out) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    check_host_batch(utf8, doc_off, n_docs, "doc_off");
    const uint64_t B = doc_off[n_docs];
    const uint64_t rows = (o->flags & CTOK_P_PAIRS) ? n_docs / 2 : n_docs;
    // held from staging to readback: another thread's call on this device cannot overwrite the
    // staged inputs or the outputs in between (the nested device call locks again, recursively)
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    ds->pad_rowlen.ensure(rows + 1);
    for (auto& b : ds->pad_out) b.ensure(cap ? cap : 1);
    stage_host_batch(ds, utf8, doc_off, n_docs, s);
    ctok_exec ex = exec ? *exec : ctok_exec{};
    ex.stream = s;
    uint64_t width = 0;
    const int rc = ctok_encode_padded_device(t, ds->pad_in_text.p, ds->pad_in_off.p, n_docs, B, o, ds->pad_out[0].p,
                                             attn ? ds->pad_out[1].p : nullptr, type ? ds->pad_out[2].p : nullptr,
                                             special ? ds->pad_out[3].p : nullptr, cap, ds->pad_rowlen.p, &width, &ex,
                                             stats);
    *width_out = width;
    if (rc != CTOK_OK && rc != CTOK_E_CAPACITY) throw_err(rc, g_err);
    HIPTRY(hipMemcpyAsync(row_len, ds->pad_rowlen.p, rows * 8, hipMemcpyDeviceToHost, s));
    if (rc == CTOK_OK && rows * width) {
      const size_t nb = rows * width * 4;
      HIPTRY(hipMemcpyAsync(ids, ds->pad_out[0].p, nb, hipMemcpyDeviceToHost, s));
      if (attn) HIPTRY(hipMemcpyAsync(attn, ds->pad_out[1].p, nb, hipMemcpyDeviceToHost, s));
      if (type) HIPTRY(hipMemcpyAsync(type, ds->pad_out[2].p, nb, hipMemcpyDeviceToHost, s));
      if (special) HIPTRY(hipMemcpyAsync(special, ds->pad_out[3].p, nb, hipMemcpyDeviceToHost, s));
    }
    HIPTRY(hipStreamSynchronize(s));
    if (rc == CTOK_E_CAPACITY) throw_err(CTOK_E_CAPACITY, "cap too small: *width_out holds the row width needed");
  });
}

// The window calls' checks that need no device: the reference's loop never ends with stride >= max_length
static void check_window_opts(const ctok_pad_opts* o, uint64_t stride) {
  if (!win::valid(o->max_length, stride))
    throw_err(CTOK_E_ARG, "stride must be smaller than max_length (the reference's truncate_with_stride never ends)");
}

static const char* const kWinCapacityMsg =
    "cap or win_cap too small: *n_windows_out and *width_out hold the windows and the row width needed";

// Overflowing stride windows (Encoding::truncate_with_stride, src/encoding.rs:175-223): the padded
// encode's rows, each cut into its windows on the device (pad.hip k_win_len, scan, k_win_rows).
int ctok_encode_windows_device(const ctok* tc, const uint8_t* d_utf8, const uint64_t* d_doc_off, uint64_t n_docs,
                               uint64_t n_bytes, const ctok_pad_opts* o, uint64_t stride, uint32_t* d_ids,
                               uint32_t* d_attn, uint32_t* d_type, uint32_t* d_special, uint64_t cap,
                               uint64_t* d_win_len, uint32_t* d_win_row, uint64_t* d_win_start, uint64_t win_cap,
                               uint64_t* d_row_win, uint64_t* n_windows_out, uint64_t* width_out,
                               const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !o || !d_doc_off || !d_row_win || !n_windows_out || !width_out || (n_bytes && !d_utf8))
    return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    double t0 = now_ms();
    check_window_opts(o, stride);
    ctok_pad_opts po = *o;
    po.flags |= CTOK_P_TRUNCATE | CTOK_P_WINDOWS;
    const uint32_t f = po.flags;
    const uint64_t rows = pad_rows_of(t, &po, n_docs);
    check_device_text(d_utf8, n_bytes);
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    ctok_stats st{};
    WinWork w{};
    w.p = pad_front(t, ds, s, dc.timing, d_utf8, d_doc_off, n_docs, n_bytes, &po, rows, &st);
    w.stride = stride;
    w.row_win = d_row_win;
    // Encoding::from_ids rows: added-token ids without a vocab string leave `tokens` short (k_win_tokens)
    std::vector<uint32_t> tokenless;
    if (!(f & CTOK_P_ADD_SPECIAL))
      for (uint32_t id : t->at_id)
        if (!t->id_to_token.count(id)) tokenless.push_back(id);
    std::sort(tokenless.begin(), tokenless.end());
    tokenless.erase(std::unique(tokenless.begin(), tokenless.end()), tokenless.end());
    if (!tokenless.empty()) {
      ds->win_tokenless.ensure(tokenless.size());
      HIPTRY(hipMemcpyAsync(ds->win_tokenless.p, tokenless.data(), tokenless.size() * 4, hipMemcpyHostToDevice, s));
      w.tokenless = ds->win_tokenless.p;
      w.n_tokenless = (uint32_t)tokenless.size();
      w.ids_bound = ctok_ids_bound(t, n_bytes, n_docs);
    }
    // windows per row, scanned into each row's first window; the total at [rows]
    HIPTRY(launch_win_len(w, s));
    ds->scan_tmp.ensure(scan_tmp_elems(rows + 1) + 64);
    HIPTRY(scan_u64(d_row_win, rows, ds->scan_tmp.p, ds->scan_tmp.cap, s));
    // one readback: the longest main window and the flags, then the total
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch, ds->pad_ctr.p, 16, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(ds->host + kPinScratch + 2, d_row_win + rows, 8, hipMemcpyDeviceToHost, s));
    spin_sync(ds, s);
    const uint64_t longest = pinned<uint64_t>(ds, kPinScratch)[0];
    const uint32_t dropped = pinned<uint32_t>(ds, kPinScratch)[2];
    const uint32_t unsliceable = pinned<uint32_t>(ds, kPinScratch)[3];
    const uint64_t n_windows = pinned<uint64_t>(ds, kPinScratch)[2];
    if (w.p.use_tpl && dropped)
      throw_err(CTOK_E_PANIC, "attempt to subtract with overflow: the post-processor template drops ids (reference src/huggingface/mod.rs:378)");
    if (unsliceable)
      throw_err(CTOK_E_PANIC, "range end index out of range for slice: a row longer than max_length has fewer tokens than ids -- the post-processor does not extend `tokens`, and without special tokens ids that have no vocab string are left out (reference src/encoding.rs:189)");
    if (n_windows >= 0xFFFFFFFFull) throw_err(CTOK_E_ARG, "too many windows (the call is limited to < 2^32); split the batch");
    // padding as Tokenizer.__call__: window 0 of each row to the longest main window or to max_length
    if ((f & CTOK_P_PAD_LONGEST) && !(f & CTOK_P_PAD_TO_MAX)) w.p.target = longest;
    const uint64_t width = std::max<uint64_t>(longest, w.p.target);
    *n_windows_out = n_windows;
    *width_out = width;
    w.n_windows = n_windows;
    w.p.width = width;
    if (n_windows > win_cap || (width && n_windows > cap / width)) throw_err(CTOK_E_CAPACITY, kWinCapacityMsg);
    if (n_windows && (!d_win_len || !d_win_row)) throw_err(CTOK_E_ARG, "null window records");
    if (n_windows * width && !d_ids) throw_err(CTOK_E_ARG, "null ids");
    w.p.out_ids = d_ids;
    w.p.out_attn = d_attn;
    w.p.out_type = d_type;
    w.p.out_special = d_special;
    w.win_len = d_win_len;
    w.win_row = d_win_row;
    w.win_start = d_win_start;
    HIPTRY(launch_win_rows(w, s));
    spin_sync(ds, s);
    if (stats) {
      *stats = st;
      stats->ms_total = now_ms() - t0;
    }
  });
}

int ctok_encode_windows(const ctok* tc, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                        const ctok_pad_opts* o, uint64_t stride, uint32_t* ids, uint32_t* attn, uint32_t* type,
                        uint32_t* special, uint64_t cap, uint64_t* win_len, uint32_t* win_row, uint64_t* win_start,
                        uint64_t win_cap, uint64_t* row_win, uint64_t* n_windows_out, uint64_t* width_out,
                        const ctok_exec* exec, ctok_stats* stats) {
  if (!tc || !o || !doc_off || !row_win || !n_windows_out || !width_out) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    check_window_opts(o, stride);
    check_host_batch(utf8, doc_off, n_docs, "doc_off");
    const uint64_t B = doc_off[n_docs];
    const uint64_t rows = (o->flags & CTOK_P_PAIRS) ? n_docs / 2 : n_docs;
    // held from staging to readback, as in ctok_encode_padded
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    ds->win_rowwin.ensure(rows + 1);
    for (auto& b : ds->pad_out) b.ensure(cap ? cap : 1);
    ds->win_len.ensure(win_cap ? win_cap : 1);
    ds->win_row.ensure(win_cap ? win_cap : 1);
    ds->win_start.ensure(win_cap ? win_cap : 1);
    stage_host_batch(ds, utf8, doc_off, n_docs, s);
    ctok_exec ex = exec ? *exec : ctok_exec{};
    ex.stream = s;
    uint64_t n_windows = 0, width = 0;
    const int rc = ctok_encode_windows_device(
        t, ds->pad_in_text.p, ds->pad_in_off.p, n_docs, B, o, stride, ds->pad_out[0].p, attn ? ds->pad_out[1].p : nullptr,
        type ? ds->pad_out[2].p : nullptr, special ? ds->pad_out[3].p : nullptr, cap, ds->win_len.p, ds->win_row.p,
        win_start ? ds->win_start.p : nullptr, win_cap, ds->win_rowwin.p, &n_windows, &width, &ex, stats);
    *n_windows_out = n_windows;
    *width_out = width;
    if (rc != CTOK_OK && rc != CTOK_E_CAPACITY) throw_err(rc, g_err);
    HIPTRY(hipMemcpyAsync(row_win, ds->win_rowwin.p, (rows + 1) * 8, hipMemcpyDeviceToHost, s));
    if (rc == CTOK_OK && n_windows) {
      if (!win_len || !win_row) throw_err(CTOK_E_ARG, "null window records");
      HIPTRY(hipMemcpyAsync(win_len, ds->win_len.p, n_windows * 8, hipMemcpyDeviceToHost, s));
      HIPTRY(hipMemcpyAsync(win_row, ds->win_row.p, n_windows * 4, hipMemcpyDeviceToHost, s));
      if (win_start) HIPTRY(hipMemcpyAsync(win_start, ds->win_start.p, n_windows * 8, hipMemcpyDeviceToHost, s));
    }
    if (rc == CTOK_OK && n_windows * width) {
      if (!ids) throw_err(CTOK_E_ARG, "null ids");
      const size_t nb = n_windows * width * 4;
      HIPTRY(hipMemcpyAsync(ids, ds->pad_out[0].p, nb, hipMemcpyDeviceToHost, s));
      if (attn) HIPTRY(hipMemcpyAsync(attn, ds->pad_out[1].p, nb, hipMemcpyDeviceToHost, s));
      if (type) HIPTRY(hipMemcpyAsync(type, ds->pad_out[2].p, nb, hipMemcpyDeviceToHost, s));
      if (special) HIPTRY(hipMemcpyAsync(special, ds->pad_out[3].p, nb, hipMemcpyDeviceToHost, s));
    }
    HIPTRY(hipStreamSynchronize(s));
    if (rc == CTOK_E_CAPACITY) throw_err(CTOK_E_CAPACITY, kWinCapacityMsg);
  });
}

// Offsets and word ids of encode_to_encoding (src/huggingface/mod.rs:395-480).  The ids and the
// piece starts (the pre-tokenizer's words) come from the GPU encode; the walk that places each
// word in the original text by str::find and each token inside its word is a sequential host
// pass per document, as in the reference.  A word's ids are its piece's ids on the device (k_emit
// leaves every piece's first id for this call), not a sum of token string lengths: with the
// rank-shift quirk (src/bpe.rs:60-69) an id's token string need not be its piece's bytes.
int ctok_encode_offsets(const ctok* tc, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                        uint32_t* ids, uint64_t* offsets, uint32_t* word_ids, uint64_t cap, uint64_t* tok_off,
                        const ctok_exec* exec) {
  if (!tc || !doc_off || !tok_off) return fail(CTOK_E_ARG, "null argument");
  ctok* t = const_cast<ctok*>(tc);
  return run([&] {
    check_host_batch(utf8, doc_off, n_docs, "doc_off");
    const uint64_t n_in = doc_off[n_docs];
    DeviceCall dc(t, exec);
    DeviceState* ds = dc.ds;
    hipStream_t s = dc.s;
    stage_host_batch(ds, utf8, doc_off, n_docs, s);
    ds->pad_ids.ensure(ctok_ids_bound(t, n_in, n_docs));
    ds->pad_tokoff.ensure(n_docs + 1);
    EncodeCall call;
    call.text = ds->pad_in_text.p, call.doc_off = ds->pad_in_off.p, call.n_docs = n_docs, call.n_bytes = n_in;
    call.ids = ds->pad_ids.p, call.ids_cap = ds->pad_ids.cap, call.tok_off = ds->pad_tokoff.p;
    call.stream = s;
    call.split_added = false;
    call.mode = EncodeMode::KeepFirst;
    const uint64_t ntok = encode_device(t, ds, call);
    const uint64_t B = ds->last_B;
    const bool norm = ds->last_norm;
    // each piece's first id: tile_tok[tile] (scanned) + tcnt[tile][j] (k_emit with keep_first)
    const uint64_t n_tiles = (B + kTile - 1) / kTile;
    std::vector<uint32_t> hid(ntok), pb((B + 31) / 32), pfirst(n_tiles * kTileSlots), tfirst(n_tiles + 1);
    std::vector<uint64_t> toff(n_docs + 1), noff;
    std::vector<uint8_t> ntext;
    HIPTRY(hipMemcpyAsync(toff.data(), ds->pad_tokoff.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    if (ntok) HIPTRY(hipMemcpyAsync(hid.data(), ds->pad_ids.p, ntok * 4, hipMemcpyDeviceToHost, s));
    if (!pb.empty()) HIPTRY(hipMemcpyAsync(pb.data(), ds->pbits.p, pb.size() * 4, hipMemcpyDeviceToHost, s));
    if (n_tiles) {
      HIPTRY(hipMemcpyAsync(pfirst.data(), ds->tcnt.p, pfirst.size() * 4, hipMemcpyDeviceToHost, s));
      HIPTRY(hipMemcpyAsync(tfirst.data(), ds->tile_tok.p, tfirst.size() * 4, hipMemcpyDeviceToHost, s));
    }
    if (norm) {
      ntext.resize(B + 1);
      noff.resize(n_docs + 1);
      if (B) HIPTRY(hipMemcpyAsync(ntext.data(), ds->norm_text.p, B, hipMemcpyDeviceToHost, s));
      HIPTRY(hipMemcpyAsync(noff.data(), ds->norm_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    HIPTRY(hipStreamSynchronize(s));
    for (uint64_t d = 0; d <= n_docs; d++) tok_off[d] = toff[d];
    if (ntok > cap) throw_err(CTOK_E_CAPACITY, "cap too small: tok_off[n_docs] holds the number of ids needed");
    if (ntok && (!ids || !offsets || !word_ids)) throw_err(CTOK_E_ARG, "null output");
    std::memcpy(ids, hid.data(), ntok * 4);
    // bytes_to_unicode (src/pretokenizers.rs:130-153): the UTF-8 of each byte's char
    std::string benc[256];
    {
      int n = 0;
      for (int b = 0; b < 256; b++) {
        const bool keep = (b >= 0x21 && b <= 0x7E) || (b >= 0xA1 && b <= 0xAC) || (b >= 0xAE && b <= 0xFF);
        const std::vector<uint32_t> cp{keep ? (uint32_t)b : 256u + (uint32_t)n++};
        benc[b] = encode_utf8(cp, 0, 1);
      }
    }
    auto is_start = [&](uint64_t g) { return (pb[g >> 5] >> (g & 31)) & 1u; };
    // first id of the piece starting at byte g, the j-th piece of its tile
    auto first_id = [&](uint64_t g, uint32_t j) { return (uint64_t)tfirst[g / kTile] + pfirst[(g / kTile) * kTileSlots + j]; };
    // documents are independent: contiguous ranges over host threads, each with its own cache
    auto walk = [&](uint64_t d_begin, uint64_t d_end) {
    std::unordered_map<uint32_t, std::pair<uint32_t, uint32_t>> tlen;  // id -> (bytes, chars) of its token string
    auto token_len = [&](uint32_t id) {
      auto it = tlen.find(id);
      if (it != tlen.end()) return it->second;
      auto jt = t->id_to_token.find(id);
      uint32_t nb = 0, nc = 0;
      if (jt != t->id_to_token.end()) {
        nb = (uint32_t)jt->second.size();
        for (unsigned char c : jt->second) nc += (c & 0xC0) != 0x80;
      }
      return tlen.emplace(id, std::make_pair(nb, nc)).first->second;
    };
    std::string word;
    uint64_t jpos = ~0ull;  // the next piece's start and its index in its tile
    uint32_t jcur = 0;
    for (uint64_t d = d_begin; d < d_end; d++) {
      const uint8_t* o = utf8 + doc_off[d];
      const uint64_t olen = doc_off[d + 1] - doc_off[d];
      const uint64_t g0 = norm ? noff[d] : doc_off[d], g1 = norm ? noff[d + 1] : doc_off[d + 1];
      const uint8_t* nt = norm ? ntext.data() + g0 : o;
      const std::string_view orig((const char*)o, olen);
      uint64_t search = 0, k = toff[d], widx = 0;
      // j: the piece's index within its tile (pieces start in text order; a tile's first piece is
      // 0), carried over from the previous document's last piece
      uint32_t j = 0;
      if (g0 < g1) {
        if (jpos == g0) j = jcur;
        else
          for (uint64_t x = (g0 / kTile) * kTile; x < g0; x++) j += is_start(x);
      }
      for (uint64_t p = g0; p < g1;) {
        uint64_t q = p + 1;
        while (q < g1 && !is_start(q)) q++;
        // the piece's ids: up to the next piece's first id (the next doc's first piece, or the end)
        uint64_t nq = q;
        while (nq < B && !is_start(nq)) nq++;
        const uint32_t jn = nq < B && nq / kTile == p / kTile ? j + 1 : 0;
        const uint64_t k_end = nq < B ? first_id(nq, jn) : ntok;
        if (first_id(p, j) != k) throw_err(CTOK_E_DEVICE, "offsets: piece ids out of order");
        word.clear();
        uint64_t kept = 0;  // bytes whose char is in the vocab (the others are dropped, src/bpe.rs:94-97)
        for (uint64_t i = p; i < q; i++) {
          const uint8_t b = nt[i - g0];
          word += benc[b];
          kept += t->byte2id[b] >= 0;
        }
        size_t lead = 0;  // trim_start_matches('Ġ' | '▁')
        while (true) {
          if (word.compare(lead, 2, "\xC4\xA0") == 0) lead += 2;
          else if (word.compare(lead, 3, "\xE2\x96\x81") == 0) lead += 3;
          else break;
        }
        const std::string_view find = lead < word.size() ? std::string_view(word).substr(lead) : std::string_view(word);
        if (search < olen && (o[search] & 0xC0) == 0x80)
          throw_err(CTOK_E_PANIC, "byte index " + std::to_string(search) +
                                      " is not a char boundary (reference src/huggingface/mod.rs:464 slices the text there)");
        const size_t pos = orig.substr(search).find(find);
        uint64_t ws, we;
        if (pos != std::string_view::npos) {
          ws = search + pos;
          we = ws + find.size();
        } else {
          ws = search;
          we = std::min<uint64_t>(ws + word.size(), olen);
        }
        search = we;
        uint64_t at = ws;
        (void)kept;
        if (k_end > toff[d + 1]) throw_err(CTOK_E_DEVICE, "offsets: ids and words disagree");
        for (; k < k_end; k++) {
          const auto L = token_len(hid[k]);
          const uint64_t e = std::min<uint64_t>(at + L.first, we);
          offsets[2 * k] = at;
          offsets[2 * k + 1] = e;
          word_ids[k] = (uint32_t)widx;
          at = e;
        }
        widx++;
        p = q;
        j = jn;
        jpos = nq;
        jcur = jn;
      }
      if (k != toff[d + 1]) throw_err(CTOK_E_DEVICE, "offsets: ids and words disagree");
    }
    };
    const unsigned nth = n_docs < 256 ? 1u : std::min(16u, usable_cpus_once());
    std::vector<CatchThread> th(nth - 1);  // (the last range runs here)
    for (unsigned w = 0; w + 1 < nth; w++) {
      const uint64_t a = n_docs * w / nth, b = n_docs * (w + 1) / nth;
      th[w].start([&, a, b] { walk(a, b); });
    }
    std::exception_ptr last;
    try {
      walk(n_docs * (nth - 1) / nth, n_docs);
    } catch (...) {
      last = std::current_exception();
    }
    for (auto& x : th) x.join();  // the error of the lowest document range
    if (last) std::rethrow_exception(last);
  });
}

}  // extern "C"
