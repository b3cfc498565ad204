// Host runtime of the Normalizer behind include/ctok_normalizer.h.
//
// Reference: Normalizer::normalize, src/normalizers.rs:43-202 (Complexity-ML/complexity-tokenizer
// v0.3.3).  A normaliser is expanded once into primitive steps (normalize_prog.h); a run takes the
// whole batch through them on the device, one step after the other:
//   count (normalize.hip k_nz_count; Strip and Replace first make what their units read), the
//   `changed` word and, when set, scan_u64 and the total come back to the host, which refuses 4 GiB
//   and grows the other of the handle's two text buffers to exactly total + 16 bytes before the write.
// A step that changes nothing leaves the batch where it is.  Lowercase is lower_device
// (lowercase_host.h), which has the same shape.  There is no CPU path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ctok_normalizer.h"
#include "ctok_internal.h"  // ctok_dev::scan_u64, scan_tmp_elems
#include "host_common.h"
#include "lowercase_host.h"
#include "normalize_internal.h"
#include "normalize_prog.h"
#include "train_host_common.h"

using ctok_host::throw_error;
using ctok_train_host::DBuf;
using normalize::kSpan;
using normalize::PrimStep;

namespace {

constexpr uint64_t kRefuseFrom = 1ull << 32;  // a batch of 4 GiB, before or after any step

struct View {  // a batch on the device
  const uint8_t* text;
  const uint64_t* off;
  uint64_t n_bytes;
};

}  // namespace

struct ctok_normalizer {
  int device = 0;
  std::vector<PrimStep> prog;
  // the steps' strings on the device, step i's a at at[2i], its b at at[2i + 1]
  std::string strings;
  std::vector<uint64_t> at;
  DBuf<uint8_t> d_strings;
  bool ready = false;  // d_strings uploaded, stream and events made
  hipStream_t own = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DBuf<uint8_t> buf[2], cand, taken, in_text;
  DBuf<uint64_t> off[2], len, tmp, trim, in_off;
  DBuf<uint32_t> changed;
  ctok_wp::LowerBufs lower;
  std::vector<double> ms;
  ctok_normalizer_info info{};

  ~ctok_normalizer() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own) (void)hipStreamDestroy(own);
  }

  void prepare() {
    HIPT(hipSetDevice(device));
    if (ready) return;
    d_strings.ensure(strings.size() + 16);
    HIPT(hipMemcpy(d_strings.p, strings.data(), strings.size(), hipMemcpyHostToDevice));
    HIPT(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    HIPT(hipEventCreate(&ev0));
    HIPT(hipEventCreate(&ev1));
    ready = true;
  }

  normalize::Step step_of(size_t i) const {
    normalize::Step st{};
    st.kind = prog[i].kind;
    st.a = d_strings.p + at[2 * i];
    st.a_len = (uint32_t)prog[i].a.size();
    st.b = d_strings.p + at[2 * i + 1];
    st.b_len = (uint32_t)prog[i].b.size();
    return st;
  }

  // One primitive step over cur; the result lies in dst (buf[w], off[w]) when the step changed
  // anything, and cur is returned as it is when not.
  View run_step(size_t i, const View& cur, uint64_t n_docs, int w, bool* wrote, hipStream_t s) {
    normalize::Step st = step_of(i);
    const uint64_t nb = cur.n_bytes, n_spans = (nb + kSpan - 1) / kSpan;
    const uint64_t around = normalize::pre_len(st) + normalize::post_len(st);
    *wrote = false;
    if (st.kind == normalize::P_LOWER) {
      if (!nb) return cur;
      View in = cur;
      if (cur.text == lower.out.p) {  // (Lowercase behind Lowercase: lower_device writes where cur lies)
        buf[w].ensure(nb + 16);
        off[w].ensure(n_docs + 1);
        HIPT(hipMemcpyAsync(buf[w].p, cur.text, nb, hipMemcpyDeviceToDevice, s));
        HIPT(hipMemsetAsync(buf[w].p + nb, 0, 16, s));
        HIPT(hipMemcpyAsync(off[w].p, cur.off, (n_docs + 1) * 8, hipMemcpyDeviceToDevice, s));
        in = View{buf[w].p, off[w].p, nb};
        *wrote = true;
      }
      const ctok_wp::Lowered L = ctok_wp::lower_device(lower, in.text, nb, in.off, n_docs, s, kRefuseFrom);
      return View{L.text, L.doc_off, L.n_bytes};
    }
    len.ensure(n_spans + 1);
    changed.ensure(1);
    HIPT(hipMemsetAsync(changed.p, 0, 4, s));
    if (nb) {
      if (st.kind == normalize::P_STRIP) {
        trim.ensure(2 * n_docs);
        HIPT(ctok_nz::launch_trim(cur.text, cur.off, n_docs, trim.p, s));
        st.trim = trim.p;
      }
      if (st.kind == normalize::P_REPLACE) {
        cand.ensure(nb);
        taken.ensure(nb);
        HIPT(ctok_nz::launch_matches(st, cur.text, nb, cur.off, n_docs, cand.p, taken.p, s));
        st.cand = cand.p;
        st.taken = taken.p;
      }
      HIPT(ctok_nz::launch_count(st, cur.text, nb, cur.off, n_docs, len.p, changed.p, s));
    }
    uint32_t ch = 0;
    HIPT(hipMemcpyAsync(&ch, changed.p, 4, hipMemcpyDeviceToHost, s));
    HIPT(hipStreamSynchronize(s));
    if (!ch && !around) return cur;
    uint64_t total = 0;
    if (nb) {
      tmp.ensure(ctok_dev::scan_tmp_elems(n_spans + 1) + 64);
      HIPT(ctok_dev::scan_u64(len.p, n_spans, tmp.p, tmp.cap, s));  // len[n_spans] = the total
      HIPT(hipMemcpyAsync(&total, len.p + n_spans, 8, hipMemcpyDeviceToHost, s));
      HIPT(hipStreamSynchronize(s));
    } else {
      HIPT(hipMemsetAsync(len.p, 0, 8, s));
    }
    if (total >= kRefuseFrom || n_docs >= kRefuseFrom || total + n_docs * around >= kRefuseFrom)
      throw_error(CTOK_E_CAPACITY, std::string("normalizer: the output of step ") + std::to_string(i) + " (" +
                                       normalize::prim_name(st.kind) + ") reaches 4 GiB");
    total += n_docs * around;
    buf[w].ensure(total + 16);
    off[w].ensure(n_docs + 1);
    HIPT(hipMemsetAsync(buf[w].p + total, 0, 16, s));
    HIPT(ctok_nz::launch_write(st, cur.text, nb, cur.off, n_docs, len.p, buf[w].p, off[w].p, s));
    *wrote = true;
    return View{buf[w].p, off[w].p, total};
  }

  // the whole program over n_docs > 0 texts; the result is valid until the handle's next run
  View run_steps(const View& in, uint64_t n_docs, hipStream_t s) {
    if (in.n_bytes >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "normalizer: the input reaches 4 GiB");
    info = ctok_normalizer_info{};
    info.steps = prog.size();
    info.bytes_in = info.bytes_peak = in.n_bytes;
    ms.assign(prog.size(), 0.0);
    View cur = in;
    int w = 0;
    for (size_t i = 0; i < prog.size(); i++) {
      HIPT(hipEventRecord(ev0, s));
      bool wrote = false;
      const View next = run_step(i, cur, n_docs, w, &wrote, s);
      if (wrote) w ^= 1;  // (the other buffer next: the step after reads this one)
      if (next.text != cur.text) info.steps_changed++;
      cur = next;
      if (cur.n_bytes > info.bytes_peak) info.bytes_peak = cur.n_bytes;
      HIPT(hipEventRecord(ev1, s));
      HIPT(hipEventSynchronize(ev1));
      float t = 0;
      HIPT(hipEventElapsedTime(&t, ev0, ev1));
      ms[i] = t;
    }
    info.bytes_out = cur.n_bytes;
    return cur;
  }
};

namespace {

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

extern "C" {

int ctok_normalizer_create(const ctok_norm_step* steps, uint64_t n_steps, int device, ctok_normalizer** out) {
  return ctok_host::run_guarded([&] {
    if (!out || (n_steps && !steps)) throw_error(CTOK_E_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<ctok_normalizer> nz(new ctok_normalizer);
    nz->device = device;
    for (uint64_t i = 0; i < n_steps; i++) {
      const ctok_norm_step& st = steps[i];
      if ((st.a_len && !st.a) || (st.b_len && !st.b)) throw_error(CTOK_E_ARG, "null argument");
      const char* err = normalize::expand(st.kind, st.flags, std::string((const char*)st.a, st.a_len),
                                          std::string((const char*)st.b, st.b_len), nz->prog);
      if (err) throw_error(CTOK_E_ARG, std::string("normalizer step ") + std::to_string(i) + ": " + err);
      if (nz->prog.size() > CTOK_NORM_MAX_STEPS)
        throw_error(CTOK_E_UNSUPPORTED, "normalizer: more than " + std::to_string(CTOK_NORM_MAX_STEPS) + " primitive steps");
    }
    for (const PrimStep& ps : nz->prog) {
      nz->at.push_back(nz->strings.size());
      nz->strings += ps.a;
      nz->at.push_back(nz->strings.size());
      nz->strings += ps.b;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
      (void)hipGetLastError();
      throw_error(CTOK_E_DEVICE, "normalizer: no HIP device " + std::to_string(device));
    }
    *out = nz.release();
  });
}

void ctok_normalizer_destroy(ctok_normalizer* nz) { delete nz; }

int ctok_normalizer_run(ctok_normalizer* nz, const uint8_t* utf8, const uint64_t* off, uint64_t n_texts, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_off) {
  return ctok_host::run_guarded([&] {
    if (!nz || !out_off || (n_texts && (!off || (off[n_texts] && !utf8)))) throw_error(CTOK_E_ARG, "null argument");
    out_off[0] = 0;
    if (!n_texts) return;
    check_utf8(utf8, off, n_texts);
    const uint64_t nb = off[n_texts];
    if (nb >= kRefuseFrom) throw_error(CTOK_E_CAPACITY, "normalizer: the input reaches 4 GiB");
    nz->prepare();
    hipStream_t s = nz->own;
    nz->in_text.ensure(nb + 16);
    nz->in_off.ensure(n_texts + 1);
    if (nb) HIPT(hipMemcpyAsync(nz->in_text.p, utf8, nb, hipMemcpyHostToDevice, s));
    HIPT(hipMemsetAsync(nz->in_text.p + nb, 0, 16, s));
    HIPT(hipMemcpyAsync(nz->in_off.p, off, (n_texts + 1) * 8, hipMemcpyHostToDevice, s));
    const View r = nz->run_steps(View{nz->in_text.p, nz->in_off.p, nb}, n_texts, s);
    HIPT(hipMemcpyAsync(out_off, r.off, (n_texts + 1) * 8, hipMemcpyDeviceToHost, s));
    if (r.n_bytes <= out_cap && r.n_bytes) {
      if (!out) throw_error(CTOK_E_ARG, "null argument");
      HIPT(hipMemcpyAsync(out, r.text, r.n_bytes, hipMemcpyDeviceToHost, s));
    }
    HIPT(hipStreamSynchronize(s));
    if (r.n_bytes > out_cap)
      throw_error(CTOK_E_CAPACITY, "ctok_normalizer_run: the output needs " + std::to_string(r.n_bytes) + " bytes");
  });
}

int ctok_normalizer_run_device(ctok_normalizer* nz, const uint8_t* d_utf8, const uint64_t* d_off, uint64_t n_texts,
                               uint64_t n_bytes, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                               uint64_t* n_bytes_out, void* stream) {
  return ctok_host::run_guarded([&] {
    if (!nz || !d_out_off || !n_bytes_out || (n_texts && !d_off) || (n_bytes && !d_utf8))
      throw_error(CTOK_E_ARG, "null argument");
    *n_bytes_out = 0;
    nz->prepare();
    hipStream_t s = (hipStream_t)stream;
    if (!n_texts) {
      HIPT(hipMemsetAsync(d_out_off, 0, 8, s));
      HIPT(hipStreamSynchronize(s));
      return;
    }
    const View r = nz->run_steps(View{d_utf8, d_off, n_bytes}, n_texts, s);
    *n_bytes_out = r.n_bytes;
    if (r.n_bytes > out_cap) {
      HIPT(hipStreamSynchronize(s));
      throw_error(CTOK_E_CAPACITY, "ctok_normalizer_run_device: the output needs " + std::to_string(r.n_bytes) + " bytes");
    }
    if (r.n_bytes && !d_out) throw_error(CTOK_E_ARG, "null argument");
    if (r.n_bytes) HIPT(hipMemcpyAsync(d_out, r.text, r.n_bytes, hipMemcpyDeviceToDevice, s));
    HIPT(hipMemcpyAsync(d_out_off, r.off, (n_texts + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIPT(hipStreamSynchronize(s));
  });
}

int ctok_normalizer_stage_ms(const ctok_normalizer* nz, double* ms, uint64_t cap, uint64_t* n) {
  return ctok_host::run_guarded([&] {
    if (!nz || !n || (cap && !ms)) throw_error(CTOK_E_ARG, "null argument");
    *n = nz->prog.size();
    for (uint64_t i = 0; i < cap && i < nz->prog.size(); i++) ms[i] = i < nz->ms.size() ? nz->ms[i] : 0.0;
  });
}

const char* ctok_normalizer_stage_name(const ctok_normalizer* nz, uint64_t i) {
  return nz && i < nz->prog.size() ? normalize::prim_name(nz->prog[i].kind) : "";
}

int ctok_normalizer_stats(const ctok_normalizer* nz, ctok_normalizer_info* out) {
  return ctok_host::run_guarded([&] {
    if (!nz || !out) throw_error(CTOK_E_ARG, "null argument");
    *out = nz->info;
  });
}

}  // extern "C"
