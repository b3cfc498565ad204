// HIP kernels (gfx950) of the Normalizer's primitive steps (normalize_hd.h: the reference's
// src/normalizers.rs:43-202): decomposition, canonical ordering, composition, the accent filter, the
// two BERT passes, Strip, Replace and the constants Prepend / Append / an empty pattern put around a
// text.  Lowercase is lowercase.hip's.
//
// Every step has the shape of lowercase.hip: a thread owns the units that start in a span of kSpan
// input bytes and (1) adds up their output bytes, (2) after the host's scan_u64 over the spans,
// writes them; the texts' new offsets come out of the same sums (k_nz_off).  A unit may reach past
// its span (a run of non-starters, a composing segment, a match) but never leaves its text, so every
// loop is bounded by the text, and no kernel waits on another workgroup.  Within a kernel no thread
// writes what another reads: Replace's candidates and the applied matches are two arrays, written by
// two kernels (k_nz_cand, k_nz_chain) before the count reads them.
#include <hip/hip_runtime.h>

#include <cstdint>

#define NZ_DATA_ATTR __device__
#include "gen/normalize_data.h"
#include "normalize_hd.h"
#include "normalize_internal.h"

namespace ctok_nz {

using normalize::kSpan;
using normalize::Step;

constexpr uint32_t kThreads = 256;

static uint32_t grid_for(uint64_t n, uint32_t max_grid) {
  const uint64_t g = (n + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ normalize::Tables dev_tables() {
  return normalize::Tables{nz_run_index, nz_run_start, nz_run_val, NZ_N_RUNS, NZ_N_INDEXED, NZ_RUN_SHIFT,
                           nz_d_cp, nz_d_loc, NZ_N_D, nz_k_cp, nz_k_loc, NZ_N_K, nz_kr_first, nz_kr_count, nz_kr_to,
                           NZ_N_KR, nz_pool, nz_comp_key, nz_comp_to, NZ_N_COMP};
}

__device__ __forceinline__ uint64_t span_end(uint64_t i, uint64_t n_bytes) {
  return (i + 1) * kSpan < n_bytes ? (i + 1) * kSpan : n_bytes;
}

__global__ __launch_bounds__(kThreads) void k_nz_count(Step st, const uint8_t* text, uint64_t n_bytes,
                                                       const uint64_t* doc_off, uint64_t n_docs, uint64_t n_spans,
                                                       uint64_t* len, uint32_t* changed) {
  const normalize::Tables T = dev_tables();
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    bool ch = false;
    len[i] = normalize::span_run(T, st, text, doc_off, n_docs, i * kSpan, span_end(i, n_bytes), nullptr, &ch);
    if (ch) atomicOr(changed, 1u);
  }
}

__global__ __launch_bounds__(kThreads) void k_nz_write(Step st, const uint8_t* text, uint64_t n_bytes,
                                                       const uint64_t* doc_off, uint64_t n_docs, uint64_t n_spans,
                                                       const uint64_t* pos, uint8_t* out) {
  const normalize::Tables T = dev_tables();
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    bool ch = false;
    (void)normalize::span_run(T, st, text, doc_off, n_docs, i * kSpan, span_end(i, n_bytes), out + pos[i], &ch);
  }
}

// out_off[d] = where text d's output begins; the thread also writes the constants at that edge
__global__ __launch_bounds__(kThreads) void k_nz_off(Step st, const uint8_t* text, uint64_t n_bytes,
                                                     const uint64_t* doc_off, uint64_t n_docs, uint64_t n_spans,
                                                     const uint64_t* pos, uint8_t* out, uint64_t* out_off) {
  const normalize::Tables T = dev_tables();
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * kThreads)
    out_off[d] = normalize::off_run(T, st, text, n_bytes, doc_off, n_docs, n_spans, pos, d, out);
}

__global__ __launch_bounds__(kThreads) void k_nz_trim(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs,
                                                      uint64_t* trim) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * kThreads) {
    uint64_t a, b;
    normalize::trim_bounds(text, doc_off[d], doc_off[d + 1], &a, &b);
    trim[2 * d] = a;
    trim[2 * d + 1] = b;
  }
}

__global__ __launch_bounds__(kThreads) void k_nz_cand(Step st, const uint8_t* text, uint64_t n_bytes,
                                                      const uint64_t* doc_off, uint64_t n_docs, uint64_t n_spans,
                                                      uint8_t* cand) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads)
    normalize::cand_run(st, text, doc_off, n_docs, i * kSpan, span_end(i, n_bytes), cand);
}

// (st.cand is k_nz_cand's finished array; taken is zero before the kernel and only chain walkers
// write it, each inside its own chain)
__global__ __launch_bounds__(kThreads) void k_nz_chain(Step st, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                                                       uint64_t n_spans, uint8_t* taken) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads)
    normalize::chain_run(st, doc_off, n_docs, i * kSpan, span_end(i, n_bytes), taken);
}

hipError_t launch_count(const Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                        uint64_t* len, uint32_t* changed, hipStream_t s) {
  const uint64_t n_spans = (n_bytes + kSpan - 1) / kSpan;
  if (n_spans && n_docs)
    k_nz_count<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(st, text, n_bytes, doc_off, n_docs, n_spans, len, changed);
  return hipGetLastError();
}

hipError_t launch_write(const Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                        const uint64_t* pos, uint8_t* out, uint64_t* out_off, hipStream_t s) {
  const uint64_t n_spans = (n_bytes + kSpan - 1) / kSpan;
  if (!n_docs) return hipSuccess;
  if (n_spans) {
    k_nz_write<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(st, text, n_bytes, doc_off, n_docs, n_spans, pos, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  k_nz_off<<<grid_for(n_docs + 1, 8192), kThreads, 0, s>>>(st, text, n_bytes, doc_off, n_docs, n_spans, pos, out, out_off);
  return hipGetLastError();
}

hipError_t launch_trim(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, uint64_t* trim, hipStream_t s) {
  if (n_docs) k_nz_trim<<<grid_for(n_docs, 8192), kThreads, 0, s>>>(text, doc_off, n_docs, trim);
  return hipGetLastError();
}

hipError_t launch_matches(const Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                          uint8_t* cand, uint8_t* taken, hipStream_t s) {
  const uint64_t n_spans = (n_bytes + kSpan - 1) / kSpan;
  if (!n_spans || !n_docs) return hipSuccess;
  hipError_t e = hipMemsetAsync(taken, 0, n_bytes, s);
  if (e != hipSuccess) return e;
  k_nz_cand<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(st, text, n_bytes, doc_off, n_docs, n_spans, cand);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  Step walk = st;
  walk.cand = cand;
  k_nz_chain<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(walk, n_bytes, doc_off, n_docs, n_spans, taken);
  return hipGetLastError();
}

}  // namespace ctok_nz
