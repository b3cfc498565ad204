// HIP kernels (gfx950) of the Lowercase normaliser (lowercase_hd.h: Rust's str::to_lowercase), the
// second step of the WordPiece trainer's Sequence[NFC, Lowercase].
//
// Two phases, as k_norm: a thread owns a span of kLowerSpan input bytes (the code points that start
// in it) and (1) adds up their output bytes, (2) after the host's scan_u64 over the spans, writes
// them.  Lowercase changes UTF-8 lengths both ways (U+023A 2 -> 3 bytes, U+212A 3 -> 1), so every
// text's new offset comes out of the same sums (k_lower_off).  Phase 1 also reports whether any
// code point changed at all: text that nothing changes (lower-case ASCII, say) is not copied.
// A sigma's context may reach across spans but never leaves its text; its two loops are bounded by
// the text.  No thread writes what another reads within a kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#define LC_DATA_ATTR __device__
#include "gen/lowercase_data.h"
#include "lowercase_hd.h"
#include "wordpiece_internal.h"

namespace ctok_wp {

constexpr uint32_t kThreads = 256;

static uint32_t grid_for(uint64_t n, uint32_t max_grid) {
  const uint64_t g = (n + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ lowercase::Tables dev_tables() {
  return lowercase::Tables{lc_map_from, lc_map_to, LC_N_MAP, lc_cased, LC_N_CASED_RANGES, lc_ignorable,
                           LC_N_IGNORABLE_RANGES};
}

// the text of byte p < doc_off[n_docs]: the d with doc_off[d] <= p < doc_off[d + 1]
__device__ __forceinline__ uint64_t doc_of(const uint64_t* doc_off, uint64_t n_docs, uint64_t p) {
  uint64_t lo = 0, hi = n_docs;  // the first d with doc_off[d + 1] > p
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (doc_off[mid + 1] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the output bytes of the units that start in [b0, b1) (b1 <= n_bytes), written to out when non-null
__device__ __forceinline__ uint64_t lower_range(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs,
                                                uint64_t b0, uint64_t b1, uint8_t* out, bool* changed) {
  const lowercase::Tables T = dev_tables();
  uint64_t d = doc_of(doc_off, n_docs, b0), total = 0;
  for (uint64_t p = b0; p < b1; p++) {
    while (d + 1 < n_docs && p >= doc_off[d + 1]) d++;
    const uint64_t lo = doc_off[d], hi = doc_off[d + 1];
    if (!lowercase::is_start(text, lo, hi, p)) continue;
    uint32_t in_len;
    bool same;
    total += lowercase::lower_at(T, text, lo, hi, p, &in_len, &same, out ? out + total : nullptr);
    if (!same) *changed = true;
    p += in_len - 1;
  }
  return total;
}

__global__ __launch_bounds__(kThreads) void k_lower_count(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                                                          uint64_t n_docs, uint64_t n_spans, uint64_t* len,
                                                          uint32_t* changed) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t b0 = i * kLowerSpan, b1 = b0 + kLowerSpan < n_bytes ? b0 + kLowerSpan : n_bytes;
    bool ch = false;
    len[i] = lower_range(text, doc_off, n_docs, b0, b1, nullptr, &ch);
    if (ch) atomicOr(changed, 1u);
  }
}

__global__ __launch_bounds__(kThreads) void k_lower_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                                                          uint64_t n_docs, uint64_t n_spans, const uint64_t* pos,
                                                          uint8_t* out) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t b0 = i * kLowerSpan, b1 = b0 + kLowerSpan < n_bytes ? b0 + kLowerSpan : n_bytes;
    bool ch = false;
    (void)lower_range(text, doc_off, n_docs, b0, b1, out + pos[i], &ch);
  }
}

// out_off[d] = where the output of the byte doc_off[d] begins (texts begin at unit starts)
__global__ __launch_bounds__(kThreads) void k_lower_off(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                                                        uint64_t n_docs, uint64_t n_spans, const uint64_t* pos,
                                                        uint64_t* out_off) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = doc_off[d];
    if (o >= n_bytes) {
      out_off[d] = pos[n_spans];
      continue;
    }
    const uint64_t i = o / kLowerSpan;
    bool ch = false;
    out_off[d] = pos[i] + lower_range(text, doc_off, n_docs, i * kLowerSpan, o, nullptr, &ch);
  }
}

hipError_t launch_lower_count(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                              uint64_t* len, uint32_t* changed, hipStream_t s) {
  const uint64_t n_spans = (n_bytes + kLowerSpan - 1) / kLowerSpan;
  if (n_spans && n_docs)
    k_lower_count<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(text, n_bytes, doc_off, n_docs, n_spans, len, changed);
  return hipGetLastError();
}

hipError_t launch_lower_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                              const uint64_t* pos, uint8_t* out, uint64_t* out_off, hipStream_t s) {
  const uint64_t n_spans = (n_bytes + kLowerSpan - 1) / kLowerSpan;
  if (!n_spans || !n_docs) return hipSuccess;
  k_lower_write<<<grid_for(n_spans, 16384), kThreads, 0, s>>>(text, n_bytes, doc_off, n_docs, n_spans, pos, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_lower_off<<<grid_for(n_docs + 1, 8192), kThreads, 0, s>>>(text, n_bytes, doc_off, n_docs, n_spans, pos, out_off);
  return hipGetLastError();
}

}  // namespace ctok_wp
