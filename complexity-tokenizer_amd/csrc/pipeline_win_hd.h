// The per-row arithmetic of PipelineTokenizer's padded batches and stride windows (pipeline_win.hip):
// Encoding::truncate, Encoding::truncate_with_stride and Encoding::pad (src/encoding.rs:87-223) as
// closed forms over a row's lengths.  Shared by the kernels, the host runtime (the panic's message) and
// tools/pipeline_win_check.cpp, which compares every function with a literal loop of the three methods
// on the CPU: integer code only, every product in 64 bits.
//
// A row has P processed ids and lists of other lengths: `tokens` has t entries (the ids before the
// post-processor; without special tokens the ids that have a vocab string), offsets / word_ids / sequence_ids
// have n.  With max_length m and stride s < m:
//   kNone     one window [0, P)
//   kCut      P > m: [0, m), the remainder is dropped; the reference slices tokens[m .. t] first
//   kWindows  P > m: window k = [k (m - s), min(k (m - s) + m, P)), 1 + ceil((P - m) / (m - s)) of them;
//             every window slices tokens[start .. end]
// A list of `len` entries gives a window list[start .. min(end, len)] when len > start, else nothing.  Only
// window 0 is padded: its Encoding grows to the target, and sequence_ids grows by as many None.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PWIN_HD __host__ __device__ __forceinline__
#else
#define PWIN_HD inline
#endif

namespace pwin {

enum Mode : uint32_t { kNone = 0, kCut = 1, kWindows = 2 };

PWIN_HD bool valid(uint32_t mode, uint64_t m, uint64_t s) { return mode != kWindows || s < m; }

// windows of a row (valid(mode, m, s))
PWIN_HD uint64_t count(uint32_t mode, uint64_t P, uint64_t m, uint64_t s) {
  if (mode != kWindows || P <= m) return 1;
  const uint64_t step = m - s, over = P - m;
  return 1 + over / step + (over % step ? 1 : 0);
}

// ids of window 0
PWIN_HD uint64_t main_len(uint32_t mode, uint64_t P, uint64_t m) { return mode != kNone && P > m ? m : P; }

PWIN_HD uint64_t start(uint64_t k, uint64_t m, uint64_t s) { return k ? k * (m - s) : 0; }

// one past the last position of window k (k < count)
PWIN_HD uint64_t end(uint32_t mode, uint64_t k, uint64_t P, uint64_t m, uint64_t s) {
  if (!k) return main_len(mode, P, m);
  const uint64_t e = start(k, m, s) + m;
  return e < P ? e : P;
}

// entries of a list of `len` that window [a, e) takes
PWIN_HD uint64_t list_len(uint64_t len, uint64_t a, uint64_t e) { return len > a ? (e < len ? e : len) - a : 0; }

// the Encoding length of window k with `ids` ids: padding included
PWIN_HD uint64_t enc_len(uint64_t k, uint64_t ids, uint64_t target) { return !k && target > ids ? target : ids; }

// does the reference panic on this row
PWIN_HD bool panics(uint32_t mode, uint64_t P, uint64_t t, uint64_t m) {
  if (mode == kNone || P <= m) return false;
  return mode == kCut ? m > t : P > t;
}

// the range end of the slice that panics (panics(...) holds): tokens[m .. t] has its start past its end in
// kCut, and the first window that ends past t in kWindows
PWIN_HD uint64_t panic_end(uint32_t mode, uint64_t P, uint64_t t, uint64_t m, uint64_t s) {
  if (mode == kCut) return t;
  const uint64_t k = t < m ? 1 : (t - m) / (m - s) + 1;
  return end(mode, k, P, m, s);
}

}  // namespace pwin
