// Stride windows of a row that is longer than max_length (Encoding::truncate_with_stride,
// src/encoding.rs:175-223, reached from Tokenizer.__call__(truncation, stride) and
// encode_with_truncation): the window count of a row and the bounds of window k.  Shared by the
// kernels (pad.hip: k_win_len, k_win_rows), the host runtime and the host-side check in tests
// (tools/window_check.cpp): integer code only, every product in 64 bits.
//
// A row of processed length P, max_length m and stride s < m:
//     P <= m   one window, [0, P)
//     P >  m   the reference cuts [0, m), then from pos = m: start = pos - s, end = min(start + m,
//              P), pos = end, until pos reaches P.  Window k therefore starts at k * (m - s) and
//              the last one is the first whose end reaches P: 1 + ceil((P - m) / (m - s)) windows.
// s >= m (m == 0 included) never advances in the reference: valid() is false and callers refuse it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WIN_HD __host__ __device__ __forceinline__
#else
#define WIN_HD inline
#endif

namespace win {

WIN_HD bool valid(uint64_t m, uint64_t s) { return s < m; }

// windows of a row (valid(m, s))
WIN_HD uint64_t count(uint64_t P, uint64_t m, uint64_t s) {
  if (P <= m) return 1;
  const uint64_t step = m - s;
  const uint64_t over = P - m;
  return 1 + over / step + (over % step ? 1 : 0);
}

// first content position of window k
WIN_HD uint64_t start(uint64_t k, uint64_t m, uint64_t s) { return k * (m - s); }

// one past the last content position of window k (k < count(P, m, s))
WIN_HD uint64_t end(uint64_t k, uint64_t P, uint64_t m, uint64_t s) {
  const uint64_t e = start(k, m, s) + m;
  return e < P ? e : P;
}

}  // namespace win
