// The whitespace word split of the classic BPE trainer (bpe_train.hip k_ws_bits), shared with the
// host (bpe_train_host.cpp) and the CPU check (tools/ws_split_check.cpp): plain integer code, no
// HIP include, no intrinsics.
//
// Reference: str::split_whitespace (src/bpe_trainer.rs:244) splits on the 25 code points with the
// Unicode White_Space property, all in the BMP:
//   1 byte   09-0D 20
//   2 bytes  C2 85 (U+0085)  C2 A0 (U+00A0)
//   3 bytes  E1 9A 80 (U+1680)  E2 80 80-8A (U+2000-200A)  E2 80 A8/A9/AF (U+2028 2029 202F)
//            E2 81 9F (U+205F)  E3 80 80 (U+3000)
// U+001C-001F (which Python's str.split also splits on) and U+200B are not among them.
//
// A run starts at a code point whose class (whitespace or not) differs from the class of the code
// point before it, and at byte 0.  Every function takes the text and its length and reads no byte
// at or past n.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WS_HD __host__ __device__ __forceinline__
#else
#define WS_HD inline
#endif

namespace wsplit {

WS_HD bool is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// the code point whose lead byte is text[p] (p < n) is whitespace
WS_HD bool ws_at(const uint8_t* text, uint64_t n, uint64_t p) {
  const uint8_t b0 = text[p];
  if (b0 < 0x80u) return (b0 >= 0x09u && b0 <= 0x0Du) || b0 == 0x20u;
  if (b0 == 0xC2u) return p + 1 < n && (text[p + 1] == 0x85u || text[p + 1] == 0xA0u);
  if (b0 < 0xE1u || b0 > 0xE3u || p + 2 >= n) return false;
  const uint8_t b1 = text[p + 1], b2 = text[p + 2];
  if (b0 == 0xE1u) return b1 == 0x9Au && b2 == 0x80u;
  if (b0 == 0xE3u) return b1 == 0x80u && b2 == 0x80u;
  if (b1 == 0x80u) return (b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu;
  return b1 == 0x81u && b2 == 0x9Fu;
}

// a run of whitespace or of non-whitespace code points starts at byte g (g < n).  Looks back at
// most 3 bytes for the previous code point's lead byte: a code point with 3 continuation bytes is
// 4 bytes long and no whitespace.
WS_HD bool run_start(const uint8_t* text, uint64_t n, uint64_t g) {
  if (is_cont(text[g])) return false;
  if (g == 0) return true;
  uint64_t q = g - 1;
  int back = 1;
  while (back < 3 && q > 0 && is_cont(text[q])) {
    q--;
    back++;
  }
  const bool prev_ws = !is_cont(text[q]) && ws_at(text, g, q);  // (the previous code point ends at g)
  return prev_ws != ws_at(text, n, g);
}

// the 32 run-start bits of text bytes [32 * w, 32 * w + 32); bits at or past n stay clear
WS_HD uint32_t run_start_bits(const uint8_t* text, uint64_t n, uint64_t w) {
  uint32_t v = 0;
  for (uint32_t j = 0; j < 32; j++) {
    const uint64_t g = w * 32 + j;
    if (g < n && run_start(text, n, g)) v |= 1u << j;
  }
  return v;
}

}  // namespace wsplit
