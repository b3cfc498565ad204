// CPU driver of csrc/lowercase_hd.h (str::to_lowercase behind lowercase.hip) for
// tests/test_lowercase_cpu.py, which compares its output with Python's str.lower().
// Build: g++ -O2 -std=c++17 lowercase_check.cpp -o lowercase_check
// stdin:  u64 n, u64 off[n + 1], then off[n] bytes: n texts behind each other
// stdout: u64 out_off[n + 1], then out_off[n] bytes
// Every byte is visited the way the kernel's threads visit it: is_start() decides whether a unit
// starts there, lower_at() gives its output, with the text's own bounds as the sigma's context.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/gen/lowercase_data.h"
#include "../csrc/lowercase_hd.h"

static bool read_all(void* p, size_t n) { return !n || fread(p, 1, n, stdin) == n; }

int main() {
  const lowercase::Tables T{lc_map_from, lc_map_to, LC_N_MAP, lc_cased, LC_N_CASED_RANGES, lc_ignorable,
                            LC_N_IGNORABLE_RANGES};
  uint64_t n = 0;
  if (!read_all(&n, 8)) return 2;
  std::vector<uint64_t> off(n + 1);
  if (!read_all(off.data(), (n + 1) * 8)) return 2;
  std::vector<uint8_t> text(off[n] + 1);
  if (!read_all(text.data(), off[n])) return 2;
  std::vector<uint8_t> out;
  std::vector<uint64_t> out_off(n + 1, 0);
  out.reserve(off[n] * 3 / 2 + 16);
  for (uint64_t d = 0; d < n; d++) {
    const uint64_t lo = off[d], hi = off[d + 1];
    for (uint64_t p = lo; p < hi; p++) {
      if (!lowercase::is_start(text.data(), lo, hi, p)) continue;
      uint8_t buf[4];
      uint32_t in_len;
      bool same;
      const uint32_t len = lowercase::lower_at(T, text.data(), lo, hi, p, &in_len, &same, buf);
      const uint32_t len2 = lowercase::lower_at(T, text.data(), lo, hi, p, &in_len, &same, nullptr);
      if (len != len2 || len > 4) return 3;  // (the counting and the writing pass must agree)
      bool equal = len == in_len;  // (`same` is what lets unchanged text go uncopied)
      for (uint32_t j = 0; j < len && equal; j++) equal = buf[j] == text[p + j];
      if (equal != same) return 4;
      out.insert(out.end(), buf, buf + len);
    }
    out_off[d + 1] = out.size();
  }
  fwrite(out_off.data(), 8, n + 1, stdout);
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
