// What the two trainers' host runtimes (trainer_host.cpp, bpe_train_host.cpp) share: the HIP error
// check, a device buffer grown on demand, UTF-8 of a code point, the host clock.  Host-only; not
// part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/ctok.h"
#include "host_common.h"

#define HIPT(x)                                                                                                   \
  do {                                                                                                            \
    hipError_t e_ = (x);                                                                                          \
    if (e_ != hipSuccess) ctok_host::throw_error(CTOK_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace ctok_train_host {

template <typename T>
struct DBuf {  // device buffer, grown on demand (the contents are not kept)
  T* p = nullptr;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    HIPT(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)));
    cap = n;
  }
  // ensure() that reports an allocation failure instead of throwing (the buffer is then empty)
  bool try_ensure(size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();  // (the failure is handled: leave no error behind for the next call)
      p = nullptr;
      return false;
    }
    cap = n;
    return true;
  }
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
};

inline std::string utf8_of(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) { s += (char)(0xC0 | (c >> 6)); s += (char)(0x80 | (c & 63)); }
  else if (c < 0x10000) { s += (char)(0xE0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  else { s += (char)(0xF0 | (c >> 18)); s += (char)(0x80 | ((c >> 12) & 63)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  return s;
}

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace ctok_train_host
