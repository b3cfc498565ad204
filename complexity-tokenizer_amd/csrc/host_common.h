// What the tokenizer's host runtime offers the trainer's (ctok_host.cpp defines it;
// trainer_host.cpp uses it).  Not part of the C ABI.  The tokenizer runtime's own shared
// internals are in host_internal.h.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

struct ctok;

namespace ctok_host {
// Throw a CTOK_E_* error (message for ctok_last_error); run_guarded turns it into the return code.
[[noreturn]] void throw_error(int code, const std::string& msg);
int run_guarded(const std::function<void()>& f);
// GPU pre-tokenization of a host batch with tokenizer t on device dev: the text the pieces index
// (NFC-normalised when normalisation ran), its doc offsets and the piece-start bitmap.
void pretokenize(ctok* t, int dev, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                 std::vector<uint8_t>& text, std::vector<uint64_t>& off, std::vector<uint32_t>& pbits,
                 uint64_t* bytes_d2h = nullptr);  // (optional) the bytes it copied device -> host
// What a pre-tokenization leaves on the device (device pointers; stream is a hipStream_t).  The
// text buffer is 16-byte aligned and has 16 readable bytes past n_bytes; pbits has a bit per text
// byte (bit g of word g / 32), clear from n_bytes on.
struct DevicePretok {
  const uint8_t* text;
  const uint64_t* doc_off;
  const uint32_t* pbits;
  uint64_t n_bytes;
  uint64_t n_docs;
  void* stream;
};
// pretokenize with no copy back to the host: use(r) runs while the device's mutex is held, after
// the pre-tokenizer's kernels on r.stream; r's buffers are valid until it returns.
void pretokenize_device(ctok* t, int dev, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs,
                        const std::function<void(const DevicePretok&)>& use);
// CPUs this process may run on: the affinity mask, capped by the cgroup v2 CPU quota (cpu.max) --
// what Rust's available_parallelism (rayon's default pool size) reports on Linux; >= 1
unsigned usable_cpus();
}  // namespace ctok_host
