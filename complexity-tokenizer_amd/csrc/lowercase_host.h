// Lowercase on the device as a host call (wordpiece_host.cpp defines it): the WordPiece trainer's
// second normaliser step, the Normalizer's Lowercase step (normalize_host.cpp) and ctok_lowercase
// share it.  Host-only; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "train_host_common.h"

namespace ctok_wp {

struct LowerBufs {
  ctok_train_host::DBuf<uint64_t> len, tmp, out_off;
  ctok_train_host::DBuf<uint8_t> out;
  ctok_train_host::DBuf<uint32_t> changed;
};

struct Lowered {  // device pointers: the input's own when nothing changed
  const uint8_t* text;
  const uint64_t* doc_off;
  uint64_t n_bytes;
  bool changed;
};

// text: n_bytes > 0 device bytes of n_docs > 0 texts (doc_off[0] = 0, doc_off[n_docs] = n_bytes).
// The result lies in b (16 zero bytes behind it) and is valid until b's next use.  An output of
// refuse_from bytes or more is CTOK_E_CAPACITY, thrown after the count and before any write.
Lowered lower_device(LowerBufs& b, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                     hipStream_t s, uint64_t refuse_from = ~0ull);

}  // namespace ctok_wp
