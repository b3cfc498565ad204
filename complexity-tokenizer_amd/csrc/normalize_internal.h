// What the Normalizer's host runtime (normalize_host.cpp) calls in normalize.hip.  Not part of the
// C ABI.  Every pointer is a device pointer (a Step's strings too); text holds n_bytes bytes of
// n_docs texts, doc_off[0] = 0, doc_off[n_docs] = n_bytes.  A span is normalize::kSpan input bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "normalize_hd.h"

namespace ctok_nz {

// len[i] = output bytes of the units that start in span i; *changed is ORed with 1 when a unit's
// output differs from its input (a step that changes nothing is not copied).  n_bytes > 0.
hipError_t launch_count(const normalize::Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                        uint64_t n_docs, uint64_t* len, uint32_t* changed, hipStream_t s);
// pos: the exclusive scan of len with the total at pos[n_spans] (pos[0] = 0 when n_bytes is 0).
// Writes the units, the constants around every text and the n_docs + 1 new offsets.
hipError_t launch_write(const normalize::Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                        uint64_t n_docs, const uint64_t* pos, uint8_t* out, uint64_t* out_off, hipStream_t s);
// Strip: trim[2d], trim[2d + 1] = the bytes text d keeps
hipError_t launch_trim(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, uint64_t* trim, hipStream_t s);
// Replace (st.a_len >= 1): cand and taken, n_bytes > 0 bytes each, as normalize_hd.h defines them
hipError_t launch_matches(const normalize::Step& st, const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                          uint64_t n_docs, uint8_t* cand, uint8_t* taken, hipStream_t s);

}  // namespace ctok_nz
