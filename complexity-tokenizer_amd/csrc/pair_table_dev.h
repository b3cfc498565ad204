// The resident pair table's device side (bpe_train_internal.h Table): the slot of a key and the
// exact add, shared by the kernels that update the table in place (bpe_train.hip k_pair_count and
// k_bpe_merge, wordpiece.hip k_wp_walk).  Device-only; include after hip_runtime.h.
#pragma once
#include <cstdint>

#include "bpe_train_internal.h"

namespace ctok_bpe {

__device__ __forceinline__ uint32_t slot_of(uint64_t key, uint32_t cap) {
  const uint64_t h = (key * 0x9E3779B97F4A7C15ull) >> 32;  // 32 hash bits -> [0, cap)
  return (uint32_t)((h * cap) >> 32);
}

// count += v for key (inserting it on first use); at most min(cap, kMaxProbe) slots are looked at
__device__ __forceinline__ void table_add(const Table& T, uint64_t key, int64_t v) {
  uint32_t h = slot_of(key, T.cap);
  const uint32_t tries = T.cap < kMaxProbe ? T.cap : kMaxProbe;
  for (uint32_t i = 0; i < tries; i++) {
    // (a stale read can only show kEmptyKey for a taken slot: the swap below then returns its key)
    uint64_t k = T.keys[h];
    if (k == kEmptyKey) {
      k = atomicCAS((unsigned long long*)&T.keys[h], (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (k == kEmptyKey) {  // this thread took the slot
        atomicAdd(&T.ctr[kCtrTaken], 1u);
        k = key;
      }
    }
    if (k == key) {
      atomicAdd((unsigned long long*)&T.vals[h], (unsigned long long)v);
      return;
    }
    h = h + 1 == T.cap ? 0 : h + 1;
  }
  atomicOr(&T.ctr[kCtrOverflow], 1u);
}

}  // namespace ctok_bpe
