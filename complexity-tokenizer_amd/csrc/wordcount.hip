// HIP kernels (gfx950) of the INL-BPE trainer's word counting.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3, src/trainer.rs): count_batch :207-220,
// count_words :265-285 -- a HashMap<String, u32> of every pre-tokenized piece of >= min_word_length
// chars.  Here the pieces never leave the device: the kernels read what a pretok-only encode call
// leaves there (the text the pieces index and k_segment's piece-start bitmap) and count into a
// global open-addressing table whose slots refer into that text (wordcount_hd.h).
//
// A word is the bytes from a piece start to the next piece start, or to the end of the text.
// k_segment sets a start bit at every non-empty document's first byte (seg::starts returns D | ...,
// D = the document starts), so a piece never spans two documents and the document offsets are not
// read at all.
//
//   k_wc_count   thread per 32-bit bitmap word (32 text bytes), grid-stride, persistent workgroups.
//                Every piece is hashed and added to the workgroup's LDS table (kLdsSlots slots,
//                kLdsProbe probes, same descriptors); a piece that finds no LDS slot goes to the
//                global table with count 1.  At its end the workgroup flushes its LDS slots as
//                (word, count) into the global table: a hot word costs one global atomic per
//                workgroup, not one per occurrence.
//   k_wc_lens / scan / k_wc_copy   the drain: lengths of the used slots, their prefix sum, and the
//                words' bytes gathered behind each other -- O(unique words) to read back.
//
// Wait-free: a slot is claimed by one 64-bit compare-and-swap of a complete descriptor; whoever
// loses reads the winner's descriptor from the swap's return value and compares against the
// (immutable) text.  No lane waits for another lane's store.  Every loop is bounded: probes by
// min(capacity, kMaxProbe), bitmap scans by the bitmap, byte loops by the word.  A probe sequence
// that runs out sets ctr[kCtrOverflow] and the kernel carries on; the host then discards the
// chunk's table and counts the chunk again (trainer_host.cpp).  No MFMA: integer/hash work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctok_internal.h"
#include "wordcount_hd.h"
#include "wordcount_internal.h"

namespace ctok_wc {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kLdsSlots = 1024;  // 16 B per slot (descriptor, count, hash bits): 16 KiB per workgroup
constexpr uint32_t kLdsProbe = 4;
constexpr uint32_t kMaxProbe = 4096;
constexpr uint32_t kMaxGrid = 2048;   // persistent workgroups: a 256 MB chunk gives each ~4096 bitmap words

// first piece start at or after byte `from`, or n_bytes
__device__ __forceinline__ uint32_t next_start(const Text& x, uint32_t from) {
  uint32_t wi = from >> 5;
  if (wi >= x.n_words) return x.n_bytes;
  uint32_t v = x.pbits[wi] & (~0u << (from & 31));
  while (!v) {
    if (++wi >= x.n_words) return x.n_bytes;
    v = x.pbits[wi];
  }
  return min(wi * 32u + (uint32_t)__ffs(v) - 1u, x.n_bytes);
}

// the descriptor d names the word text[pos .. pos + len) (tag and clipped length compared by the caller)
__device__ __forceinline__ bool same_word(const Text& x, uint64_t d, uint32_t pos, uint32_t len) {
  const uint32_t r = wc::pos_of(d);
  // a clipped length says only ">= kLenClip": the resident word must end where this one does
  if (len >= wc::kLenClip && next_start(x, r + 1) - r != len) return false;
  return wc::words_equal(x.text, pos, r, len);
}

__device__ __forceinline__ void global_add(const Text& x, const Table& t, uint32_t pos, uint32_t len, uint64_t hash,
                                           uint32_t count) {
  const uint32_t lc = wc::clip_len(len), tag = (uint32_t)hash & 0xFFFFu;
  const uint64_t mine = wc::pack(pos, lc, tag);
  uint32_t h = (uint32_t)(hash >> 32) & t.mask;
  const uint32_t tries = min(t.mask, kMaxProbe - 1u) + 1u;
  for (uint32_t i = 0; i < tries; i++, h = (h + 1) & t.mask) {
    // (a stale read can only show kEmpty for a taken slot: the swap below then returns its descriptor)
    uint64_t k = t.keys[h];
    if (k == wc::kEmpty) {
      k = atomicCAS((unsigned long long*)&t.keys[h], (unsigned long long)wc::kEmpty, (unsigned long long)mine);
      if (k == wc::kEmpty) {  // this thread took the slot
        t.used[atomicAdd(&t.ctr[kCtrUsed], 1u)] = h;
        k = mine;
      }
    }
    if (k == mine || (wc::may_match(k, lc, tag) && same_word(x, k, pos, len))) {
      atomicAdd(&t.vals[h], count);
      return;
    }
  }
  atomicOr(&t.ctr[kCtrOverflow], 1u);
}

__global__ __launch_bounds__(kThreads) void k_wc_pieces(Text x, uint32_t* ctr) {
  uint32_t n = 0;
  for (uint32_t wi = blockIdx.x * kThreads + threadIdx.x; wi < x.n_words; wi += gridDim.x * kThreads) n += __popc(x.pbits[wi]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctr[kCtrPieces], n);
}

__global__ __launch_bounds__(kThreads) void k_wc_count(Text x, Table t, uint32_t min_len) {
  __shared__ unsigned long long s_key[kLdsSlots];
  __shared__ uint32_t s_cnt[kLdsSlots];
  __shared__ uint32_t s_hi[kLdsSlots];  // hash bits 63..32 of the slot's word (the global slot)
  for (uint32_t i = threadIdx.x; i < kLdsSlots; i += kThreads) {
    s_key[i] = wc::kEmpty;
    s_cnt[i] = 0;
  }
  __syncthreads();
  uint32_t n_words = 0;
  for (uint32_t wi = blockIdx.x * kThreads + threadIdx.x; wi < x.n_words; wi += gridDim.x * kThreads) {
    // (the chunk is counted again after an overflow: stop early)
    if (__hip_atomic_load(&t.ctr[kCtrOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    uint32_t v = x.pbits[wi];
    while (v) {
      const uint32_t pos = wi * 32u + (uint32_t)__ffs(v) - 1u;
      v &= v - 1;
      const uint32_t end = v ? wi * 32u + (uint32_t)__ffs(v) - 1u : next_start(x, (wi + 1) * 32u);
      const uint32_t len = end - pos;
      if (len < min_len) continue;
      n_words++;
      const uint64_t hash = wc::word_hash(x.text, pos, len);
      const uint32_t lc = wc::clip_len(len), tag = (uint32_t)hash & 0xFFFFu;
      const uint64_t mine = wc::pack(pos, lc, tag);
      uint32_t ls = (uint32_t)(hash >> 16) & (kLdsSlots - 1);
      bool done = false;
      for (uint32_t j = 0; j < kLdsProbe && !done; j++, ls = (ls + 1) & (kLdsSlots - 1)) {
        uint64_t k = __hip_atomic_load(&s_key[ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == wc::kEmpty) {
          k = atomicCAS(&s_key[ls], (unsigned long long)wc::kEmpty, (unsigned long long)mine);
          if (k == wc::kEmpty) {
            s_hi[ls] = (uint32_t)(hash >> 32);  // (read only after the barrier below)
            k = mine;
          }
        }
        if (k == mine || (wc::may_match(k, lc, tag) && same_word(x, k, pos, len))) {
          atomicAdd(&s_cnt[ls], 1u);
          done = true;
        }
      }
      if (!done) global_add(x, t, pos, len, hash, 1u);
    }
  }
  __syncthreads();
  // flush: (word, count) of every LDS slot into the global table
  for (uint32_t i = threadIdx.x; i < kLdsSlots; i += kThreads) {
    const uint64_t k = s_key[i];
    if (k == wc::kEmpty) continue;
    const uint32_t pos = wc::pos_of(k);
    const uint32_t len = wc::len_of(k) < wc::kLenClip ? wc::len_of(k) : next_start(x, pos + 1) - pos;
    global_add(x, t, pos, len, ((uint64_t)s_hi[i] << 32) | wc::tag_of(k), s_cnt[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_words += __shfl_xor(n_words, o, 64);
  if ((threadIdx.x & 63) == 0 && n_words) atomicAdd(&t.ctr[kCtrWords], n_words);
}

// drain, step 1: the used slots' lengths (scanned to offsets), first occurrences and counts
__global__ __launch_bounds__(kThreads) void k_wc_lens(Text x, Table t, uint32_t n_used, uint64_t* out_off, uint32_t* out_cnt,
                                                      uint32_t* pos_out) {
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n_used; i += gridDim.x * kThreads) {
    const uint32_t h = t.used[i];
    const uint64_t k = t.keys[h];
    const uint32_t pos = wc::pos_of(k);
    out_off[i] = wc::len_of(k) < wc::kLenClip ? wc::len_of(k) : next_start(x, pos + 1) - pos;
    out_cnt[i] = t.vals[h];
    pos_out[i] = pos;
  }
}

// drain, step 2: word i's bytes to out_bytes[out_off[i] .. out_off[i + 1]); a wavefront per word
__global__ __launch_bounds__(kThreads) void k_wc_copy(Text x, uint32_t n_used, const uint64_t* out_off, const uint32_t* pos,
                                                      uint8_t* out_bytes) {
  const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (kThreads / 64);
  for (uint32_t i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); i < n_used; i += waves) {
    const uint64_t o = out_off[i], len = out_off[i + 1] - o;
    const uint8_t* src = x.text + pos[i];
    for (uint64_t b = lane; b < len; b += 64) out_bytes[o + b] = src[b];
  }
}

static uint32_t grid_for(uint64_t n, uint32_t per_block) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

hipError_t launch_pieces(const Text& x, uint32_t* ctr, hipStream_t s) {
  if (x.n_words) k_wc_pieces<<<grid_for(x.n_words, kThreads), kThreads, 0, s>>>(x, ctr);
  return hipGetLastError();
}

hipError_t launch_count(const Text& x, const Table& t, uint32_t min_len, hipStream_t s) {
  if (x.n_words) k_wc_count<<<grid_for(x.n_words, kThreads), kThreads, 0, s>>>(x, t, min_len);
  return hipGetLastError();
}

uint64_t drain_tmp_elems(uint64_t n_used) { return ctok_dev::scan_tmp_elems(n_used + 1) + 64; }

hipError_t launch_drain(const Text& x, const Table& t, uint32_t n_used, uint8_t* out_bytes, uint64_t* out_off,
                        uint32_t* out_cnt, uint32_t* pos, uint64_t* tmp, uint64_t tmp_cap, hipStream_t s) {
  if (!n_used) return hipSuccess;
  k_wc_lens<<<grid_for(n_used, kThreads), kThreads, 0, s>>>(x, t, n_used, out_off, out_cnt, pos);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = ctok_dev::scan_u64(out_off, n_used, tmp, tmp_cap, s);  // exclusive; out_off[n_used] = total
  if (e != hipSuccess) return e;
  k_wc_copy<<<grid_for(n_used, kThreads / 64), kThreads, 0, s>>>(x, n_used, out_off, pos, out_bytes);
  return hipGetLastError();
}

}  // namespace ctok_wc
