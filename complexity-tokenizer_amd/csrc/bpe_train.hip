// HIP kernels (gfx950) of the classic frequency-BPE trainer behind include/ctok_bpe_trainer.h.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3, src/bpe_trainer.rs):
//   build_word_frequencies :240-273  str::split_whitespace per text          -> k_ws_bits (+ wordcount.hip)
//   count_pairs            :341-375  (first, second) -> sum of word freqs     -> k_pair_count
//   max_by_key             :152-155  the pair with the largest count          -> k_pair_best (two launches)
//   merge_pair             :378-399  every word rewritten, i += 2 on a merge  -> k_bpe_merge
// The reference counts all pairs again before every merge; here the pair table stays on the device
// and every merge updates it exactly (k_bpe_merge), so a merge costs one pass over the words, one
// pass over the table and a 32-byte readback.
//
// Words live in HBM as the INL trainer's CSR (trainer_internal.h Words); one thread owns a word, so
// words need no synchronisation.  Pair counts are 64-bit device atomics on one table (they execute
// at the memory side: workgroups on different XCDs add exactly, and integer sums do not depend on
// order).  A key is written once, by a compare-and-swap from kEmptyKey, and never changes until
// the host clears the table between kernels.  Every loop is bounded: probes by min(capacity,
// kMaxProbe), word loops by the word's length, reductions by the grid.  An add that finds no slot
// sets ctr[kCtrOverflow] and returns; the host then rebuilds the table from the words.  The only
// hand-off between workgroups is the kernel boundary.  No MFMA: integer/hash work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bpe_train_internal.h"
#include "pair_best_hd.h"
#include "pair_table_dev.h"
#include "ws_split_hd.h"

namespace ctok_bpe {

constexpr uint32_t kThreads = 256;

static uint32_t grid_for(uint64_t n, uint32_t max_grid) {
  const uint64_t g = (n + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

// ---- the whitespace split ------------------------------------------------------------------------

// thread per bitmap word (32 text bytes): its run-start bits, by a plain store of the whole word
__global__ __launch_bounds__(kThreads) void k_ws_bits(const uint8_t* text, uint32_t n_bytes, uint32_t n_words,
                                                      uint32_t* pbits) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < n_words; w += gridDim.x * kThreads)
    pbits[w] = wsplit::run_start_bits(text, n_bytes, w);
}

// thread per text: the start bit of a non-empty text.  Runs after k_ws_bits (the kernel boundary
// orders it behind that kernel's plain stores); texts that share a bitmap word meet in an atomic OR.
__global__ __launch_bounds__(kThreads) void k_ws_doc_starts(const uint64_t* doc_off, uint64_t n_docs, uint32_t n_bytes,
                                                            uint32_t* pbits) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = doc_off[d];
    if (o < doc_off[d + 1] && o < n_bytes) atomicOr(&pbits[o >> 5], 1u << (o & 31));
  }
}

// ---- the resident pair table (its exact add, table_add: pair_table_dev.h) ---------------------------

// count_pairs: thread per word (grid-stride)
__global__ __launch_bounds__(kThreads) void k_pair_count(Words W, Table T) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < W.n_words; w += gridDim.x * kThreads) {
    const int64_t f = (int64_t)W.wfreq[w];
    const uint32_t n = W.wlen[w];
    if (!f || n < 2) continue;
    const uint32_t* t = W.tok + W.wstart[w];
    for (uint32_t i = 0; i + 1 < n; i++) table_add(T, pbest::pair_key(t[i], t[i + 1]), f);
  }
}

// the workgroup's best candidate, valid in thread 0
__device__ __forceinline__ pbest::Cand block_best(pbest::Cand c) {
  __shared__ long long s_count[kThreads / 64];
  __shared__ unsigned long long s_key[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const pbest::Cand other = {(int64_t)__shfl_xor((long long)c.count, o, 64),
                               (uint64_t)__shfl_xor((unsigned long long)c.key, o, 64)};
    c = pbest::best_of(c, other);
  }
  if ((threadIdx.x & 63) == 0) {
    s_count[threadIdx.x >> 6] = c.count;
    s_key[threadIdx.x >> 6] = c.key;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t i = 1; i < kThreads / 64; i++) c = pbest::best_of(c, pbest::Cand{s_count[i], s_key[i]});
  return c;
}

// first launch: grid-stride over the slots, one partial (count, key) per workgroup
__global__ __launch_bounds__(kThreads) void k_pair_best_partial(Table T, uint64_t* partial) {
  pbest::Cand c = pbest::kNone;
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < T.cap; i += gridDim.x * kThreads) {
    const int64_t v = T.vals[i];
    if (v > 0) c = pbest::best_of(c, pbest::Cand{v, T.keys[i]});
  }
  c = block_best(c);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = (uint64_t)c.count;
    partial[2 * blockIdx.x + 1] = c.key;
  }
}

// second launch: one workgroup over the n_partial partials; the result and the table's counters
__global__ __launch_bounds__(kThreads) void k_pair_best_final(Table T, const uint64_t* partial, uint32_t n_partial,
                                                              Best* out) {
  pbest::Cand c = pbest::kNone;
  for (uint32_t i = threadIdx.x; i < n_partial; i += kThreads)
    c = pbest::best_of(c, pbest::Cand{(int64_t)partial[2 * i], partial[2 * i + 1]});
  c = block_best(c);
  if (threadIdx.x == 0) {
    out->count = c.count > 0 ? c.count : 0;
    out->key = c.key;
    out->taken = T.ctr[kCtrTaken];
    out->overflow = T.ctr[kCtrOverflow];
  }
}

// merge_pair for (a, b) -> nid: thread per word.  A word without an occurrence is only read.  A
// word with one takes all its adjacent pairs out of the table, is rewritten in place by a read and
// a write cursor (the reference's loop: i += 2 after a merge, so `a a a` with (a, a) gives `aa a`),
// and puts its new adjacent pairs in: the table equals a fresh count of the words after every
// merge, and (a, b) ends at 0 by itself.
__global__ __launch_bounds__(kThreads) void k_bpe_merge(Words W, Table T, uint32_t a, uint32_t b, uint32_t nid) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < W.n_words; w += gridDim.x * kThreads) {
    const uint32_t n = W.wlen[w];
    if (n < 2) continue;
    uint32_t* t = W.tok + W.wstart[w];
    bool found = false;
    for (uint32_t i = 0; i + 1 < n && !found; i++) found = t[i] == a && t[i + 1] == b;
    if (!found) continue;
    const int64_t f = (int64_t)W.wfreq[w];
    if (f)
      for (uint32_t i = 0; i + 1 < n; i++) table_add(T, pbest::pair_key(t[i], t[i + 1]), -f);
    uint32_t r = 0, m = 0;
    while (r < n) {
      if (r + 1 < n && t[r] == a && t[r + 1] == b) {
        t[m++] = nid;
        r += 2;
      } else {
        t[m++] = t[r++];
      }
    }
    W.wlen[w] = m;
    if (f)
      for (uint32_t i = 0; i + 1 < m; i++) table_add(T, pbest::pair_key(t[i], t[i + 1]), f);
  }
}

// ---- launchers -------------------------------------------------------------------------------------

hipError_t launch_ws_bits(const uint8_t* text, uint32_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                          uint32_t* pbits, hipStream_t s) {
  const uint32_t n_words = (uint32_t)(((uint64_t)n_bytes + 31) / 32);
  if (!n_words) return hipSuccess;
  k_ws_bits<<<grid_for(n_words, 8192), kThreads, 0, s>>>(text, n_bytes, n_words, pbits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !n_docs) return e;
  k_ws_doc_starts<<<grid_for(n_docs, 8192), kThreads, 0, s>>>(doc_off, n_docs, n_bytes, pbits);
  return hipGetLastError();
}

hipError_t launch_pair_count(const Words& W, const Table& T, hipStream_t s) {
  if (W.n_words) k_pair_count<<<grid_for(W.n_words, 8192), kThreads, 0, s>>>(W, T);
  return hipGetLastError();
}

hipError_t launch_pair_best(const Table& T, uint64_t* partial, Best* out, hipStream_t s) {
  const uint32_t blocks = grid_for(T.cap, kBestBlocks);
  k_pair_best_partial<<<blocks, kThreads, 0, s>>>(T, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_pair_best_final<<<1, kThreads, 0, s>>>(T, partial, blocks, out);
  return hipGetLastError();
}

hipError_t launch_merge(const Words& W, const Table& T, uint32_t a, uint32_t b, uint32_t nid, hipStream_t s) {
  if (W.n_words) k_bpe_merge<<<grid_for(W.n_words, 8192), kThreads, 0, s>>>(W, T, a, b, nid);
  return hipGetLastError();
}

}  // namespace ctok_bpe
