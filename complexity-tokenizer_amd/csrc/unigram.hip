// HIP kernels (gfx950) of the Unigram trainer and model (include/ctok_unigram.h).
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3): UnigramTrainer, src/trainers.rs:287-546,
// and UnigramModel::tokenize, src/models.rs:225-269.  Both run a Viterbi search whose inner loop
// builds a String per (start, end) pair and looks it up in a HashMap.  Here the lookups and the
// search are two steps with a kernel boundary between them:
//
//   k_meta_*      Metaspace after NFC: a thread owns 64 input bytes, measures, and after the host's
//                 two scans writes the sentence bytes behind each other and the sentences' offsets
//   k_sent_bits / k_lead / k_sent_chars   the sentence-start bitmap, the char starts (their scan is
//                 the char index of every byte) and every sentence's first char
//   k_sub_count   thread per char start: its substrings of 1 .. max_piece_length chars into the
//                 count table of wordcount_hd.h (one CAS per new string, one atomic add per
//                 occurrence; a chunk that overflows is counted again by the host)
//   k_lattice     thread per char start: FNV-1a char by char, one probe of the string table per
//                 boundary (unigram_hd.h matches); lat[j][c] = symbol of the j + 1 chars at c.
//                 n x window independent probes, no chain.  Built once per training: the vocab
//                 only shrinks, so an iteration changes score[] and live[] and nothing here
//   k_viterbi     a wavefront per sentence, ends in order, lanes over the candidate starts of one
//                 end: best[start] + score[sym] from the last window's best values in an LDS ring,
//                 a butterfly that keeps the maximum and among equal sums the smallest start
//                 (unigram_hd.h takes), (length, symbol) per end to global memory
//   k_back_*      thread per sentence walks the back pointers: the trainer adds 1 to count[sym], the
//                 model counts its ids and, after a scan, writes them
//
// The kernel boundary is the only ordering between kernels; inside k_viterbi a workgroup is one
// wavefront and __syncthreads orders the ring.  Every loop is bounded: walks by the sentence and
// the window, probes by wptab::kMaxProbe and the count table's kMaxProbe, back walks by the
// sentence's chars.  A back pointer of 0 (nothing reaches the position) ends the walk and sets a
// flag; nothing is read at index -1.  The only f64 operation is the add of a step, so there is
// nothing to contract or reassociate.  No MFMA: integer, hash and compare work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "unigram_hd.h"
#include "unigram_internal.h"
#include "wordcount_hd.h"

namespace ctok_uni {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxProbe = 4096;

static uint32_t grid_for(uint64_t n, uint32_t per_block, uint32_t max_grid) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

// ---- Metaspace -------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_meta_measure(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                                                           uint64_t n_docs, uint64_t n_spans, uint64_t* len,
                                                           uint64_t* nsent) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t b0 = i * uni::kSpan, b1 = b0 + uni::kSpan < n_bytes + 1 ? b0 + uni::kSpan : n_bytes + 1;
    uint64_t o, k;
    uni::meta_range(text, n_bytes, doc_off, n_docs, b0, b1, nullptr, 0, nullptr, &o, &k);
    len[i] = o;
    nsent[i] = k;
  }
}

__global__ __launch_bounds__(kThreads) void k_meta_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off,
                                                         uint64_t n_docs, uint64_t n_spans, const uint64_t* len,
                                                         const uint64_t* nsent, uint8_t* out, uint64_t* sent_off) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n_spans; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t b0 = i * uni::kSpan, b1 = b0 + uni::kSpan < n_bytes + 1 ? b0 + uni::kSpan : n_bytes + 1;
    uint64_t o, k;
    uni::meta_range(text, n_bytes, doc_off, n_docs, b0, b1, out + len[i], len[i], sent_off + nsent[i], &o, &k);
  }
}

hipError_t launch_meta_measure(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                               uint64_t* len, uint64_t* nsent, hipStream_t s) {
  const uint64_t n_spans = meta_spans(n_bytes);
  k_meta_measure<<<grid_for(n_spans, kThreads, 16384), kThreads, 0, s>>>(text, n_bytes, doc_off, n_docs, n_spans, len, nsent);
  return hipGetLastError();
}

hipError_t launch_meta_write(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint64_t n_docs,
                             const uint64_t* len, const uint64_t* nsent, uint8_t* out, uint64_t* sent_off, hipStream_t s) {
  const uint64_t n_spans = meta_spans(n_bytes);
  k_meta_write<<<grid_for(n_spans, kThreads, 16384), kThreads, 0, s>>>(text, n_bytes, doc_off, n_docs, n_spans, len, nsent,
                                                                      out, sent_off);
  return hipGetLastError();
}

// ---- sentences -------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_sent_bits(Sents x, uint32_t* bits) {
  for (uint64_t k = blockIdx.x * kThreads + threadIdx.x; k < x.n_sent; k += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = x.sent_off[k];
    if (o < x.n_bytes && x.sent_off[k + 1] > o) atomicOr(&bits[o >> 5], 1u << (o & 31));
  }
}

__global__ __launch_bounds__(kThreads) void k_lead(Sents x, uint32_t* lead) {
  for (uint64_t p = blockIdx.x * kThreads + threadIdx.x; p < x.n_bytes; p += (uint64_t)gridDim.x * kThreads)
    lead[p] = uni::is_lead(x.text[p]) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void k_sent_chars(Sents x, const uint32_t* cidx, uint32_t* sent_c) {
  for (uint64_t k = blockIdx.x * kThreads + threadIdx.x; k <= x.n_sent; k += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = x.sent_off[k];
    sent_c[k] = cidx[o < x.n_bytes ? o : x.n_bytes];  // (cidx has n_bytes + 1 entries)
  }
}

hipError_t launch_sent_bits(const Sents& x, uint32_t* bits, hipStream_t s) {
  if (x.n_sent) k_sent_bits<<<grid_for(x.n_sent, kThreads, 8192), kThreads, 0, s>>>(x, bits);
  return hipGetLastError();
}
hipError_t launch_lead_flags(const Sents& x, uint32_t* lead, hipStream_t s) {
  if (x.n_bytes) k_lead<<<grid_for(x.n_bytes, kThreads, 16384), kThreads, 0, s>>>(x, lead);
  return hipGetLastError();
}
hipError_t launch_sent_chars(const Sents& x, const uint32_t* cidx, uint32_t* sent_c, hipStream_t s) {
  k_sent_chars<<<grid_for(x.n_sent + 1, kThreads, 8192), kThreads, 0, s>>>(x, cidx, sent_c);
  return hipGetLastError();
}

// ---- substring counts ------------------------------------------------------------------------------
// Wait-free as k_wc_count: a slot is claimed by one 64-bit compare-and-swap of a complete
// descriptor; whoever loses compares against the immutable text.

__device__ __forceinline__ void sub_add(const uint8_t* text, const ctok_wc::Table& t, uint32_t pos, uint32_t len) {
  const uint64_t hash = wc::word_hash(text, pos, len);
  const uint32_t tag = (uint32_t)hash & 0xFFFFu;
  const uint64_t mine = wc::pack(pos, len, tag);
  uint32_t h = (uint32_t)(hash >> 32) & t.mask;
  const uint32_t tries = min(t.mask, kMaxProbe - 1u) + 1u;
  for (uint32_t i = 0; i < tries; i++, h = (h + 1) & t.mask) {
    uint64_t k = t.keys[h];
    if (k == wc::kEmpty) {
      k = atomicCAS((unsigned long long*)&t.keys[h], (unsigned long long)wc::kEmpty, (unsigned long long)mine);
      if (k == wc::kEmpty) {
        t.used[atomicAdd(&t.ctr[ctok_wc::kCtrUsed], 1u)] = h;  // (one entry per slot: < capacity)
        k = mine;
      }
    }
    if (k == mine || (wc::may_match(k, len, tag) && wc::words_equal(text, pos, wc::pos_of(k), len))) {
      atomicAdd(&t.vals[h], 1u);  // (a string occurs once per position: < 2^32 per chunk)
      return;
    }
  }
  atomicOr(&t.ctr[ctok_wc::kCtrOverflow], 1u);
}

__global__ __launch_bounds__(kThreads) void k_sub_count(Sents x, const uint32_t* bits, uint64_t max_chars, ctok_wc::Table t) {
  for (uint64_t p = blockIdx.x * kThreads + threadIdx.x; p < x.n_bytes; p += (uint64_t)gridDim.x * kThreads) {
    if (!uni::is_lead(x.text[p])) continue;
    if (__hip_atomic_load(&t.ctr[ctok_wc::kCtrOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    uni::substrings(x.text, x.n_bytes, bits, p, max_chars, [&](uint64_t e) {
      const uint64_t len = e - p;
      if (len >= wc::kLenClip) atomicOr(&t.ctr[ctok_wc::kCtrOverflow], 2u);
      else sub_add(x.text, t, (uint32_t)p, (uint32_t)len);
    });
  }
}

__global__ __launch_bounds__(kThreads) void k_sub_drain(ctok_wc::Table t, uint32_t n_used, uint32_t* pos, uint32_t* len,
                                                        uint32_t* cnt) {
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n_used; i += gridDim.x * kThreads) {
    const uint32_t h = t.used[i] & t.mask;
    const uint64_t k = t.keys[h];
    pos[i] = wc::pos_of(k);
    len[i] = wc::len_of(k);
    cnt[i] = t.vals[h];
  }
}

hipError_t launch_sub_count(const Sents& x, const uint32_t* bits, uint64_t max_chars, const ctok_wc::Table& t, hipStream_t s) {
  if (x.n_bytes && max_chars) k_sub_count<<<grid_for(x.n_bytes, kThreads, 16384), kThreads, 0, s>>>(x, bits, max_chars, t);
  return hipGetLastError();
}

hipError_t launch_sub_drain(const ctok_wc::Table& t, uint32_t n_used, uint32_t* pos, uint32_t* len, uint32_t* cnt,
                            hipStream_t s) {
  if (n_used) k_sub_drain<<<grid_for(n_used, kThreads, 8192), kThreads, 0, s>>>(t, n_used, pos, len, cnt);
  return hipGetLastError();
}

// ---- lattice ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_lattice(Sents x, const uint32_t* bits, const uint32_t* cidx, wptab::View v,
                                                      uint32_t wl, uint32_t n_chars, uint32_t* lat) {
  for (uint64_t p = blockIdx.x * kThreads + threadIdx.x; p < x.n_bytes; p += (uint64_t)gridDim.x * kThreads) {
    if (!uni::is_lead(x.text[p])) continue;
    const uint32_t c = cidx[p];
    if (c >= n_chars) continue;
    uint32_t next = 0;  // the rows below `next` are written
    uni::matches(v, x.text, x.n_bytes, bits, p, wl, [&](uint32_t j, uint32_t sym) {
      for (; next < j; next++) lat[(uint64_t)next * n_chars + c] = uni::kNone;
      lat[(uint64_t)j * n_chars + c] = sym;
      next = j + 1;
    });
    for (; next < wl; next++) lat[(uint64_t)next * n_chars + c] = uni::kNone;
  }
}

hipError_t launch_lattice(const Sents& x, const uint32_t* bits, const uint32_t* cidx, const wptab::View& v, uint32_t wl,
                          uint32_t n_chars, uint32_t* lat, hipStream_t s) {
  if (x.n_bytes && wl) k_lattice<<<grid_for(x.n_bytes, kThreads, 16384), kThreads, 0, s>>>(x, bits, cidx, v, wl, n_chars, lat);
  return hipGetLastError();
}

// ---- Viterbi ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_viterbi(Viterbi a, uint32_t ring_mask) {
  extern __shared__ double ring[];  // best[pos] at ring[pos & ring_mask]; ring_mask + 1 >= wv + 2
  const uint32_t lane = threadIdx.x;
  const double ninf = -__builtin_inf();
  for (uint64_t k = blockIdx.x; k < a.n_sent; k += gridDim.x) {
    const uint32_t c0 = a.sent_c[k], c1 = a.sent_c[k + 1];
    if (c1 <= c0 || c1 > a.n_chars) continue;  // (the same for the whole wavefront)
    const uint32_t n = c1 - c0;
    __syncthreads();  // the sentence before is done with the ring
    if (lane == 0) ring[0] = 0.0;
    __syncthreads();
    for (uint32_t e = 1; e <= n; e++) {
      // the best candidate so far: its sum, its length - 1, its symbol.  Three scalars that move under
      // one predicate: as a struct assigned in a branch, the compiled code left the symbol behind when
      // a lane replaced its candidate on an equal sum
      double b_sum = ninf;
      uint32_t b_j = 0, b_sym = uni::kNone;
      const uint32_t w = a.wv < e ? a.wv : e;
      for (uint32_t j = lane; j < w; j += 64) {  // the token of j + 1 chars that ends at e
        const uint32_t st = e - j - 1;
        uint32_t sym = j < a.wl ? a.lat[(uint64_t)j * a.n_chars + c0 + st] : uni::kNone;
        if (sym != uni::kNone && a.live && !a.live[sym]) sym = uni::kNone;
        double sc;
        if (sym != uni::kNone) {
          sc = a.score[sym];
        } else if (j == 0) {
          sc = a.fb_score;
          sym = a.fb_sym;
        } else {
          continue;
        }
        const double sum = ring[st & ring_mask] + sc;
        const bool take = uni::takes(sum, j, b_sum, b_j);
        b_sum = take ? sum : b_sum;
        b_j = take ? j : b_j;
        b_sym = take ? sym : b_sym;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double sum = __shfl_xor(b_sum, o, 64);
        const uint32_t j = __shfl_xor(b_j, o, 64), sym = __shfl_xor(b_sym, o, 64);
        const bool take = uni::takes(sum, j, b_sum, b_j);
        b_sum = take ? sum : b_sum;
        b_j = take ? j : b_j;
        b_sym = take ? sym : b_sym;
      }
      if (lane == 0) {
        const bool reached = b_sum > ninf;
        ring[e & ring_mask] = reached ? b_sum : ninf;
        a.back_len[c0 + e - 1] = reached ? b_j + 1 : 0u;
        a.back_sym[c0 + e - 1] = b_sym;
      }
      __syncthreads();
    }
  }
}

hipError_t launch_viterbi(const Viterbi& a, hipStream_t s) {
  if (!a.n_sent || !a.n_chars) return hipSuccess;
  if (a.wv > kMaxWindow) return hipErrorInvalidValue;
  uint32_t ring = 4;
  while (ring < a.wv + 2) ring <<= 1;
  const uint32_t grid = (uint32_t)(a.n_sent < 32768 ? a.n_sent : 32768);
  k_viterbi<<<grid, 64, ring * sizeof(double), s>>>(a, ring - 1);
  return hipGetLastError();
}

// One sentence's back walk, from its last char: each(sym) per token in reverse order.  Returns 0,
// 1 (a position nothing reaches: each was not called for it) or 2 (a pointer past the start).
template <typename Each>
__device__ __forceinline__ uint32_t back_walk(const Viterbi& a, uint32_t c0, uint32_t c1, Each each) {
  uint32_t pos = c1 - c0;
  while (pos > 0) {  // (pos falls by >= 1 per round)
    const uint32_t len = a.back_len[c0 + pos - 1];
    if (!len) return 1;
    if (len > pos) return 2;
    each(a.back_sym[c0 + pos - 1]);
    pos -= len;
  }
  return 0;
}

__global__ __launch_bounds__(kThreads) void k_back_train(Viterbi a, unsigned long long* count, uint32_t* err) {
  for (uint64_t k = blockIdx.x * kThreads + threadIdx.x; k < a.n_sent; k += (uint64_t)gridDim.x * kThreads) {
    const uint32_t c0 = a.sent_c[k], c1 = a.sent_c[k + 1];
    if (c1 <= c0 || c1 > a.n_chars) continue;
    const uint32_t rc = back_walk(a, c0, c1, [&](uint32_t sym) {
      if (sym != uni::kNone) atomicAdd(&count[sym], 1ull);
    });
    if (rc) atomicOr(err, rc);
  }
}

__global__ __launch_bounds__(kThreads) void k_back_count(Viterbi a, uint32_t* cnt) {
  for (uint64_t k = blockIdx.x * kThreads + threadIdx.x; k < a.n_sent; k += (uint64_t)gridDim.x * kThreads) {
    const uint32_t c0 = a.sent_c[k], c1 = a.sent_c[k + 1];
    uint32_t n = 0;
    if (c1 > c0 && c1 <= a.n_chars && back_walk(a, c0, c1, [&](uint32_t) { n++; }) == 1) n++;  // (the id 0 of the quirk)
    cnt[k] = n;
  }
}

__global__ __launch_bounds__(kThreads) void k_back_emit(Viterbi a, const uint32_t* pos, uint32_t* ids, uint64_t* tok_off) {
  for (uint64_t k = blockIdx.x * kThreads + threadIdx.x; k <= a.n_sent; k += (uint64_t)gridDim.x * kThreads) {
    tok_off[k] = pos[k];
    if (k == a.n_sent) continue;
    const uint32_t c0 = a.sent_c[k], c1 = a.sent_c[k + 1];
    if (c1 <= c0 || c1 > a.n_chars) continue;
    const uint32_t lo = pos[k];
    uint32_t at = pos[k + 1];  // written from the back; never below lo: the same walk counted them
    const uint32_t rc = back_walk(a, c0, c1, [&](uint32_t sym) {
      if (at > lo) ids[--at] = sym;
    });
    if (rc == 1 && at > lo) ids[--at] = 0;
  }
}

hipError_t launch_back_train(const Viterbi& a, unsigned long long* count, uint32_t* err, hipStream_t s) {
  if (a.n_sent && a.n_chars) k_back_train<<<grid_for(a.n_sent, kThreads, 8192), kThreads, 0, s>>>(a, count, err);
  return hipGetLastError();
}
hipError_t launch_back_count(const Viterbi& a, uint32_t* cnt, hipStream_t s) {
  if (a.n_sent) k_back_count<<<grid_for(a.n_sent, kThreads, 8192), kThreads, 0, s>>>(a, cnt);
  return hipGetLastError();
}
hipError_t launch_back_emit(const Viterbi& a, const uint32_t* pos, uint32_t* ids, uint64_t* tok_off, hipStream_t s) {
  k_back_emit<<<grid_for(a.n_sent + 1, kThreads, 8192), kThreads, 0, s>>>(a, pos, ids, tok_off);
  return hipGetLastError();
}

}  // namespace ctok_uni
