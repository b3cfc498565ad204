// HIP kernels (gfx950) of the WordPiece trainer and model behind include/ctok_wordpiece.h.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   tokenize_for_training  src/trainers.rs:228-273  greedy longest match      -> k_wp_match, k_wp_add, k_wp_walk_train
//   the pair counts        src/trainers.rs:182-190  (a, b) -> sum of freqs     -> k_wp_walk_train on the resident table
//   max_by_key             src/trainers.rs:197-199                              -> bpe_train.hip k_pair_best, unchanged
//   tokenize_word, encode  src/models.rs:52-106                                 -> k_wp_match, k_wp_walk_model
// The reference tokenises every word against the whole vocab before every merge.  The vocab only
// grows, by one string per round, so the longest match at a position after a round is the longer
// of the match before it and the new string, where that matches: k_wp_match runs once per training
// and k_wp_add compares one string per round.  Words whose matches changed are walked again, and
// the walk moves their pairs in the resident pair table (pair_table_dev.h), so the table equals a
// fresh count of the words after every round.
//
// A thread owns a byte position (match, add) or a word (walk); a position's match is written by
// its own thread only, dirty flags are plain stores of 1, pair counts are the table's 64-bit
// atomics.  Every loop is bounded: a match by the longest pattern and the table's probe bound, an
// add by the new string, a walk by its word.  The only hand-off between workgroups is the kernel
// boundary.  No MFMA: integer/hash work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pair_best_hd.h"
#include "pair_table_dev.h"
#include "wordpiece_internal.h"
#include "ws_split_hd.h"

namespace ctok_wp {

constexpr uint32_t kThreads = 256;

static uint32_t grid_for(uint64_t n, uint32_t max_grid) {
  const uint64_t g = (n + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

// ---- matches ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_wp_match(Text x, wptab::View v, uint32_t skip_ws, Matches m) {
  for (uint64_t g = blockIdx.x * kThreads + threadIdx.x; g < x.n_bytes; g += (uint64_t)gridDim.x * kThreads) {
    const uint32_t p = (uint32_t)g;  // (the index is 64-bit: n_bytes may be within a stride of 2^32)
    wptab::Match r = {wptab::kNone, 0};
    if (!wsplit::is_cont(x.text[p]) && !(skip_ws && wsplit::ws_at(x.text, x.n_bytes, p)))
      r = wptab::longest(v, x.text, x.n_bytes, x.starts, p, wptab::bit_at(x.starts, p) ? 0u : 1u);
    m.msym[p] = r.sym;
    m.mlen[p] = r.len;
  }
}

// the word of byte p: the last w with woff[w] <= p (woff[0] = 0, n_words >= 1)
__device__ __forceinline__ uint32_t word_of(const uint32_t* woff, uint32_t n_words, uint32_t p) {
  uint32_t lo = 0, hi = n_words;  // woff[lo] <= p < woff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (woff[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_wp_add(Text x, const uint8_t* pat0, uint32_t len0, const uint8_t* pat1,
                                                     uint32_t len1, uint32_t sym, uint32_t relabel, Matches m,
                                                     const uint32_t* woff, uint32_t n_words, uint32_t* dirty) {
  for (uint64_t g = blockIdx.x * kThreads + threadIdx.x; g < x.n_bytes; g += (uint64_t)gridDim.x * kThreads) {
    const uint32_t p = (uint32_t)g;
    if (wsplit::is_cont(x.text[p])) continue;
    const bool first = wptab::bit_at(x.starts, p);
    const uint8_t* pat = first ? pat0 : pat1;
    const uint32_t len = first ? len0 : len1;
    if (!len || len > x.n_bytes - p) continue;
    // a longer match replaces the stored one; an equal one only the fallback token of the same
    // string (the new string is prefix + char: `relabel` is that char's fallback symbol)
    const uint32_t have = m.mlen[p];
    if (len < have || (len == have && m.msym[p] != relabel)) continue;
    uint32_t j = 0;
    while (j < len && x.text[p + j] == pat[j]) j++;
    if (j < len) continue;
    // inside the word: no word starts in (p, p + len), and p + len is a code-point boundary
    bool inside = p + len == x.n_bytes || !wsplit::is_cont(x.text[p + len]);
    for (uint32_t q = p + 1; q < p + len && inside; q++) inside = !wptab::bit_at(x.starts, q);
    if (!inside) continue;
    m.msym[p] = sym;
    m.mlen[p] = len;
    dirty[word_of(woff, n_words, p)] = 1u;
  }
}

// ---- the trainer's walk ------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_wp_walk_train(const uint32_t* woff, Matches m, Words W, Table T,
                                                            uint32_t update, uint32_t* dirty, uint32_t all,
                                                            unsigned long long* stat) {
  uint32_t walked = 0;
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < W.n_words; w += gridDim.x * kThreads) {
    if (!all && !dirty[w]) continue;
    dirty[w] = 0;
    walked++;
    const int64_t f = update ? (int64_t)W.wfreq[w] : 0;
    uint32_t* t = W.tok + W.wstart[w];
    const uint32_t room = W.wstart[w + 1] - W.wstart[w];
    const uint32_t n_old = W.wlen[w];
    if (f)
      for (uint32_t i = 0; i + 1 < n_old; i++) ctok_bpe::table_add(T, pbest::pair_key(t[i], t[i + 1]), -f);
    const uint32_t e = woff[w + 1];
    uint32_t p = woff[w], n = 0;
    while (p < e) {
      const uint32_t s = m.msym[p], l = m.mlen[p];
      if (s == wptab::kNone || !l || l > e - p || n >= room) {  // (cannot happen: every char has a pattern)
        atomicOr(&stat[0], 1ull);
        break;
      }
      t[n++] = s;
      p += l;
    }
    W.wlen[w] = n;
    if (f)
      for (uint32_t i = 0; i + 1 < n; i++) ctok_bpe::table_add(T, pbest::pair_key(t[i], t[i + 1]), f);
  }
  // statistics: the words walked, one 64-bit add per workgroup (every thread gets here)
  __shared__ uint32_t s_walked;
  if (threadIdx.x == 0) s_walked = 0;
  __syncthreads();
  if (walked) atomicAdd(&s_walked, walked);
  __syncthreads();
  if (threadIdx.x == 0 && s_walked) atomicAdd(&stat[1], (unsigned long long)s_walked);
}

// ---- the model's walk --------------------------------------------------------------------------------

// the ids of the word that starts at byte p (a set start bit on a non-whitespace code point);
// EMIT: written to out, else only counted
template <bool EMIT>
__device__ __forceinline__ uint32_t walk_word(const Text& x, const Matches& m, uint32_t p, uint64_t max_chars,
                                              uint32_t has_unk, uint32_t unk_id, uint32_t* out) {
  uint32_t e = p;
  uint64_t chars = 0;
  do {  // the word's end and its chars
    const uint32_t l = wptab::cp_len(x.text[e]);
    e = l > x.n_bytes - e ? x.n_bytes : e + l;
    chars++;
  } while (e < x.n_bytes && !wptab::bit_at(x.starts, e));
  uint32_t n = 0;
  if (chars > max_chars) {
    if (has_unk) {
      if (EMIT) out[0] = unk_id;
      n = 1;
    }
    return n;
  }
  uint32_t q = p;
  while (q < e) {
    const uint32_t s = m.msym[q], l = m.mlen[q];
    if (s != wptab::kNone && l && l <= e - q) {
      if (EMIT) out[n] = s;
      n++;
      q += l;
    } else {
      if (has_unk) {
        if (EMIT) out[n] = unk_id;
        n++;
      }
      const uint32_t c = wptab::cp_len(x.text[q]);
      q = c > e - q ? e : q + c;
    }
  }
  return n;
}

__device__ __forceinline__ bool word_start(const Text& x, uint32_t p) {
  return wptab::bit_at(x.starts, p) && !wsplit::is_cont(x.text[p]) && !wsplit::ws_at(x.text, x.n_bytes, p);
}

__global__ __launch_bounds__(kThreads) void k_wp_walk_model_count(Text x, Matches m, uint64_t max_chars, uint32_t has_unk,
                                                                  uint32_t* cnt) {
  for (uint64_t g = blockIdx.x * kThreads + threadIdx.x; g < x.n_bytes; g += (uint64_t)gridDim.x * kThreads) {
    const uint32_t p = (uint32_t)g;
    cnt[p] = word_start(x, p) ? walk_word<false>(x, m, p, max_chars, has_unk, 0, nullptr) : 0u;
  }
}

__global__ __launch_bounds__(kThreads) void k_wp_walk_model_emit(Text x, Matches m, uint64_t max_chars, uint32_t has_unk,
                                                                 uint32_t unk_id, const uint32_t* pos, uint32_t* ids) {
  for (uint64_t g = blockIdx.x * kThreads + threadIdx.x; g < x.n_bytes; g += (uint64_t)gridDim.x * kThreads) {
    const uint32_t p = (uint32_t)g;
    if (word_start(x, p) && pos[g + 1] > pos[p]) walk_word<true>(x, m, p, max_chars, has_unk, unk_id, ids + pos[p]);
  }
}

__global__ __launch_bounds__(kThreads) void k_wp_tokoff(const uint64_t* doc_off, uint64_t n_docs, const uint32_t* pos,
                                                        uint32_t n_bytes, uint64_t* tok_off) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = doc_off[d];
    tok_off[d] = pos[o < n_bytes ? o : n_bytes];
  }
}

// ---- launchers -------------------------------------------------------------------------------------

hipError_t launch_match(const Text& x, const wptab::View& v, bool skip_ws, const Matches& m, hipStream_t s) {
  if (x.n_bytes) k_wp_match<<<grid_for(x.n_bytes, 16384), kThreads, 0, s>>>(x, v, skip_ws ? 1u : 0u, m);
  return hipGetLastError();
}

hipError_t launch_add(const Text& x, const uint8_t* pat0, uint32_t len0, const uint8_t* pat1, uint32_t len1,
                      uint32_t sym, uint32_t relabel, const Matches& m, const uint32_t* woff, uint32_t n_words,
                      uint32_t* dirty, hipStream_t s) {
  if (x.n_bytes && n_words)
    k_wp_add<<<grid_for(x.n_bytes, 16384), kThreads, 0, s>>>(x, pat0, len0, pat1, len1, sym, relabel, m, woff,
                                                             n_words, dirty);
  return hipGetLastError();
}

hipError_t launch_walk_train(const uint32_t* woff, const Matches& m, const Words& W, const Table* T, uint32_t* dirty,
                             bool all, unsigned long long* stat, hipStream_t s) {
  if (W.n_words)
    k_wp_walk_train<<<grid_for(W.n_words, 8192), kThreads, 0, s>>>(woff, m, W, T ? *T : Table{nullptr, nullptr, 0, nullptr},
                                                                   T ? 1u : 0u, dirty, all ? 1u : 0u, stat);
  return hipGetLastError();
}

hipError_t launch_model_count(const Text& x, const Matches& m, uint64_t max_chars, uint32_t has_unk, uint32_t* cnt,
                              hipStream_t s) {
  if (x.n_bytes) k_wp_walk_model_count<<<grid_for(x.n_bytes, 16384), kThreads, 0, s>>>(x, m, max_chars, has_unk, cnt);
  return hipGetLastError();
}

hipError_t launch_model_emit(const Text& x, const Matches& m, uint64_t max_chars, uint32_t has_unk, uint32_t unk_id,
                             const uint32_t* pos, uint32_t* ids, const uint64_t* doc_off, uint64_t n_docs,
                             uint64_t* tok_off, hipStream_t s) {
  if (x.n_bytes) {
    k_wp_walk_model_emit<<<grid_for(x.n_bytes, 16384), kThreads, 0, s>>>(x, m, max_chars, has_unk, unk_id, pos, ids);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  k_wp_tokoff<<<grid_for(n_docs + 1, 8192), kThreads, 0, s>>>(doc_off, n_docs, pos, x.n_bytes, tok_off);
  return hipGetLastError();
}

}  // namespace ctok_wp
