// HIP kernels (gfx950) of the string-keyed merge engine behind include/ctok_models.h: the encode of
// WordLevelModel, CharBpeModel and ByteLevelBpeModel.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   WordLevelModel::encode     src/models.rs:331-337  split_whitespace, one lookup per word
//   ByteLevelBpeModel::encode  src/models.rs:520-557  a word at byte 0 and at every U+0020
//   CharBpeModel::encode       src/models.rs:695-705  split_whitespace, last char + suffix
//   tokenize_word              src/models.rs:471-517, :644-692  the merge loop (strmerge_hd.h)
// Stages: start bits -> the run list (runs, symbol counts, three classes by symbol count) -> the
// initial symbols and the merge loop in three tiers -> count, scan, emit.  The tiers have one
// meaning, the literal loop "lowest rank, leftmost, one merge per step":
//   <= kTier1 symbols   a thread per word, tokens and cached ranks in thread-interleaved LDS columns
//   <= kTier2 symbols   a wavefront per word, a linked list and a rank cache in its LDS; a round is a
//                       wave-min of the rank, a wave-min of the position and one merge
//   above               the same wave code over global-memory state (agent-scope loads and stores)
//
// A thread owns a bitmap word, a run or a text; a wavefront owns a long word.  Every loop is
// bounded: by the bitmap word, the run's bytes or symbols, the table's probe bound, log2 of the
// texts.  Every text index is below n_bytes and every run ends where the next begins, so no byte
// outside the buffers is read whatever the bytes are, and no word runs across a text boundary
// (every non-empty text's first byte has a start bit).  The only hand-off between workgroups is
// the kernel boundary.  No MFMA: integer/hash work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "strmerge_compile.h"  // strmerge::Kind
#include "strmerge_internal.h"
#include "ws_split_hd.h"

namespace ctok_sm {

using strmerge::kDead;
using strmerge::kNoRank;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortThreads = 128;  // k_sm_short: 2 x kTier1 x 128 u32 of LDS = 32 KiB

static uint32_t grid_for(uint64_t n, uint32_t threads, uint32_t max_grid) {
  const uint64_t g = (n + threads - 1) / threads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ bool bit_at(const uint32_t* bits, uint32_t g) { return (bits[g >> 5] >> (g & 31)) & 1u; }

// ---- start bits --------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_sm_byte_bits(Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_w; w += gridDim.x * kThreads) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 32; j++) {
      const uint64_t g = (uint64_t)w * 32 + j;
      if (g < b.n_bytes && b.text[g] == 0x20u) v |= 1u << j;
    }
    b.bits[w] = v;
    b.dbits[w] = 0;
  }
}

// thread per text: a non-empty text's first byte.  Runs after k_sm_byte_bits (the kernel boundary
// orders it behind that kernel's plain stores); texts that share a bitmap word meet in an atomic OR.
__global__ __launch_bounds__(kThreads) void k_sm_doc_bits(Batch b) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d < b.n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = b.doc_off[d];
    if (o < b.doc_off[d + 1] && o < b.n_bytes) {
      atomicOr(&b.bits[o >> 5], 1u << (o & 31));
      atomicOr(&b.dbits[o >> 5], 1u << (o & 31));
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_sm_popc(Batch b, uint32_t* pc, uint32_t* cpc) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_w; w += gridDim.x * kThreads) {
    pc[w] = __popc(b.bits[w]);
    if (cpc) {
      uint32_t c = 0;
      for (uint32_t j = 0; j < 32; j++) {
        const uint64_t g = (uint64_t)w * 32 + j;
        if (g < b.n_bytes && !wsplit::is_cont(b.text[g])) c++;
      }
      cpc[w] = c;
    }
  }
}

// ---- the run list ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_sm_runs(Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w <= b.n_w; w += gridDim.x * kThreads) {
    uint32_t r = b.wrank[w];
    if (w == b.n_w) {
      b.runs[r] = b.n_bytes;
      continue;
    }
    for (uint32_t v = b.bits[w]; v; v &= v - 1) b.runs[r++] = w * 32 + (uint32_t)__ffs((int)v) - 1;
  }
}

// code-point starts among the bytes before x (x <= n_bytes)
__device__ __forceinline__ uint32_t chars_before(const Batch& b, uint32_t x) {
  uint32_t c = b.crank[x >> 5];
  for (uint32_t g = x & ~31u; g < x; g++) c += wsplit::is_cont(b.text[g]) ? 0u : 1u;
  return c;
}

// does the byte-level word at p get the virtual leading space?  (a text's first word, when the
// text does not start with U+0020; src/models.rs:523-527)
__device__ __forceinline__ bool virtual_space(const Model& m, const Batch& b, uint32_t p) {
  return m.prefix_space && bit_at(b.dbits, p) && b.text[p] != 0x20u;
}

__global__ __launch_bounds__(kThreads) void k_sm_word_info(Model m, Batch b, uint32_t n_runs) {
  uint32_t top = 0;
  for (uint32_t r = blockIdx.x * kThreads + threadIdx.x; r < n_runs; r += gridDim.x * kThreads) {
    const uint32_t p = b.runs[r], e = b.runs[r + 1];
    uint32_t n = 0;
    if (p < e && e <= b.n_bytes) {
      if (m.kind == strmerge::kByteLevel) n = e - p + (virtual_space(m, b, p) ? 1u : 0u);
      else if (wsplit::is_cont(b.text[p]) || wsplit::ws_at(b.text, b.n_bytes, p)) n = 0;
      else if (m.kind == strmerge::kWordLevel) n = 1;
      else n = chars_before(b, e) - chars_before(b, p);
    }
    b.nsym[r] = n;
    if (n > top) top = n;
    if (n > kTier2) {
      const uint32_t k = atomicAdd(&b.ctr[kCtrList3], 1u);
      b.list3[k] = r;  // (room for every run that can be this long: models_host.cpp)
      b.state3[k] = atomicAdd((unsigned long long*)(b.ctr + kCtrState), (unsigned long long)n);
    } else if (n > kTier1) {
      b.list2[atomicAdd(&b.ctr[kCtrList2], 1u)] = r;
    }
  }
  if (top) atomicMax(&b.ctr[kCtrMaxSym], top);
}

// ---- initial symbols ---------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t byte_sym(const Model& m, const Batch& b, uint32_t p, bool virt, uint32_t k) {
  if (virt) return m.byte2sym[k ? b.text[p + k - 1] : 0x20u];
  return m.byte2sym[b.text[p + k]];
}

// the symbol of the string text[q .. q + len) in `form`, or the foreign symbol
__device__ __forceinline__ uint32_t string_sym(const Model& m, const Batch& b, uint32_t q, uint32_t len, uint32_t form) {
  if (!len || len > m.strings.max_len) return m.foreign;
  uint32_t h = wptab::kSeed;
  for (uint32_t j = 0; j < len; j++) h = wptab::step(h, b.text[q + j]);
  const uint32_t s = wptab::find(m.strings, b.text + q, len, h, form);
  return s == wptab::kNone ? m.foreign : s;
}

// the char that starts at q (a code-point start) inside the word that ends at e: its bytes run to
// the next code-point start.  A char of more than 4 bytes (not UTF-8) is foreign.
__device__ __forceinline__ uint32_t char_sym(const Model& m, const Batch& b, uint32_t q, uint32_t e, bool last) {
  uint32_t r = q + 1;
  while (r < e && r - q < 5 && wsplit::is_cont(b.text[r])) r++;
  return r - q > 4 ? m.foreign : string_sym(m, b, q, r - q, last ? 1u : 0u);
}

// ---- tier 1: a thread per word ---------------------------------------------------------------------

__global__ __launch_bounds__(kShortThreads) void k_sm_short(Model m, Batch b, uint32_t n_runs) {
  __shared__ uint32_t s_tok[kTier1 * kShortThreads];
  __shared__ uint32_t s_rank[kTier1 * kShortThreads];
  uint32_t* tok = s_tok + threadIdx.x;
  uint32_t* rank = s_rank + threadIdx.x;
  for (uint32_t r = blockIdx.x * kShortThreads + threadIdx.x; r < n_runs; r += gridDim.x * kShortThreads) {
    const uint32_t n = b.nsym[r];
    if (n > kTier1) continue;  // (the wave tiers write fcnt)
    if (!n) {
      b.fcnt[r] = 0;
      continue;
    }
    const uint32_t p = b.runs[r], e = b.runs[r + 1];
    if (m.kind == strmerge::kByteLevel) {
      const bool virt = virtual_space(m, b, p);
      for (uint32_t k = 0; k < n; k++) tok[k * kShortThreads] = byte_sym(m, b, p, virt, k);
    } else if (m.kind == strmerge::kWordLevel) {
      tok[0] = string_sym(m, b, p, e - p, 0);
    } else {
      uint32_t k = 0;
      for (uint32_t q = p; q < e && k < n; q++)
        if (!wsplit::is_cont(b.text[q])) {
          tok[k * kShortThreads] = char_sym(m, b, q, e, k + 1 == n);
          k++;
        }
      for (; k < n; k++) tok[k * kShortThreads] = m.foreign;  // (cannot happen: n counted these starts)
    }
    const uint32_t left = strmerge::merge_word(m.pairs, tok, rank, kShortThreads, n);
    uint32_t* out = b.tok + b.soff[r];
    for (uint32_t k = 0; k < left; k++) out[k] = tok[k * kShortThreads];
    b.fcnt[r] = left;
  }
}

// ---- tiers 2 and 3: a wavefront per word -----------------------------------------------------------

typedef __attribute__((address_space(3))) uint32_t lds_u32;

// A word's state: token, next, previous and cached rank per initial position.  GMEM: global memory,
// every access an agent-scope relaxed atomic, so the lanes of the wave see each other's stores
// between rounds (the vector L1 does not); else the wave's LDS.
template <bool GMEM>
struct State;

template <>
struct State<true> {
  uint32_t *tok, *nxt, *prv, *rk;
  static __device__ __forceinline__ uint32_t ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
  }
};

template <>
struct State<false> {
  lds_u32 *tok, *nxt, *prv, *rk;
  static __device__ __forceinline__ uint32_t ld(const lds_u32* p) { return *p; }
  static __device__ __forceinline__ void st(lds_u32* p, uint32_t v) { *p = v; }
  static __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
    v = u < v ? u : v;
  }
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// the merge of the pair at position i (one lane)
template <bool G>
__device__ __forceinline__ void merge_at(const Model& m, const State<G>& L, uint32_t i, uint32_t n) {
  const uint32_t j = L.ld(L.nxt + i);
  if (j >= n) {  // (cannot happen: a position with a rank has a right neighbour)
    L.st(L.rk + i, kNoRank);
    return;
  }
  const uint32_t nj = L.ld(L.nxt + j);
  const uint32_t sym = strmerge::pair_find(m.pairs, L.ld(L.tok + i), L.ld(L.tok + j)).sym;
  L.st(L.tok + i, sym);
  L.st(L.tok + j, kDead);
  L.st(L.rk + j, kNoRank);
  L.st(L.nxt + i, nj);
  uint32_t right = kNoRank;
  if (nj < n) {
    L.st(L.prv + nj, i);
    right = strmerge::pair_find(m.pairs, sym, L.ld(L.tok + nj)).rank;
  }
  L.st(L.rk + i, right);
  const uint32_t h = L.ld(L.prv + i);
  if (h < n) L.st(L.rk + h, strmerge::pair_find(m.pairs, L.ld(L.tok + h), sym).rank);
}

template <bool G>
__device__ __forceinline__ void wave_word(const Model& m, const Batch& b, const State<G>& L, uint32_t r) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = b.nsym[r], p = b.runs[r], e = b.runs[r + 1];
  // the initial symbols
  if (m.kind == strmerge::kByteLevel) {
    const bool virt = virtual_space(m, b, p);
    for (uint32_t k = lane; k < n; k += 64) L.st(L.tok + k, byte_sym(m, b, p, virt, k));
  } else {
    uint32_t base = 0;  // chars before this stretch of 64 bytes
    for (uint32_t q0 = p; q0 < e; q0 += 64) {  // (uniform: every lane takes every turn)
      const uint32_t q = q0 + lane;
      const bool start = q < e && !wsplit::is_cont(b.text[q]);
      const unsigned long long mask = __ballot(start);
      const uint32_t k = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (start && k < n) L.st(L.tok + k, char_sym(m, b, q, e, k + 1 == n));
      base += (uint32_t)__popcll(mask);
    }
    for (uint32_t k = base + lane; k < n; k += 64) L.st(L.tok + k, m.foreign);  // (cannot happen)
  }
  L.sync();
  for (uint32_t k = lane; k < n; k += 64) {
    L.st(L.nxt + k, k + 1);
    L.st(L.prv + k, k ? k - 1 : kDead);
    L.st(L.rk + k, k + 1 < n ? strmerge::pair_find(m.pairs, L.ld(L.tok + k), L.ld(L.tok + k + 1)).rank : kNoRank);
  }
  L.sync();
  // one merge per round: the lowest rank, the leftmost of its positions
  for (uint32_t round = 0; round + 1 < n; round++) {
    uint32_t lmin = kNoRank, lpos = kNoRank;
    for (uint32_t k = lane; k < n; k += 64) {
      const uint32_t x = L.ld(L.rk + k);
      if (x < lmin) lmin = x, lpos = k;
    }
    const uint32_t best = wave_min(lmin);
    if (best == kNoRank) break;
    const uint32_t at = wave_min(lmin == best ? lpos : kNoRank);
    if (at >= n) break;  // (cannot happen)
    if (lane == 0) merge_at(m, L, at, n);
    L.sync();
  }
  // the tokens left, in order
  uint32_t* out = b.tok + b.soff[r];
  uint32_t cnt = 0;
  for (uint32_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t k = k0 + lane;
    const uint32_t t = k < n ? L.ld(L.tok + k) : kDead;
    const unsigned long long mask = __ballot(t != kDead);
    if (t != kDead) out[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = t;
    cnt += (uint32_t)__popcll(mask);
  }
  if (lane == 0) b.fcnt[r] = cnt;
  L.sync();  // (the state is the next word's)
}

__global__ __launch_bounds__(64) void k_sm_wave_lds(Model m, Batch b, uint32_t n_list) {
  __shared__ uint32_t s_state[4 * kTier2];
  lds_u32* lds = (lds_u32*)s_state;
  const State<false> L{lds, lds + kTier2, lds + 2 * kTier2, lds + 3 * kTier2};
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t r = b.list2[i];
    if (b.nsym[r] <= kTier2) wave_word<false>(m, b, L, r);
  }
}

__global__ __launch_bounds__(64) void k_sm_wave_gmem(Model m, Batch b, uint32_t n_list) {
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t r = b.list3[i];
    const uint64_t n = b.nsym[r];
    uint32_t* g = b.state + 4 * b.state3[i];
    const State<true> L{g, g + n, g + 2 * n, g + 3 * n};
    wave_word<true>(m, b, L, r);
  }
}

// ---- emit ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_sm_empty_flags(Batch b, uint32_t* flag) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d < b.n_docs; d += (uint64_t)gridDim.x * kThreads)
    flag[d] = b.doc_off[d] >= b.doc_off[d + 1] ? 1u : 0u;
}

// the text of byte p: the last d < n_docs with doc_off[d] <= p (doc_off[0] = 0; of the texts that
// start at one byte, the last is the one that is not empty)
__device__ __forceinline__ uint64_t doc_of(const Batch& b, uint32_t p) {
  uint64_t lo = 0, hi = b.n_docs;  // doc_off[lo] <= p < doc_off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (b.doc_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_sm_emit(Model m, Batch b, uint32_t n_runs, uint32_t* ids) {
  for (uint32_t r = blockIdx.x * kThreads + threadIdx.x; r < n_runs; r += gridDim.x * kThreads) {
    const uint32_t n = b.fcnt[r];
    if (!n) continue;
    const uint32_t* t = b.tok + b.soff[r];
    uint32_t* out = ids + b.wpos[r] + (b.empty_before ? b.empty_before[doc_of(b, b.runs[r])] : 0u);
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t s = t[k];
      out[k] = m.sym_id[s < m.foreign ? s : m.foreign];
    }
  }
}

// tok_off[d] = the ids before text d: those of the runs before its first byte and one per empty
// text before it (byte-level with the prefix space: an empty text is the one-symbol word " ")
__global__ __launch_bounds__(kThreads) void k_sm_tokoff(Model m, Batch b, uint32_t n_runs, uint32_t* ids, uint64_t* tok_off) {
  for (uint64_t d = blockIdx.x * kThreads + threadIdx.x; d <= b.n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = b.doc_off[d];
    uint32_t r = n_runs;
    if (o < b.n_bytes) {
      const uint32_t g = (uint32_t)o;
      r = b.wrank[g >> 5] + __popc(b.bits[g >> 5] & ((1u << (g & 31)) - 1u));
      if (r > n_runs) r = n_runs;
    }
    const uint64_t at = (uint64_t)b.wpos[r] + (b.empty_before ? b.empty_before[d] : 0u);
    tok_off[d] = at;
    if (b.empty_before && d < b.n_docs && o >= b.doc_off[d + 1]) ids[at] = m.sym_id[m.byte2sym[0x20]];
  }
}

// ---- launchers -------------------------------------------------------------------------------------

hipError_t launch_byte_starts(const Batch& b, hipStream_t s) {
  if (!b.n_w) return hipSuccess;
  k_sm_byte_bits<<<grid_for(b.n_w, kThreads, 8192), kThreads, 0, s>>>(b);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !b.n_docs) return e;
  k_sm_doc_bits<<<grid_for(b.n_docs, kThreads, 8192), kThreads, 0, s>>>(b);
  return hipGetLastError();
}

hipError_t launch_popc(const Batch& b, uint32_t* pc, uint32_t* cpc, hipStream_t s) {
  if (b.n_w) k_sm_popc<<<grid_for(b.n_w, kThreads, 8192), kThreads, 0, s>>>(b, pc, cpc);
  return hipGetLastError();
}

hipError_t launch_runs(const Batch& b, hipStream_t s) {
  k_sm_runs<<<grid_for((uint64_t)b.n_w + 1, kThreads, 8192), kThreads, 0, s>>>(b);
  return hipGetLastError();
}

hipError_t launch_word_info(const Model& m, const Batch& b, uint32_t n_runs, hipStream_t s) {
  if (n_runs) k_sm_word_info<<<grid_for(n_runs, kThreads, 8192), kThreads, 0, s>>>(m, b, n_runs);
  return hipGetLastError();
}

hipError_t launch_merge(const Model& m, const Batch& b, uint32_t n_runs, uint32_t n2, uint32_t n3, hipStream_t s) {
  if (!n_runs) return hipSuccess;
  k_sm_short<<<grid_for(n_runs, kShortThreads, 8192), kShortThreads, 0, s>>>(m, b, n_runs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n2) {
    k_sm_wave_lds<<<n2 < 4096 ? n2 : 4096, 64, 0, s>>>(m, b, n2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n3) k_sm_wave_gmem<<<n3 < 4096 ? n3 : 4096, 64, 0, s>>>(m, b, n3);
  return hipGetLastError();
}

hipError_t launch_empty_flags(const Batch& b, uint32_t* flag, hipStream_t s) {
  if (b.n_docs) k_sm_empty_flags<<<grid_for(b.n_docs, kThreads, 8192), kThreads, 0, s>>>(b, flag);
  return hipGetLastError();
}

hipError_t launch_emit(const Model& m, const Batch& b, uint32_t n_runs, uint32_t* ids, uint64_t* tok_off, hipStream_t s) {
  if (n_runs) {
    k_sm_emit<<<grid_for(n_runs, kThreads, 8192), kThreads, 0, s>>>(m, b, n_runs, ids);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  k_sm_tokoff<<<grid_for(b.n_docs + 1, kThreads, 8192), kThreads, 0, s>>>(m, b, n_runs, ids, tok_off);
  return hipGetLastError();
}

}  // namespace ctok_sm
