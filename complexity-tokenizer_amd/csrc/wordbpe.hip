// HIP kernels (gfx950) of the id-keyed word BPE behind include/ctok_pipeline.h: the last stage of
// PipelineTokenizer, over the packed words a PreTokenizer run leaves on the device.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   HuggingFaceTokenizer::encode     src/huggingface/mod.rs:551-613  the added-token loop inside a word
//   find_added_token                 src/huggingface/mod.rs:637-675  first occurrence, three checks
//   BpeTokenizer::encode_with_dropout(0)  src/bpe.rs:88-153  chars -> ids, lowest rank, leftmost, one merge a step
// Stages: word-start bits -> (with added tokens) match bits, the segments counted and written ->
// keep bits, their scan, the initial ids -> segment sizes and classes -> the merge loop in three
// tiers -> count, scan, emit.  The tiers are strmerge.hip's in shape and meaning:
//   <= kTier1 symbols   a thread per segment, ids and cached ranks in thread-interleaved LDS columns
//   <= kTier2 symbols   a wavefront per segment, a linked list and a rank cache in its LDS; a round is
//                       a wave-min of the rank, a wave-min of the position and one merge
//   above               the same wave code over global-memory state (agent-scope loads and stores)
// New here: every rank lookup tests the panic mark (wordbpe_hd.h); a segment that sees a marked pair
// stops, leaves the pair's rank at the head of its symbols and enters its index in ctr[kCtrPanic] with
// atomicMin, so the host reports the first such segment of the lowest-numbered text.
//
// A thread owns a bitmap word, a word, a segment or a text; a wavefront owns a long segment.  Every
// loop is bounded: by the bitmap word, the word's bytes, the added tokens that share a first byte,
// the table's probe bounds, the segment's symbols.  Every byte index is below n_bytes, a char or an
// added token is taken only when no word starts inside it, and every segment lies inside one word,
// so no byte outside the buffers is read whatever the bytes are.  The only hand-off between
// workgroups is the kernel boundary.  No MFMA: integer/hash work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wordbpe_internal.h"

namespace ctok_wb {

using wordbpe::kDead;
using wordbpe::kNoId;
using wordbpe::kNoPanic;
using wordbpe::kNoRank;
using wordbpe::kPanicBit;
using wordbpe::Seg;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortThreads = 128;  // k_wb_short: 2 x kTier1 x 128 u32 of LDS = 32 KiB

static uint32_t grid_for(uint64_t n, uint32_t threads, uint32_t max_grid) {
  const uint64_t g = (n + threads - 1) / threads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ bool bit_at(const uint32_t* bits, uint32_t g) { return (bits[g >> 5] >> (g & 31)) & 1u; }

// does a word start at one of the bytes (p, p + len)?  (p + len <= n_bytes)
__device__ __forceinline__ bool word_starts_inside(const Batch& b, uint32_t p, uint32_t len) {
  for (uint32_t j = 1; j < len; j++)
    if (bit_at(b.wbits, p + j)) return true;
  return false;
}

// ---- word-start bits ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_wb_word_bits(Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_words; w += gridDim.x * kThreads) {
    const uint64_t o = b.word_off[w];
    if (o < b.word_off[w + 1] && o < b.n_bytes) atomicOr(&b.wbits[o >> 5], 1u << (o & 31));
  }
}

// ---- the segments ------------------------------------------------------------------------------------

// mbits: bit g is set when some added token's bytes stand at g inside one word (the filter: a first-
// byte set, then the compare)
__global__ __launch_bounds__(kThreads) void k_wb_match_bits(Tables t, Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w <= b.n_w; w += gridDim.x * kThreads) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 32 && w < b.n_w; j++) {
      const uint64_t g64 = (uint64_t)w * 32 + j;
      if (g64 >= b.n_bytes) break;
      const uint32_t g = (uint32_t)g64;
      const uint32_t c = b.text[g];
      if (!((t.first_byte[c >> 5] >> (c & 31)) & 1u)) continue;
      for (uint32_t i = t.added.group[c]; i < t.added.group[c + 1]; i++) {
        if (!wordbpe::added_at(t.added, i, b.text, g, b.n_bytes)) continue;
        if (word_starts_inside(b, g, t.added.off[i + 1] - t.added.off[i])) continue;
        v |= 1u << j;
        break;
      }
    }
    b.mbits[w] = v;
  }
}

// the word's bytes, clamped into the buffer
__device__ __forceinline__ void word_range(const Batch& b, uint32_t w, uint32_t* wb, uint32_t* we) {
  uint64_t a = b.word_off[w], e = b.word_off[w + 1];
  if (e > b.n_bytes) e = b.n_bytes;
  if (a > e) a = e;
  *wb = (uint32_t)a;
  *we = (uint32_t)e;
}

// thread per word: the number of its segments.  A word without a match bit is one segment; one with
// a match bit runs the literal loop (wordbpe::split_word), unless it is above the work bound: then
// it is counted as one and reported through ctr[kCtrMaxFlagged], and the host refuses the call.
__global__ __launch_bounds__(kThreads) void k_wb_seg_count(Tables t, Batch b) {
  uint32_t top = 0;
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_words; w += gridDim.x * kThreads) {
    uint32_t wb, we;
    word_range(b, w, &wb, &we);
    uint32_t n = 1;
    if (wordbpe::next_candidate(b.mbits, wb, we) < we) {
      if (we - wb > b.flag_cap) top = top > we - wb ? top : we - wb;
      else n = wordbpe::split_word(t.added, b.text, wb, we, b.mbits, nullptr);
    }
    b.wseg[w] = n;
  }
  if (top) atomicMax(&b.ctr[kCtrMaxFlagged], top);
}

__global__ __launch_bounds__(kThreads) void k_wb_seg_write(Tables t, Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_words; w += gridDim.x * kThreads) {
    uint32_t wb, we;
    word_range(b, w, &wb, &we);
    const uint32_t at = b.segoff ? b.segoff[w] : w;
    const uint32_t room = b.segoff ? b.segoff[w + 1] - at : 1u;
    if (at >= b.n_segs || room > b.n_segs - at) continue;  // (cannot happen: segoff is the scan of wseg)
    if (b.mbits && room >= 1 && wordbpe::next_candidate(b.mbits, wb, we) < we && we - wb <= b.flag_cap) {
      // (the same loop as the count, over the same bytes: it writes `room` segments)
      wordbpe::split_word(t.added, b.text, wb, we, b.mbits, b.segs + at);
    } else {
      b.segs[at] = Seg{wb, we};
    }
  }
}

// ---- initial symbols ---------------------------------------------------------------------------------

// the id of the well-formed char at g that lies inside one word and has a one-char vocab string
__device__ __forceinline__ uint32_t char_id(const Tables& t, const Batch& b, uint32_t g) {
  uint32_t cp = 0;
  const uint32_t len = wordbpe::dec_char(b.text, g, b.n_bytes, &cp);
  if (!len || word_starts_inside(b, g, len)) return kNoId;
  return wordbpe::cp_find(t.cps, cp);
}

__global__ __launch_bounds__(kThreads) void k_wb_keep_bits(Tables t, Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w <= b.n_w; w += gridDim.x * kThreads) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 32 && w < b.n_w; j++) {
      const uint64_t g = (uint64_t)w * 32 + j;
      if (g >= b.n_bytes) break;
      if (wordbpe::is_cont(b.text[g])) continue;
      if (char_id(t, b, (uint32_t)g) != kNoId) v |= 1u << j;
    }
    b.kbits[w] = v;
    b.kpc[w] = __popc(v);
  }
}

__global__ __launch_bounds__(kThreads) void k_wb_symbols(Tables t, Batch b) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < b.n_w; w += gridDim.x * kThreads) {
    uint32_t at = b.krank[w];
    for (uint32_t v = b.kbits[w]; v; v &= v - 1) {
      const uint32_t g = w * 32 + (uint32_t)__ffs((int)v) - 1;
      b.sym[at++] = char_id(t, b, g);  // (at < krank[w + 1] <= the kept chars: kbits counted these)
    }
  }
}

// kept chars among the bytes before x (x <= n_bytes)
__device__ __forceinline__ uint32_t kept_before(const Batch& b, uint32_t x) {
  return b.krank[x >> 5] + (uint32_t)__popc(b.kbits[x >> 5] & ((1u << (x & 31)) - 1u));
}

__global__ __launch_bounds__(kThreads) void k_wb_seg_info(Batch b) {
  uint32_t top = 0;
  for (uint32_t s = blockIdx.x * kThreads + threadIdx.x; s < b.n_segs; s += gridDim.x * kThreads) {
    const Seg g = b.segs[s];
    uint32_t n = 0, at = 0;
    if (g.a == kNoId) {
      b.fcnt[s] = 1;
    } else if (g.a <= g.b && g.b <= b.n_bytes) {
      at = kept_before(b, g.a);
      n = kept_before(b, g.b) - at;
      if (!n) b.fcnt[s] = 0;
    } else {
      b.fcnt[s] = 0;  // (cannot happen)
    }
    b.nsym[s] = n;
    b.soff[s] = at;
    if (n > top) top = n;
    if (n > kTier2) {
      const uint32_t k = atomicAdd(&b.ctr[kCtrList3], 1u);
      b.list3[k] = s;  // (room for every segment that can be this long: pipeline_host.cpp)
      b.state3[k] = atomicAdd((unsigned long long*)(b.ctr + kCtrState), (unsigned long long)n);
    } else if (n > kTier1) {
      b.list2[atomicAdd(&b.ctr[kCtrList2], 1u)] = s;
    }
  }
  if (top) atomicMax(&b.ctr[kCtrMaxSym], top);
}

// ---- the panic report --------------------------------------------------------------------------------

// segment s saw a marked pair of rank r (one thread): the rank at the head of its symbols (a segment
// with a pair has two), no ids, and the lowest such segment of the batch
__device__ __forceinline__ void report_panic(const Batch& b, uint32_t s, uint32_t r) {
  b.sym[b.soff[s]] = r;
  b.fcnt[s] = 0;
  atomicMin(&b.ctr[kCtrPanic], s);
}

// ---- tier 1: a thread per segment --------------------------------------------------------------------

__global__ __launch_bounds__(kShortThreads) void k_wb_short(Tables t, Batch b) {
  __shared__ uint32_t s_tok[kTier1 * kShortThreads];
  __shared__ uint32_t s_rank[kTier1 * kShortThreads];
  uint32_t* tok = s_tok + threadIdx.x;
  uint32_t* rank = s_rank + threadIdx.x;
  for (uint32_t s = blockIdx.x * kShortThreads + threadIdx.x; s < b.n_segs; s += gridDim.x * kShortThreads) {
    const uint32_t n = b.nsym[s];
    if (!n || n > kTier1) continue;  // (k_wb_seg_info and the wave tiers write those fcnt)
    uint32_t* io = b.sym + b.soff[s];
    for (uint32_t k = 0; k < n; k++) tok[k * kShortThreads] = io[k];
    uint32_t pr = kNoPanic;
    const uint32_t left = wordbpe::merge_ids(t.pairs, tok, rank, kShortThreads, n, &pr);
    if (pr != kNoPanic) {
      report_panic(b, s, pr);
      continue;
    }
    for (uint32_t k = 0; k < left; k++) io[k] = tok[k * kShortThreads];
    b.fcnt[s] = left;
  }
}

// ---- tiers 2 and 3: a wavefront per segment ----------------------------------------------------------

typedef __attribute__((address_space(3))) uint32_t lds_u32;

// A segment's state: id, next, previous and cached rank per initial position.  GMEM: global memory,
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

// the merge of the pair at position i (one lane); the rank of a marked pair it made adjacent -- the
// left one first, as the reference's next scan meets them -- or kNoPanic
template <bool G>
__device__ __forceinline__ uint32_t merge_at(const Tables& t, const State<G>& L, uint32_t i, uint32_t n) {
  const uint32_t j = L.ld(L.nxt + i);
  if (j >= n) {  // (cannot happen: a position with a rank has a right neighbour)
    L.st(L.rk + i, kNoRank);
    return kNoPanic;
  }
  const uint32_t nj = L.ld(L.nxt + j);
  const uint32_t sym = strmerge::pair_find(t.pairs, L.ld(L.tok + i), L.ld(L.tok + j)).sym;
  L.st(L.tok + i, sym);
  L.st(L.tok + j, kDead);
  L.st(L.rk + j, kNoRank);
  L.st(L.nxt + i, nj);
  uint32_t panic = kNoPanic;
  const uint32_t h = L.ld(L.prv + i);
  if (h < n) {
    const uint32_t r = strmerge::pair_find(t.pairs, L.ld(L.tok + h), sym).rank;
    if (wordbpe::is_panic(r)) panic = r & ~kPanicBit;
    L.st(L.rk + h, r);
  }
  uint32_t right = kNoRank;
  if (nj < n) {
    L.st(L.prv + nj, i);
    right = strmerge::pair_find(t.pairs, sym, L.ld(L.tok + nj)).rank;
    if (panic == kNoPanic && wordbpe::is_panic(right)) panic = right & ~kPanicBit;
  }
  L.st(L.rk + i, right);
  return panic;
}

template <bool G>
__device__ __forceinline__ void wave_segment(const Tables& t, const Batch& b, const State<G>& L, uint32_t s) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = b.nsym[s];
  uint32_t* io = b.sym + b.soff[s];
  for (uint32_t k = lane; k < n; k += 64) L.st(L.tok + k, io[k]);
  L.sync();
  uint32_t ppos = kNoRank;  // this lane's leftmost marked pair
  for (uint32_t k = lane; k < n; k += 64) {
    L.st(L.nxt + k, k + 1);
    L.st(L.prv + k, k ? k - 1 : kDead);
    const uint32_t r = k + 1 < n ? strmerge::pair_find(t.pairs, L.ld(L.tok + k), L.ld(L.tok + k + 1)).rank : kNoRank;
    if (wordbpe::is_panic(r) && ppos == kNoRank) ppos = k;
    L.st(L.rk + k, r);
  }
  L.sync();
  const uint32_t first = wave_min(ppos);
  if (first != kNoRank) {  // (uniform: the first scan of the reference meets this pair)
    if (lane == 0) report_panic(b, s, L.ld(L.rk + first) & ~kPanicBit);
    L.sync();
    return;
  }
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
    uint32_t pr = kNoPanic;
    if (lane == 0) pr = merge_at(t, L, at, n);
    pr = (uint32_t)__shfl((int)pr, 0, 64);
    if (pr != kNoPanic) {  // (uniform)
      if (lane == 0) report_panic(b, s, pr);
      L.sync();
      return;
    }
    L.sync();
  }
  // the ids left, in order, over the head of the segment's own symbols (the state is apart from them)
  uint32_t cnt = 0;
  for (uint32_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t k = k0 + lane;
    const uint32_t v = k < n ? L.ld(L.tok + k) : kDead;
    const unsigned long long mask = __ballot(v != kDead);
    if (v != kDead) io[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = v;
    cnt += (uint32_t)__popcll(mask);
  }
  if (lane == 0) b.fcnt[s] = cnt;
  L.sync();  // (the state is the next segment's)
}

__global__ __launch_bounds__(64) void k_wb_wave_lds(Tables t, Batch b, uint32_t n_list) {
  __shared__ uint32_t s_state[4 * kTier2];
  lds_u32* lds = (lds_u32*)s_state;
  const State<false> L{lds, lds + kTier2, lds + 2 * kTier2, lds + 3 * kTier2};
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t s = b.list2[i];
    if (s < b.n_segs && b.nsym[s] <= kTier2) wave_segment<false>(t, b, L, s);
  }
}

__global__ __launch_bounds__(64) void k_wb_wave_gmem(Tables t, Batch b, uint32_t n_list) {
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t s = b.list3[i];
    if (s >= b.n_segs) continue;
    const uint64_t n = b.nsym[s];
    uint32_t* g = b.state + 4 * b.state3[i];
    const State<true> L{g, g + n, g + 2 * n, g + 3 * n};
    wave_segment<true>(t, b, L, s);
  }
}

// ---- emit --------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_wb_emit(Batch b, uint32_t* ids) {
  for (uint32_t s = blockIdx.x * kThreads + threadIdx.x; s < b.n_segs; s += gridDim.x * kThreads) {
    const uint32_t n = b.fcnt[s];
    if (!n) continue;
    uint32_t* out = ids + b.wpos[s];
    const Seg g = b.segs[s];
    if (g.a == kNoId) {
      out[0] = g.b;
      continue;
    }
    const uint32_t* v = b.sym + b.soff[s];
    for (uint32_t k = 0; k < n; k++) out[k] = v[k];
  }
}

// tok_off[i] = the ids before text i's first word
__global__ __launch_bounds__(kThreads) void k_wb_tokoff(Batch b, uint64_t* tok_off) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i <= b.n_texts; i += (uint64_t)gridDim.x * kThreads) {
    uint64_t w = b.text_word[i];
    if (w > b.n_words) w = b.n_words;
    uint32_t s = b.segoff ? b.segoff[w] : (uint32_t)w;
    if (s > b.n_segs) s = b.n_segs;
    tok_off[i] = b.wpos[s];
  }
}

__global__ __launch_bounds__(kThreads) void k_wb_iota(uint64_t* p, uint64_t n) {
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) p[i] = i;
}

// ---- launchers ---------------------------------------------------------------------------------------

hipError_t launch_word_bits(const Batch& b, hipStream_t s) {
  if (b.n_words) k_wb_word_bits<<<grid_for(b.n_words, kThreads, 8192), kThreads, 0, s>>>(b);
  return hipGetLastError();
}

hipError_t launch_match_bits(const Tables& t, const Batch& b, hipStream_t s) {
  k_wb_match_bits<<<grid_for((uint64_t)b.n_w + 1, kThreads, 8192), kThreads, 0, s>>>(t, b);
  return hipGetLastError();
}

hipError_t launch_seg_count(const Tables& t, const Batch& b, hipStream_t s) {
  if (b.n_words) k_wb_seg_count<<<grid_for(b.n_words, kThreads, 8192), kThreads, 0, s>>>(t, b);
  return hipGetLastError();
}

hipError_t launch_seg_write(const Tables& t, const Batch& b, hipStream_t s) {
  if (b.n_words) k_wb_seg_write<<<grid_for(b.n_words, kThreads, 8192), kThreads, 0, s>>>(t, b);
  return hipGetLastError();
}

hipError_t launch_keep_bits(const Tables& t, const Batch& b, hipStream_t s) {
  k_wb_keep_bits<<<grid_for((uint64_t)b.n_w + 1, kThreads, 8192), kThreads, 0, s>>>(t, b);
  return hipGetLastError();
}

hipError_t launch_symbols(const Tables& t, const Batch& b, hipStream_t s) {
  if (b.n_w) k_wb_symbols<<<grid_for(b.n_w, kThreads, 8192), kThreads, 0, s>>>(t, b);
  return hipGetLastError();
}

hipError_t launch_seg_info(const Batch& b, hipStream_t s) {
  if (b.n_segs) k_wb_seg_info<<<grid_for(b.n_segs, kThreads, 8192), kThreads, 0, s>>>(b);
  return hipGetLastError();
}

hipError_t launch_merge(const Tables& t, const Batch& b, uint32_t n2, uint32_t n3, hipStream_t s) {
  if (!b.n_segs) return hipSuccess;
  k_wb_short<<<grid_for(b.n_segs, kShortThreads, 8192), kShortThreads, 0, s>>>(t, b);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n2) {
    k_wb_wave_lds<<<n2 < 4096 ? n2 : 4096, 64, 0, s>>>(t, b, n2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n3) k_wb_wave_gmem<<<n3 < 4096 ? n3 : 4096, 64, 0, s>>>(t, b, n3);
  return hipGetLastError();
}

hipError_t launch_emit(const Batch& b, uint32_t* ids, uint64_t* tok_off, hipStream_t s) {
  if (b.n_segs) {
    k_wb_emit<<<grid_for(b.n_segs, kThreads, 8192), kThreads, 0, s>>>(b, ids);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  k_wb_tokoff<<<grid_for(b.n_texts + 1, kThreads, 8192), kThreads, 0, s>>>(b, tok_off);
  return hipGetLastError();
}

hipError_t launch_iota(uint64_t* p, uint64_t n, hipStream_t s) {
  if (n) k_wb_iota<<<grid_for(n, kThreads, 8192), kThreads, 0, s>>>(p, n);
  return hipGetLastError();
}

}  // namespace ctok_wb
