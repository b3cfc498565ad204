// HIP kernels (gfx950) of the PreTokenizer (pretok_hd.h: the reference's src/pretokenizers.rs:69-594).
//
// A thread owns one byte and a wavefront the 64 bytes of one bitmap word: the lanes' answers become
// the word by one ballot, which lane 0 stores.  The steps fall into two families.
//   Pure splitters never touch a byte: k_pt_split maps (in_word, begin) to new bitmaps, every lane by
//   split_bits() from the old bitmaps and a bounded neighbourhood of its byte.  What a rule needs from
//   farther away is made by kernels before it: the literal matches (k_pt_cand marks candidates,
//   k_pt_chain walks chains of overlapping ones), the matches of a general pattern (k_pt_dfa_len runs
//   its DFA from every lead byte, k_pt_dfa_tail / k_pt_dfa_carry / k_pt_dfa_chain resolve the
//   leftmost non-overlapping ones by a prefix max of the matches' ends), whether a word holds a match (k_pt_hit, by the
//   word's ordinal from a scan of the begin counts), and the script carry of UnicodeScripts: "the last
//   script value before me" is the nearest lower lane that has one (ballot, lane read), else the
//   wavefront's running value, which starts from the carry of the wavefront tiles before
//   (k_pt_script_tail per tile, k_pt_script_carry over the tiles by one workgroup).
//   Rewriters (ByteLevel, Metaspace) count per bitmap word (k_pt_rw_count), the host scans, and
//   k_pt_rw_write places every lane's bytes by a prefix sum over the wavefront, with a begin flag per
//   output byte that k_pt_pack ballots into the new bitmaps.
// The final gather is the same count / scan / write over the in_word and begin bits.
// No kernel waits on another workgroup; within a kernel no thread writes what another reads; every
// loop is bounded by the text (the chain walk by its chain) and a long word is the work of as many
// threads as it has bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#define PT_DATA_ATTR __device__
#include "gen/pretok_data.h"
#include "ctok_internal.h"  // ctok_dev::scan_u64
#include "pretok_hd.h"
#include "pretok_internal.h"

namespace ctok_pt {

using pretok::Ctx;
using pretok::Step;
using pretok::Tables;

static uint32_t grid_for(uint64_t n_threads, uint32_t max_grid = 1u << 18) {
  const uint64_t g = (n_threads + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ Tables with_nd(Tables T) {
  T.nd_lo = pt_nd_lo;
  T.nd_hi = pt_nd_hi;
  T.n_nd = PT_N_ND;
  return T;
}
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint64_t wave_id() { return ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6; }
__device__ __forceinline__ uint64_t n_waves() { return (uint64_t)gridDim.x * (kThreads / 64); }
__device__ __forceinline__ uint64_t below(uint32_t lane) { return (1ull << lane) - 1; }
// the value of the highest lane of m (m != 0): the same for every lane
__device__ __forceinline__ uint32_t top_of(uint64_t m, uint32_t v) { return (uint32_t)__shfl((int)v, 63 - __clzll((long long)m), 64); }

__global__ __launch_bounds__(kThreads) void k_pt_init(uint64_t n, uint64_t nw, Bits out) {
  for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < nw; j += (uint64_t)gridDim.x * kThreads) {
    out.inw[j] = n - j * 64 >= 64 ? ~0ull : below((uint32_t)(n - j * 64));
    out.beg[j] = 0;
  }
}

// (after k_pt_init: the only writers of beg are these atomics)
__global__ __launch_bounds__(kThreads) void k_pt_doc_begin(const uint64_t* doc_off, uint64_t n_docs, uint64_t n,
                                                           uint64_t* beg) {
  for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = doc_off[d];
    if (o < doc_off[d + 1] && o < n) atomicOr((unsigned long long*)&beg[o >> 6], 1ull << (o & 63));
  }
}

__global__ __launch_bounds__(kThreads) void k_pt_split(Tables T0, Step st, Ctx x, uint64_t nw, Bits out) {
  const Tables T = with_nd(T0);
  for (uint64_t j = wave_id(); j < nw; j += n_waves()) {
    const uint64_t p = j * 64 + lane_id();
    bool in = false, bg = false;
    if (p < x.n) pretok::split_bits(T, st, x, p, 0, &in, &bg);
    const uint64_t mi = __ballot(in), mb = __ballot(bg);
    if (lane_id() == 0) {
      out.inw[j] = mi;
      out.beg[j] = mb;
    }
  }
}

// ---- UnicodeScripts ------------------------------------------------------------------------------------

// tail[t] = the last non-zero script value of wavefront tile t, 0 when it has none
__global__ __launch_bounds__(kThreads) void k_pt_script_tail(Ctx x, uint64_t n_tiles, uint8_t* tail) {
  for (uint64_t t = wave_id(); t < n_tiles; t += n_waves()) {
    uint32_t last = 0;
    for (uint32_t k = 0; k < kWaveWords; k++) {
      const uint64_t p = (t * kWaveWords + k) * 64 + lane_id();
      const uint32_t v = p < x.n ? pretok::script_val(x, p) : 0;
      const uint64_t m = __ballot(v != 0);
      if (m) last = top_of(m, v);
    }
    if (lane_id() == 0) tail[t] = (uint8_t)last;
  }
}

// carry[t] = the last non-zero tail before tile t: one workgroup, kThreads tiles a round
__global__ __launch_bounds__(kThreads) void k_pt_script_carry(const uint8_t* tail, uint64_t n_tiles, uint8_t* carry) {
  __shared__ uint32_t wave_last[kThreads / 64];
  __shared__ uint32_t run;
  if (threadIdx.x == 0) run = 0;
  __syncthreads();
  const uint32_t w = threadIdx.x >> 6;
  for (uint64_t base = 0; base < n_tiles; base += kThreads) {
    const uint64_t t = base + threadIdx.x;
    const uint32_t v = t < n_tiles ? tail[t] : 0;
    const uint64_t m = __ballot(v != 0), lower = m & below(lane_id());
    const uint32_t near = (uint32_t)__shfl((int)v, lower ? 63 - __clzll((long long)lower) : 0, 64);
    const uint32_t top = m ? top_of(m, v) : 0;
    if (lane_id() == 0) wave_last[w] = top;
    __syncthreads();
    uint32_t pv = lower ? near : 0;
    for (int k = (int)w - 1; k >= 0 && !pv; k--) pv = wave_last[k];
    if (!pv) pv = run;
    if (t < n_tiles) carry[t] = (uint8_t)pv;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = kThreads / 64 - 1; k >= 0; k--)
        if (wave_last[k]) {
          run = wave_last[k];
          break;
        }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void k_pt_script(Tables T0, Step st, Ctx x, uint64_t n_tiles, const uint8_t* carry,
                                                        Bits out) {
  const Tables T = with_nd(T0);
  for (uint64_t t = wave_id(); t < n_tiles; t += n_waves()) {
    uint32_t run = carry[t];
    for (uint32_t k = 0; k < kWaveWords; k++) {
      const uint64_t j = t * kWaveWords + k, p = j * 64 + lane_id();
      if (j * 64 >= x.n) break;  // (the same for every lane)
      const uint32_t v = p < x.n ? pretok::script_val(x, p) : 0;
      const uint64_t m = __ballot(v != 0), lower = m & below(lane_id());
      const uint32_t near = (uint32_t)__shfl((int)v, lower ? 63 - __clzll((long long)lower) : 0, 64);
      bool in = false, bg = false;
      if (p < x.n) pretok::split_bits(T, st, x, p, lower ? near : run, &in, &bg);
      const uint64_t mi = __ballot(in), mb = __ballot(bg);
      if (lane_id() == 0) {
        out.inw[j] = mi;
        out.beg[j] = mb;
      }
      if (m) run = top_of(m, v);
    }
  }
}

// ---- `split`: literal matches, words that hold a match -------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_pt_cand(Step st, Ctx x, uint8_t* cand) {
  for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < x.n; p += (uint64_t)gridDim.x * kThreads)
    cand[p] = pretok::lit_cand(st, x, p) ? 1 : 0;
}

// (st.cand is k_pt_cand's finished array; mark is zero before the kernel and only chain walkers
// write it, each inside its own chain)
__global__ __launch_bounds__(kThreads) void k_pt_chain(Step st, uint64_t n, uint8_t* mark) {
  for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kThreads)
    pretok::lit_chain(st, n, p, mark);
}

// ---- `split`: DFA matches --------------------------------------------------------------------------------

// len[p] = the match that starts at byte p (dfa_len); *over = the lowest start that passes the cap.
// kLds: every workgroup first copies the transition table (at most kDfaLdsBytes) into LDS.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_pt_dfa_len(Tables T0, Step st, Ctx x, uint32_t* len, uint32_t* over) {
  __shared__ uint16_t tab[kLds ? kDfaLdsBytes / 2 : 1];
  const uint16_t* trans = st.dfa.trans;
  if (kLds) {
    const uint32_t ne = st.dfa.n_states * st.dfa.n_symbols;
    for (uint32_t i = threadIdx.x; i < ne && i < kDfaLdsBytes / 2; i += kThreads) tab[i] = st.dfa.trans[i];
    __syncthreads();
    trans = tab;
  }
  const Tables T = with_nd(T0);
  for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < x.n; p += (uint64_t)gridDim.x * kThreads) {
    bool ov;
    len[p] = pretok::dfa_len(T, st.dfa, trans, x, p, &ov);
    if (ov) atomicMin(over, (uint32_t)p);
  }
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {  // the maximum of this lane and the lanes below
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane_id() >= (uint32_t)o && u > v) v = u;
  }
  return v;
}
// where the match that starts at p ends; 0: none starts there
__device__ __forceinline__ uint32_t match_end(const uint32_t* len, uint64_t n, uint64_t p) {
  return p < n && len[p] ? (uint32_t)p + len[p] : 0;
}

// tmax[t] = the largest match end of wavefront tile t
__global__ __launch_bounds__(kThreads) void k_pt_dfa_tail(const uint32_t* len, uint64_t n, uint64_t n_tiles, uint32_t* tmax) {
  for (uint64_t t = wave_id(); t < n_tiles; t += n_waves()) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < kWaveWords; k++) {
      const uint32_t e = match_end(len, n, (t * kWaveWords + k) * 64 + lane_id());
      if (e > m) m = e;
    }
    m = (uint32_t)__shfl((int)wave_incl_max(m), 63, 64);
    if (lane_id() == 0) tmax[t] = m;
  }
}

// carry[t] = the largest tmax before tile t: one workgroup, kThreads tiles a round
__global__ __launch_bounds__(kThreads) void k_pt_dfa_carry(const uint32_t* tmax, uint64_t n_tiles, uint32_t* carry) {
  __shared__ uint32_t wave_max[kThreads / 64];
  __shared__ uint32_t run;
  if (threadIdx.x == 0) run = 0;
  __syncthreads();
  const uint32_t w = threadIdx.x >> 6;
  for (uint64_t base = 0; base < n_tiles; base += kThreads) {
    const uint64_t t = base + threadIdx.x;
    const uint32_t inc = wave_incl_max(t < n_tiles ? tmax[t] : 0);
    const uint32_t up = (uint32_t)__shfl_up((int)inc, 1, 64);
    if (lane_id() == 63) wave_max[w] = inc;
    __syncthreads();
    uint32_t pv = lane_id() ? up : 0;
    for (uint32_t k = 0; k < w; k++) pv = wave_max[k] > pv ? wave_max[k] : pv;
    if (run > pv) pv = run;
    if (t < n_tiles) carry[t] = pv;
    __syncthreads();
    if (threadIdx.x == 0)
      for (uint32_t k = 0; k < kThreads / 64; k++)
        if (wave_max[k] > run) run = wave_max[k];
    __syncthreads();
  }
}

// Every chain head walks its chain (dfa_walk).  reach(p), the largest match end before p, is the
// tile's carry, the wavefront's running maximum and the lanes below.  (mark is zero before the
// kernel and only the walkers write it, each inside its own chain.)
__global__ __launch_bounds__(kThreads) void k_pt_dfa_chain(const uint32_t* len, uint64_t n, uint64_t n_tiles,
                                                           const uint32_t* carry, uint8_t* mark) {
  for (uint64_t t = wave_id(); t < n_tiles; t += n_waves()) {
    uint32_t run = carry[t];
    for (uint32_t k = 0; k < kWaveWords; k++) {
      const uint64_t p = (t * kWaveWords + k) * 64 + lane_id();
      if ((t * kWaveWords + k) * 64 >= n) break;  // (the same for every lane)
      const uint32_t inc = wave_incl_max(match_end(len, n, p));
      const uint32_t up = (uint32_t)__shfl_up((int)inc, 1, 64), top = (uint32_t)__shfl((int)inc, 63, 64);
      uint32_t reach = lane_id() ? up : 0;
      if (run > reach) reach = run;
      if (p < n && len[p] && reach <= p) pretok::dfa_walk(len, n, p, mark);
      if (top > run) run = top;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_pt_popc(const uint64_t* a, const uint64_t* b, uint64_t nw, uint64_t* ca,
                                                      uint64_t* cb) {
  for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < nw; j += (uint64_t)gridDim.x * kThreads) {
    ca[j] = (uint64_t)__popcll(a[j]);
    if (cb) cb[j] = (uint64_t)__popcll(b[j]);
  }
}

// (whit is zero before the kernel; every writer stores 1)
__global__ __launch_bounds__(kThreads) void k_pt_hit(Tables T0, Step st, Ctx x, uint8_t* whit) {
  const Tables T = with_nd(T0);
  for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < x.n; p += (uint64_t)gridDim.x * kThreads) {
    if (!pretok::in_word(x, p) || pretok::unit_lead(x, p) != p) continue;
    uint32_t l;
    if (pretok::split_in(T, st, x, p, pretok::cp_at(x, p, &l))) whit[pretok::word_of(st, x, p)] = 1;
  }
}

// ---- the rewriters -------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_excl(uint32_t v) {  // the sum of the lanes below
  uint32_t inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o, 64);
    if (lane_id() >= (uint32_t)o) inc += u;
  }
  return inc - v;
}

__global__ __launch_bounds__(kThreads) void k_pt_rw_count(Tables T0, Step st, Ctx x, uint64_t nw, uint64_t* len) {
  const Tables T = with_nd(T0);
  for (uint64_t j = wave_id(); j < nw; j += n_waves()) {
    const uint64_t p = j * 64 + lane_id();
    uint8_t unit[pretok::kMaxUnit];
    bool bg;
    const uint32_t l = wave_sum(p < x.n ? pretok::rw_unit(T, st, x, p, unit, &bg) : 0);
    if (lane_id() == 0) len[j] = l;
  }
}

__global__ __launch_bounds__(kThreads) void k_pt_rw_write(Tables T0, Step st, Ctx x, uint64_t nw, const uint64_t* pos,
                                                          uint8_t* out, uint8_t* out_beg) {
  const Tables T = with_nd(T0);
  for (uint64_t j = wave_id(); j < nw; j += n_waves()) {
    const uint64_t p = j * 64 + lane_id();
    uint8_t unit[pretok::kMaxUnit];
    bool bg = false;
    const uint32_t l = p < x.n ? pretok::rw_unit(T, st, x, p, unit, &bg) : 0;
    const uint64_t at = pos[j] + wave_excl(l);
    for (uint32_t k = 0; k < l; k++) {
      out[at + k] = unit[k];
      out_beg[at + k] = k == 0 && bg ? 1 : 0;
    }
  }
}

// out_off[d]: the output bytes of the input bytes before text d
__global__ __launch_bounds__(kThreads) void k_pt_rw_off(Tables T0, Step st, Ctx x, uint64_t nw, const uint64_t* pos,
                                                        const uint64_t* doc_off, uint64_t n_docs, uint64_t* out_off) {
  const Tables T = with_nd(T0);
  for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = doc_off[d];
    uint64_t at = o >= x.n ? pos[nw] : pos[o >> 6];
    if (o < x.n)
      for (uint64_t p = o & ~63ull; p < o; p++) {
        uint8_t unit[pretok::kMaxUnit];
        bool bg;
        at += pretok::rw_unit(T, st, x, p, unit, &bg);
      }
    out_off[d] = at;
  }
}

__global__ __launch_bounds__(kThreads) void k_pt_pack(const uint8_t* flags, uint64_t n, uint64_t nw, Bits out) {
  for (uint64_t j = wave_id(); j < nw; j += n_waves()) {
    const uint64_t p = j * 64 + lane_id();
    const uint64_t mi = __ballot(p < n), mb = __ballot(p < n && flags[p] != 0);
    if (lane_id() == 0) {
      out.inw[j] = mi;
      out.beg[j] = mb;
    }
  }
}

// ---- the final gather ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_pt_empty(const uint64_t* doc_off, uint64_t n_docs, uint64_t* e) {
  for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * kThreads)
    e[d] = doc_off[d] == doc_off[d + 1] ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_pt_gather(Ctx x, Gather g) {
  for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < x.n; p += (uint64_t)gridDim.x * kThreads) {
    if (!pretok::in_word(x, p)) continue;
    const uint64_t j = p >> 6, lo = below((uint32_t)(p & 63));
    const uint64_t before = g.ex ? g.ex[normalize::doc_of(g.doc_off, g.n_docs, p)] : 0;
    const uint64_t ob = g.posb[j] + (uint64_t)__popcll(x.inw[j] & lo) + before * g.eb;
    g.words[ob] = x.t[p];
    if (pretok::bit(x.beg, p)) g.word_off[g.posw[j] + (uint64_t)__popcll(x.beg[j] & lo) + before * g.ew] = ob;
  }
}

// text_word, the words of the empty texts and the closing word_off
__global__ __launch_bounds__(kThreads) void k_pt_gather_text(Ctx x, Gather g, uint64_t nw) {
  for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d <= g.n_docs; d += (uint64_t)gridDim.x * kThreads) {
    const uint64_t o = g.doc_off[d], lo = below((uint32_t)(o & 63));
    const uint64_t wb = o < x.n ? g.posw[o >> 6] + (uint64_t)__popcll(x.beg[o >> 6] & lo) : g.posw[nw];
    const uint64_t bb = o < x.n ? g.posb[o >> 6] + (uint64_t)__popcll(x.inw[o >> 6] & lo) : g.posb[nw];
    const uint64_t before = g.ex ? g.ex[d] : 0;
    g.text_word[d] = wb + before * g.ew;
    if (d == g.n_docs) {
      g.word_off[g.n_words] = g.n_bytes;
    } else if (g.ex && g.ex[d + 1] != g.ex[d]) {  // (empty in the input: it has no byte now either)
      for (uint64_t k = 0; k < g.ew; k++) g.word_off[wb + before * g.ew + k] = bb + before * g.eb + g.ew_off[k];
      for (uint64_t k = 0; k < g.eb; k++) g.words[bb + before * g.eb + k] = g.ew_bytes[k];
    }
  }
}

// ---- launchers -----------------------------------------------------------------------------------------

#define PT_LAUNCHED()                          \
  do {                                         \
    const hipError_t e_ = hipGetLastError();   \
    if (e_ != hipSuccess) return e_;           \
  } while (0)

hipError_t launch_init(uint64_t n, const uint64_t* doc_off, uint64_t n_docs, Bits out, hipStream_t s) {
  const uint64_t nw = words64(n);
  if (!nw) return hipSuccess;
  k_pt_init<<<grid_for(nw), kThreads, 0, s>>>(n, nw, out);
  PT_LAUNCHED();
  k_pt_doc_begin<<<grid_for(n_docs), kThreads, 0, s>>>(doc_off, n_docs, n, out.beg);
  return hipGetLastError();
}

hipError_t count_begins(const Ctx& x, uint64_t* wpos, uint64_t* tmp, uint64_t tmp_cap, uint64_t* n_words, hipStream_t s) {
  const uint64_t nw = words64(x.n);
  *n_words = 0;
  if (!nw) return hipMemsetAsync(wpos, 0, 8, s);
  k_pt_popc<<<grid_for(nw), kThreads, 0, s>>>(x.beg, nullptr, nw, wpos, nullptr);
  PT_LAUNCHED();
  hipError_t e = ctok_dev::scan_u64(wpos, nw, tmp, tmp_cap, s);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(n_words, wpos + nw, 8, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

hipError_t launch_split(const Tables& T, Step st, const Ctx& x, const Scratch& sc, Bits out, hipStream_t s) {
  const uint64_t nw = words64(x.n);
  if (!nw) return hipSuccess;
  if (st.kind == pretok::K_SCRIPTS) {
    const uint64_t nt = wave_tiles(x.n);
    k_pt_script_tail<<<grid_for(nt * 64), kThreads, 0, s>>>(x, nt, sc.tail);
    PT_LAUNCHED();
    k_pt_script_carry<<<1, kThreads, 0, s>>>(sc.tail, nt, sc.carry);
    PT_LAUNCHED();
    k_pt_script<<<grid_for(nt * 64), kThreads, 0, s>>>(T, st, x, nt, sc.carry, out);
    return hipGetLastError();
  }
  if (st.kind == pretok::K_SPLIT && st.mode == pretok::M_LITERAL) {
    hipError_t e = hipMemsetAsync(sc.mark, 0, x.n, s);
    if (e != hipSuccess) return e;
    k_pt_cand<<<grid_for(x.n), kThreads, 0, s>>>(st, x, sc.cand);
    PT_LAUNCHED();
    st.cand = sc.cand;
    k_pt_chain<<<grid_for(x.n), kThreads, 0, s>>>(st, x.n, sc.mark);
    PT_LAUNCHED();
    st.mark = sc.mark;
  }
  if (st.kind == pretok::K_SPLIT && st.mode == pretok::M_DFA) {
    const uint64_t nt = wave_tiles(x.n);
    hipError_t e = hipMemsetAsync(sc.mark, 0, x.n, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(sc.over, 0xFF, 4, s);
    if (e != hipSuccess) return e;
    // (the table in LDS: a workgroup strides over many bytes, so that the copy is shared)
    if ((uint64_t)st.dfa.n_states * st.dfa.n_symbols * 2 <= kDfaLdsBytes)
      k_pt_dfa_len<true><<<grid_for(x.n, 2048), kThreads, 0, s>>>(T, st, x, sc.len, sc.over);
    else
      k_pt_dfa_len<false><<<grid_for(x.n), kThreads, 0, s>>>(T, st, x, sc.len, sc.over);
    PT_LAUNCHED();
    k_pt_dfa_tail<<<grid_for(nt * 64), kThreads, 0, s>>>(sc.len, x.n, nt, sc.tmax);
    PT_LAUNCHED();
    k_pt_dfa_carry<<<1, kThreads, 0, s>>>(sc.tmax, nt, sc.tcarry);
    PT_LAUNCHED();
    k_pt_dfa_chain<<<grid_for(nt * 64), kThreads, 0, s>>>(sc.len, x.n, nt, sc.tcarry, sc.mark);
    PT_LAUNCHED();
    st.mark = sc.mark;
  }
  if (st.kind == pretok::K_SPLIT && st.mode != pretok::M_IDENTITY && (st.flags & 15u) == pretok::B_REMOVED) {
    // (wpos is count_begins' scan, whit zero and large enough: the host's part)
    st.wpos = sc.wpos;
    k_pt_hit<<<grid_for(x.n), kThreads, 0, s>>>(T, st, x, sc.whit);
    PT_LAUNCHED();
    st.whit = sc.whit;
  }
  k_pt_split<<<grid_for(nw * 64), kThreads, 0, s>>>(T, st, x, nw, out);
  return hipGetLastError();
}

hipError_t launch_rw_count(const Tables& T, const Step& st, const Ctx& x, uint64_t* len, hipStream_t s) {
  const uint64_t nw = words64(x.n);
  if (!nw) return hipSuccess;
  k_pt_rw_count<<<grid_for(nw * 64), kThreads, 0, s>>>(T, st, x, nw, len);
  return hipGetLastError();
}

hipError_t launch_rw_write(const Tables& T, const Step& st, const Ctx& x, const uint64_t* pos, const uint64_t* doc_off,
                           uint64_t n_docs, uint8_t* out, uint8_t* out_beg, uint64_t* out_off, hipStream_t s) {
  const uint64_t nw = words64(x.n);
  if (nw) {
    k_pt_rw_write<<<grid_for(nw * 64), kThreads, 0, s>>>(T, st, x, nw, pos, out, out_beg);
    PT_LAUNCHED();
  }
  k_pt_rw_off<<<grid_for(n_docs + 1), kThreads, 0, s>>>(T, st, x, nw, pos, doc_off, n_docs, out_off);
  return hipGetLastError();
}

hipError_t launch_pack(const uint8_t* flags, uint64_t n, Bits out, hipStream_t s) {
  const uint64_t nw = words64(n);
  if (!nw) return hipSuccess;
  k_pt_pack<<<grid_for(nw * 64), kThreads, 0, s>>>(flags, n, nw, out);
  return hipGetLastError();
}

hipError_t launch_gather_count(const Ctx& x, uint64_t* cb, uint64_t* cw, hipStream_t s) {
  const uint64_t nw = words64(x.n);
  if (!nw) return hipSuccess;
  k_pt_popc<<<grid_for(nw), kThreads, 0, s>>>(x.inw, x.beg, nw, cb, cw);
  return hipGetLastError();
}

hipError_t launch_empty(const uint64_t* doc_off, uint64_t n_docs, uint64_t* e, hipStream_t s) {
  if (!n_docs) return hipSuccess;
  k_pt_empty<<<grid_for(n_docs), kThreads, 0, s>>>(doc_off, n_docs, e);
  return hipGetLastError();
}

hipError_t launch_gather(const Ctx& x, const Gather& g, hipStream_t s) {
  if (x.n) {
    k_pt_gather<<<grid_for(x.n), kThreads, 0, s>>>(x, g);
    PT_LAUNCHED();
  }
  k_pt_gather_text<<<grid_for(g.n_docs + 1), kThreads, 0, s>>>(x, g, words64(x.n));
  return hipGetLastError();
}

}  // namespace ctok_pt
