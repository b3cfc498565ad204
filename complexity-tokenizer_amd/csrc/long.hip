// Encode path, stage 3: long pieces (> 64 B, and a tile's overflow) -- k_long_len, k_long_order,
// the wave tiers k_bpe_wave (dense <= 256 B, segmented to 4096 B), the linked-list k_bpe_long
// (added tokens; global memory past 4096 B).
#include "dev_common.h"
#include "pair_lookup_dev.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// BPE, long pieces: one wavefront per piece over a doubly linked token list in global memory.
// Each round finds the global minimum rank r (wave reduction).  If the merge table is
// rank-monotone ("proper": every merge consuming token z ranks after every merge producing
// z), the sequential algorithm applies all non-overlapping occurrences of r left to right
// before any other merge, so they are applied in one parallel round; (x,x) chains and
// non-monotone tables fall back to the exact sequential order.

// Working state of one long piece.  GMEM = arrays in global memory (any length): every access
// is an agent-scope relaxed atomic (`global_load/store ... sc1`, served by L2), so lanes of the
// wave see each other's stores between rounds (the vector L1 does not).  LDS = arrays in the
// wave's slice of LDS (pieces up to kLdsPos), accessed through address-space-3 pointers so the
// compiler emits in-order ds_read/ds_write (never flat).
template <bool GMEM>
struct LongState;

template <>
struct LongState<true> {
  uint32_t* tok;
  uint32_t* nxt;
  uint32_t* prv;
  uint32_t* rk;
  static __device__ __forceinline__ uint32_t ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t Tok(uint32_t i) const { return ld(tok + i); }
  __device__ __forceinline__ uint32_t Nxt(uint32_t i) const { return ld(nxt + i); }
  __device__ __forceinline__ uint32_t Prv(uint32_t i) const { return ld(prv + i); }
  __device__ __forceinline__ uint32_t Rk(uint32_t i) const { return ld(rk + i); }
  __device__ __forceinline__ void sTok(uint32_t i, uint32_t v) const { st(tok + i, v); }
  __device__ __forceinline__ void sNxt(uint32_t i, uint32_t v) const { st(nxt + i, v); }
  __device__ __forceinline__ void sPrv(uint32_t i, uint32_t v) const { st(prv + i, v); }
  __device__ __forceinline__ void sRk(uint32_t i, uint32_t v) const { st(rk + i, v); }
  static __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  }
};

template <>
struct LongState<false> {
  lds_u32* tok;
  lds_u32* nxt;
  lds_u32* prv;
  lds_u32* rk;
  __device__ __forceinline__ uint32_t Tok(uint32_t i) const { return tok[i]; }
  __device__ __forceinline__ uint32_t Nxt(uint32_t i) const { return nxt[i]; }
  __device__ __forceinline__ uint32_t Prv(uint32_t i) const { return prv[i]; }
  __device__ __forceinline__ uint32_t Rk(uint32_t i) const { return rk[i]; }
  __device__ __forceinline__ void sTok(uint32_t i, uint32_t v) const { tok[i] = v; }
  __device__ __forceinline__ void sNxt(uint32_t i, uint32_t v) const { nxt[i] = v; }
  __device__ __forceinline__ void sPrv(uint32_t i, uint32_t v) const { prv[i] = v; }
  __device__ __forceinline__ void sRk(uint32_t i, uint32_t v) const { rk[i] = v; }
  static __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
};

template <bool G>
__device__ __forceinline__ void merge_one(const Tables& t, const LongState<G>& L, uint32_t i, uint32_t nid,
                                          uint32_t* err) {
  const uint32_t j = L.Nxt(i);
  const uint32_t nj = L.Nxt(j);
  L.sTok(i, nid);
  L.sTok(j, kDead);
  L.sRk(j, kNoRank);
  L.sNxt(i, nj);
  if (nj != kNone) L.sPrv(nj, i);
  L.sRk(i, nj != kNone ? rank_of(t, nid, L.Tok(nj), err) : kNoRank);
  const uint32_t p = L.Prv(i);
  if (p != kNone) L.sRk(p, rank_of(t, L.Tok(p), nid, err));
}


template <bool G>
__device__ uint32_t bpe_wave(const Tables& t, const uint8_t* bytes, uint32_t n, const LongState<G>& L, uint32_t* out,
                             uint32_t* err, uint32_t* sink) {
  const uint32_t lane = threadIdx.x & 63;
  // initial ids, dropping bytes whose char is not in the vocab (order-preserving compaction)
  uint32_t m = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const uint32_t i = i0 + lane;
    const int32_t id = i < n ? t.byte2id[bytes[i]] : -1;
    const uint64_t bal = __ballot(id >= 0);
    if (id >= 0) L.sTok(m + __popcll(bal & lanemask_lt()), (uint32_t)id);
    m = uni(m + __popcll(bal));
  }
  L.sync();
  if (m == 0) return 0;
  for (uint32_t i = lane; i < m; i += 64) {
    L.sNxt(i, i + 1 < m ? i + 1 : kNone);
    L.sPrv(i, i > 0 ? i - 1 : kNone);
    L.sRk(i, i + 1 < m ? rank_of(t, L.Tok(i), L.Tok(i + 1), err) : kNoRank);
  }
  L.sync();
  for (;;) {
    uint32_t lmin = kNoRank;
    for (uint32_t i = lane; i < m; i += 64) lmin = min(lmin, L.Rk(i));
    const uint32_t r = uni(wave_min_u32(lmin));
    if (r == kNoRank) break;
    const uint32_t nid = uni(new_id_of(t, r));
    uint32_t lpos = kNone;
    for (uint32_t i = lane; i < m; i += 64) {
      if (L.Rk(i) == r) { lpos = i; break; }
    }
    const uint32_t lm = uni(wave_min_u32(lpos));
    const uint32_t chain = uni(L.Tok(lm) == L.Tok(L.Nxt(lm)) ? 1u : 0u);
    // sites past `cut` wait for a later round (eager merges, see first_cascade)
    uint32_t cut = kNone;
    if (serial_round(t, r) && !chain) {
      uint32_t c = kNone;
      for (uint32_t i = lane; i < m; i += 64) {
        if (L.Rk(i) != r) continue;
        const uint32_t pp = L.Prv(i), j = L.Nxt(i), nj = L.Nxt(j);
        const bool left_site = pp != kNone && L.Prv(pp) != kNone && L.Rk(L.Prv(pp)) == r;
        const uint32_t rl = pp == kNone ? kNoRank : rank_of(t, left_site ? nid : L.Tok(pp), nid, sink);
        const uint32_t rr = nj == kNone ? kNoRank : rank_of(t, nid, L.Tok(nj), sink);
        if (rl < r || rr < r) c = min(c, i);
      }
      cut = uni(wave_min_u32(c));
    }
    if (serial_round(t, r) && chain) {
      merge_one(t, L, lm, nid, err);  // every lane performs the same update
    } else if (chain) {
      // (x,x) runs: the sequential left-to-right order, walked by the whole wave in lockstep
      for (uint32_t i = lm; i != kNone; i = uni(L.Nxt(i))) {
        if (uni(L.Rk(i)) == r) merge_one(t, L, i, nid, err);
      }
    } else {
      // phase A: splice out the right token of every occurrence (up to cut)
      for (uint32_t i = lane; i < m; i += 64) {
        if (L.Rk(i) != r || (cut != kNone && i > cut)) continue;
        const uint32_t j = L.Nxt(i);
        const uint32_t nj = L.Nxt(j);
        L.sTok(i, nid);
        L.sTok(j, kDead);
        L.sRk(j, kNoRank);
        L.sRk(i, kSel);
        L.sNxt(i, nj);
        if (nj != kNone) L.sPrv(nj, i);
      }
      L.sync();
      // phase B: ranks of the new pairs (left pair only when its left end is not a site)
      for (uint32_t i = lane; i < m; i += 64) {
        if (L.Rk(i) != kSel) continue;
        const uint32_t nj = L.Nxt(i);
        L.sRk(i, nj != kNone ? rank_of(t, nid, L.Tok(nj), err) : kNoRank);
        const uint32_t p = L.Prv(i);
        if (p != kNone && L.Rk(p) != kSel) L.sRk(p, rank_of(t, L.Tok(p), nid, err));
      }
    }
    L.sync();
    // (no per-round read of the panic flag: a panicking pair ranks as kNoRank, so the loop still
    // ends, and the host discards the batch -- a global load per round would double its latency)
  }
  // emit surviving tokens in order
  uint32_t c = 0;
  for (uint32_t i0 = 0; i0 < m; i0 += 64) {
    const uint32_t i = i0 + lane;
    const uint32_t v = i < m ? L.Tok(i) : kDead;
    const uint64_t bal = __ballot(v != kDead);
    if (v != kDead) out[c + __popcll(bal & lanemask_lt())] = v;
    c = uni(c + __popcll(bal));
  }
  return c;
}

constexpr uint32_t kLdsPos = 2048;  // positions per wave in LDS (4 u32 arrays: 32 KiB per wave)
constexpr uint32_t kWaveMax = 64 * 64;  // longest piece of the dense wave tiers (k_bpe_wave)

template <bool G>
__device__ uint32_t long_piece(const Tables& t, const uint8_t* bytes, uint32_t n, const LongState<G>& L,
                               uint32_t* out, uint32_t* err) {
  const uint32_t lane = threadIdx.x & 63;
  if (t.n_at == 0) return bpe_wave<G>(t, bytes, n, L, out, err, err - 2 + kCtrSink);
  uint32_t cnt = 0, pos = 0;
  while (pos < n) {  // every lane computes the same added-token split; kept in SGPRs
    int32_t best = -1;
    uint32_t blen = 0;
    for (uint32_t k = 0; k < t.n_at; k++) {
      const uint32_t m = t.at_off[k + 1] - t.at_off[k];
      if (AddedMatch::find(t, k, bytes + pos, n - pos) == 0 && (best < 0 || m > blen)) { best = (int32_t)k; blen = m; }
    }
    best = (int32_t)uni((uint32_t)best);
    blen = uni(blen);
    if (best >= 0) {
      if (lane == 0) out[cnt] = t.at_id[best];
      cnt++;
      pos += blen;
      continue;
    }
    uint32_t nxt = n - pos;
    for (uint32_t k = 0; k < t.n_at; k++) {
      const int64_t f = AddedMatch::find(t, k, bytes + pos, n - pos);
      if (f > 0 && (uint32_t)f < nxt) nxt = (uint32_t)f;
    }
    nxt = uni(nxt);
    cnt = uni(cnt + bpe_wave<G>(t, bytes + pos, nxt, L, out + cnt, err, err - 2 + kCtrSink));
    pos += nxt;
  }
  return cnt;
}

// End of the piece starting at s: the next set bit of the piece-start bitmap, else n_bytes.
// Wave-uniform (64 bitmap words per step).
__device__ __forceinline__ uint32_t piece_end(const Work& w, uint32_t s) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t first = (s + 1) >> 5, sh = (s + 1) & 31;
  for (uint32_t base = first; base < w.n_words; base += 64) {
    const uint32_t idx = base + lane;
    uint32_t v = idx < w.n_words ? w.pbits[idx] : 0u;
    if (idx == first) v &= ~0u << sh;
    const uint64_t m = __ballot(v != 0);
    if (m) {
      const uint32_t l = uni(__ffsll((unsigned long long)m) - 1);
      const uint32_t vv = uni((uint32_t)__shfl((int)v, (int)l, 64));
      return min(w.n_bytes, ((base + l) << 5) + (uint32_t)__builtin_ctz(vv));
    }
  }
  return w.n_bytes;
}

// One wavefront per long piece, pieces dealt to waves by a static stride (no work-queue
// atomics: every loop bound and index is a scalar, so the wave never splits).  GMEM selects the
// tier: LDS for pieces up to kLdsPos positions, global memory beyond.
template <bool GMEM>
__global__ __launch_bounds__(256) void k_bpe_long(Work w, Tables t) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_long[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wid = uni(threadIdx.x >> 6);
  const uint32_t n_long = uni(long_count(w));
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  uint32_t* err = &w.counters[kCtrErr];
  for (uint32_t li = uni(blockIdx.x * (blockDim.x >> 6) + wid); li < n_long; li += n_waves) {
    const uint64_t e = w.long_list[li];
    const uint32_t s = uni((uint32_t)e);
    const uint32_t o = uni(long_ord(e));
    const uint32_t n = uni(piece_end(w, s) - s);
    // tiers: LDS up to kLdsPos positions, global memory beyond (only beyond the dense wave tiers
    // when those run, i.e. without added tokens)
    const uint32_t gmin = (t.n_at != 0 || t.dbg == 7) ? kLdsPos : kWaveMax;
    if (GMEM != (n > gmin)) continue;
    const uint8_t* bytes = w.text + s;
    uint32_t* out = w.lids + w.long_pos[li];
    uint32_t cnt;
    if constexpr (GMEM) {
      uint32_t* lw = w.lw + 4 * (size_t)w.lw_pos[li];
      LongState<true> L{lw, lw + n, lw + 2 * (size_t)n, lw + 3 * (size_t)n};
      cnt = long_piece<true>(t, bytes, n, L, out, err);
    } else {
      lds_u32* lds = (lds_u32*)s_long + wid * 4 * kLdsPos;
      LongState<false> L{lds, lds + kLdsPos, lds + 2 * kLdsPos, lds + 3 * kLdsPos};
      cnt = long_piece<false>(t, bytes, n, L, out, err);
    }
    if (lane == 0) {
      const uint32_t tile = s / kTile;
      w.long_cnt[li] = cnt;
      w.mrec[(size_t)tile * kTileSlots + o] = kRecLong | li;
      atomicAdd(&w.tile_tok[tile], cnt);
    }
  }
}

// ------------------------------------------------------------------------------------------
// BPE, pieces of kMedMax+1 .. 64K bytes without added tokens: one wavefront per piece, the
// piece's tokens and pair ranks dense in the wave's LDS slice (position p in lane p % 64 of
// step p / 64).  A round: r = wave minimum of the pair ranks; the merge sites are every
// position whose pair has rank r (proper tables: occurrences never overlap unless the pair is
// (x, x), where runs take every other site from the left, as the sequential loop does;
// non-monotone tables: the leftmost site only); the sites' right tokens are dropped while the
// survivors are compacted into the other buffer (ballot prefix counts), and only pairs that
// touch a new token are looked up again (Bloom filter in LDS, global table on a Bloom hit).
// The live token count shrinks every round, and so does the work per round.

template <int K>
struct WaveSlice {  // per-wave LDS slice: 64K positions (compacted in place every round)
  static constexpr uint32_t C = 64 * K;
  static constexpr uint32_t kBytes = 8 * C + 2 * (C + 64) + 2 * C;
  lds_u32* base;  // tok | rk | chg | sel | pos (u16: the token's first initial position, window rounds)
  __device__ __forceinline__ lds_u32* tok() const { return base; }
  __device__ __forceinline__ lds_u32* rk() const { return base + C; }
  __device__ __forceinline__ __attribute__((address_space(3))) uint8_t* chg() const {
    return (__attribute__((address_space(3))) uint8_t*)(base + 2 * C);
  }
  __device__ __forceinline__ __attribute__((address_space(3))) uint8_t* sel() const {
    return (__attribute__((address_space(3))) uint8_t*)(base + 2 * C) + C + 64;
  }
  __device__ __forceinline__ __attribute__((address_space(3))) uint16_t* pos() const {
    return (__attribute__((address_space(3))) uint16_t*)(sel() + C + 64);
  }
};

template <int K, bool HOT>
__device__ uint32_t bpe_wave_dense(const Tables& t, const PairLds& P, const int32_t* s_b2id, const uint8_t* bytes,
                                   uint32_t n, const WaveSlice<K>& S, uint32_t* out, uint32_t* err, uint32_t* sink,
                                 uint32_t* rounds = nullptr /* += this piece's rounds (per-wave register) */) {
  const uint32_t lane = threadIdx.x & 63;
  lds_u32* tok = S.tok();
  lds_u32* rk = S.rk();
  auto chg = S.chg();
  auto sel = S.sel();
  auto pos = S.pos();
  // initial ids (bytes whose char is not in the vocab are dropped: order-preserving compaction);
  // the raw bytes go to chg for the initial pair ranks
  uint32_t m = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const uint32_t i = i0 + lane;
    const int32_t id = i < n ? s_b2id[bytes[i]] : -1;
    const uint64_t bal = __ballot(id >= 0);
    if (id >= 0) {
      const uint32_t q = m + __popcll(bal & lanemask_lt());
      tok[q] = (uint32_t)id;
      chg[q] = bytes[i];
    }
    m = uni(m + __popcll(bal));
  }
  wave_sync_lds();
  if (m == 0) return 0;
  // initial pairs are byte pairs: the 256 x 256 byte-pair table (byte pairs are left out of the
  // LDS image; every later pair holds a merged token)
#pragma unroll 4
  for (uint32_t p = lane; p < m; p += 64) {
    uint32_t r = kNoRank;
    if (p + 1 < m) {
      r = t.pair0[((uint32_t)chg[p] << 8) | chg[p + 1]];
      if (r != kNoRank && value_panics(t, r)) {
        atomicOr(err, kErrPanic);
        r = kNoRank;
      }
    }
    rk[p] = r;
    pos[p] = (uint16_t)p;
  }
  const uint32_t m0 = m;  // initial positions (window rounds: token spans are in these units)
  wave_sync_lds();
  uint32_t nr = 0;  // rounds (statistics: ctok_stats.long_rounds)
  for (;;) {
    nr++;
    uint32_t lmin = kNoRank;
#pragma unroll 8
    for (uint32_t p = lane; p < m; p += 64) lmin = min(lmin, (uint32_t)rk[p]);
    const uint32_t r = uni(wave_min_full_u32(lmin));
    if (r == kNoRank) break;
    const uint32_t nid = uni(new_id_of(t, r));
    // sites: positions whose pair has rank r; lm = the leftmost
    uint32_t lpos = kNone;
#pragma unroll 4
    for (uint32_t p = lane; p < m; p += 64) {
      const bool site = rk[p] == r;
      sel[p] = site ? 1 : 0;
      lpos = min(lpos, site ? p : kNone);
    }
    const uint32_t lm = uni(wave_min_full_u32(lpos));
    const bool chain = uni(tok[lm] == tok[lm + 1] ? 1u : 0u) != 0;
    wave_sync_lds();
    if (serial_round(t, r) && chain) {
      for (uint32_t p = lane; p < m; p += 64) sel[p] = p == lm ? 1 : 0;
      wave_sync_lds();
    } else if (serial_round(t, r)) {
      // eager merge (first_cascade): the sites up to the first whose sequential new pairs
      // include a lower rank
      uint32_t c = kNone;
      for (uint32_t p = lane; p < m; p += 64) {
        if (!sel[p]) continue;
        const bool left_site = p >= 2 && sel[p - 2];
        const uint32_t rl = p == 0 ? kNoRank : rank_pair<HOT>(t, P, left_site ? nid : (uint32_t)tok[p - 1], nid, sink);
        const uint32_t rr = p + 2 >= m ? kNoRank : rank_pair<HOT>(t, P, nid, tok[p + 2], sink);
        if (rl < r || rr < r) c = min(c, p);
      }
      const uint32_t cm = uni(wave_min_full_u32(c));
      if (cm != kNone) {
        for (uint32_t p = lane; p < m; p += 64)
          if (p > cm) sel[p] = 0;
        wave_sync_lds();
      }
    } else if (chain) {
      // (x, x): in a run of consecutive sites the sequential loop merges the 1st, 3rd, ... one
      // (the choice goes through chg, rewritten by the compaction below)
      for (uint32_t p = lane; p < m; p += 64) {
        uint32_t d = 0;
        if (sel[p]) {
          while (d < p && sel[p - 1 - d]) d++;
        }
        chg[p] = (sel[p] && (d & 1) == 0) ? 1 : 0;
      }
      wave_sync_lds();
      for (uint32_t p = lane; p < m; p += 64) sel[p] = chg[p];
      wave_sync_lds();
    }
    // window rounds (t.window, see bpe_wave_seg): a pair p of rank rc > r merges too when every
    // other pair starting in its window [pos(x) - left(x), end(y) + right(y)) ranks above rc
    // (pos: each token's first initial position, carried through the compaction; end(y) = the
    // next token's pos).  Only local minima are checked (both neighbour pairs lie in every
    // window); the scans walk out from p and stop at the window's ends or the first lower pair.
    if (t.window) {
      for (uint32_t p = lane; p + 1 < m; p += 64) {
        const uint32_t rc = rk[p];
        if (rc == kNoRank || rc == r || (p > 0 && (uint32_t)rk[p - 1] <= rc) || (uint32_t)rk[p + 1] <= rc) continue;
        const uint32_t wl = t.wmeta[tok[p]] & 0xFFFFu, wr = t.wmeta[tok[p + 1]] >> 16;
        const uint32_t p0 = pos[p];
        uint32_t lo = p0 > wl ? p0 - wl : 0u;
        uint32_t hi = (p + 2 < m ? (uint32_t)pos[p + 2] : m0) + wr;
        if (serial_round(t, rc)) {
          // eager candidate (not rank-monotone; see bpe_wave_seg): its new pairs with today's
          // neighbours rank above it, and the window covers the neighbours' own windows
          const uint32_t nn = new_id_of(t, rc);
          const uint32_t rl = p > 0 ? rank_pair<HOT>(t, P, tok[p - 1], nn, sink) : kNoRank;
          const uint32_t rr = p + 2 < m ? rank_pair<HOT>(t, P, nn, tok[p + 2], sink) : kNoRank;
          if (rl <= rc || rr <= rc) continue;
          if (p > 0) {
            const uint32_t wlu = t.wmeta[tok[p - 1]] & 0xFFFFu, pu = pos[p - 1];
            lo = min(lo, pu > wlu ? pu - wlu : 0u);
          }
          if (p + 2 < m) hi = max(hi, (p + 3 < m ? (uint32_t)pos[p + 3] : m0) + (t.wmeta[tok[p + 2]] >> 16));
        }
        bool fire = true;
        for (uint32_t j = p; fire && j > 0;) {
          --j;
          if ((uint32_t)pos[j] < lo) break;
          fire = (uint32_t)rk[j] > rc;
        }
        for (uint32_t j = p + 1; fire && j + 1 < m; j++) {
          if ((uint32_t)pos[j] >= hi) break;
          fire = (uint32_t)rk[j] > rc;
        }
        if (fire) sel[p] = 1;
      }
      wave_sync_lds();
    }
    // in-place compaction: a site's right neighbour is dropped, the site takes its new id (nid,
    // or in window rounds its own rank's).  Position p moves to q <= p; a step reads its 64
    // positions before it writes, and later steps read only positions past every q written so far.
    uint32_t base = 0;
    for (uint32_t p0 = 0; p0 < m; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool in = p < m;
      const bool site = in && sel[p];
      const bool dead = in && p > 0 && sel[p - 1];
      const bool alive = in && !dead;
      const uint32_t tv = in ? (uint32_t)tok[p] : 0u, rv = in ? (uint32_t)rk[p] : 0u;
      const uint32_t pv = in ? (uint32_t)pos[p] : 0u;
      const uint64_t bal = __ballot(alive);
      if (alive) {
        const uint32_t q = base + __popcll(bal & lanemask_lt());
        tok[q] = site ? (t.window ? new_id_of(t, rv) : nid) : tv;
        rk[q] = rv;
        pos[q] = (uint16_t)pv;
        chg[q] = site ? 1 : 0;
      }
      base = uni(base + __popcll(bal));
    }
    m = base;
    if (lane == 0) chg[m] = 0;
    wave_sync_lds();
    // pairs touching a new token get their rank again
    for (uint32_t p = lane; p < m; p += 64) {
      if (chg[p] | chg[p + 1]) rk[p] = p + 1 < m ? rank_pair<HOT>(t, P, tok[p], tok[p + 1], err) : kNoRank;
    }
    wave_sync_lds();
    // (no per-round read of the panic flag: a panicking pair ranks as kNoRank, so the loop still
    // ends, and the host discards the batch -- a global load per round would double its latency)
  }
#pragma unroll 4
  for (uint32_t p = lane; p < m; p += 64) out[p] = tok[p];
  if (rounds) *rounds += nr;
  return m;
}

// Long pieces (hundreds to thousands of tokens): positions stay put and are linked into a list
// (nxt / prv, u16); lane l owns the contiguous segment [l*S, (l+1)*S), in four groups of S/4
// positions whose ranks it keeps in registers with each group's minimum.  A round costs a
// 64-lane minimum, then only the lanes that hold a site look at the group(s) holding it, and
// only groups whose ranks changed are reloaded -- instead of every round sweeping and compacting
// the whole piece.
template <int K>
struct SegSlice {  // per-wave LDS slice for up to 64K positions
  static constexpr uint32_t C = 64 * K;
  static constexpr uint32_t kBytes = 12 * C + 256 + 1024;
  lds_u32* base;  // tok[C] | rk[C] | nxt[C] u16 | prv[C] u16 (the raw bytes until the list is built) |
                  // dirty[256] u8 (per group) | gmin[256] u32 (per group: its minimum rank, window rounds)
  __device__ __forceinline__ lds_u32* tok() const { return base; }
  __device__ __forceinline__ lds_u32* rk() const { return base + C; }
  __device__ __forceinline__ __attribute__((address_space(3))) uint16_t* nxt() const {
    return (__attribute__((address_space(3))) uint16_t*)(base + 2 * C);
  }
  __device__ __forceinline__ __attribute__((address_space(3))) uint16_t* prv() const { return nxt() + C; }
  __device__ __forceinline__ __attribute__((address_space(3))) uint8_t* dirty() const {
    return (__attribute__((address_space(3))) uint8_t*)(prv() + C);
  }
  __device__ __forceinline__ lds_u32* gmin() const { return (lds_u32*)(dirty() + 256); }
};

constexpr uint32_t kNoPos = 0xFFFFu;

template <int K, bool HOT>
__device__ uint32_t bpe_wave_seg(const Tables& t, const PairLds& P, const int32_t* s_b2id, const uint8_t* bytes,
                                 uint32_t n, const SegSlice<K>& S, uint32_t* out, uint32_t* err, uint32_t* sink,
                                 uint32_t* rounds = nullptr /* += this piece's rounds (per-wave register) */) {
  static_assert(K % 16 == 0 && K <= 64, "segment width: a multiple of 16, at most 64");
  constexpr uint32_t R = K / 4;  // registers per group
  const uint32_t lane = threadIdx.x & 63;
  lds_u32* tok = S.tok();
  lds_u32* rk = S.rk();
  auto nxt = S.nxt();
  auto prv = S.prv();
  auto raw = S.prv();  // (the raw bytes, for the byte-pair ranks, until prv is built)
  auto dirty = S.dirty();
  // initial ids (dropped bytes compacted away); raw bytes parked in prv for the byte-pair ranks.
  // The byte loads of 16 rows of 64 (coalesced) are issued together, then the rows are
  // compacted: one global latency per 1 KiB instead of one per 64 bytes.
  uint32_t m = 0;
  for (uint32_t j0 = 0; j0 * 64 < n; j0 += 16) {
    uint32_t bb[16];
    int32_t id[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t i = (j0 + j) * 64 + lane;
      bb[j] = i < n ? (uint32_t)bytes[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) id[j] = ((j0 + j) * 64 + lane < n) ? s_b2id[bb[j]] : -1;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t bal = __ballot(id[j] >= 0);
      if (id[j] >= 0) {
        const uint32_t q = m + __popcll(bal & lanemask_lt());
        tok[q] = (uint32_t)id[j];
        raw[q] = (uint16_t)bb[j];
      }
      m = uni(m + __popcll(bal));
    }
  }
  wave_sync_lds();
  if (m == 0) return 0;
  // lane l owns positions [l*SW, l*SW + SW) in four groups of G = SW/4 positions: SW is a
  // multiple of 16, so a group's ranks are read with G/4 independent 16-byte LDS loads into
  // v[g*R ..] (one LDS latency per group instead of one per position); positions >= m hold
  // kNoRank.  Group of position p (its dirty flag): p / G, by a multiply-high (p < 2^16).
  const uint32_t SW = min((uint32_t)K, (((m + 63) / 64) + 15) & ~15u);
  const uint32_t G = SW >> 2;
  const uint32_t gmag = (uint32_t)(((1ull << 32) + G - 1) / G);
  auto unit = [&](uint32_t p) { return __umulhi(p, gmag); };
  const uint32_t a0 = lane * SW;
  auto pos = [&](uint32_t b) { return a0 + (b / R) * G + (b % R); };  // site bit -> position
  // initial pair ranks, 16 positions at a time (their byte-pair table loads in flight together)
  for (uint32_t k0 = 0; k0 < SW; k0 += 16) {
    uint32_t sb[17], r[16];
#pragma unroll
    for (int k = 0; k < 17; k++) sb[k] = a0 + k0 + k < m ? (uint32_t)raw[a0 + k0 + k] : 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) r[k] = a0 + k0 + k + 1 < m ? t.pair0[(sb[k] << 8) | sb[k + 1]] : kNoRank;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint32_t p = a0 + k0 + k;
      if (r[k] != kNoRank && value_panics(t, r[k])) {
        atomicOr(err, kErrPanic);
        r[k] = kNoRank;
      }
      rk[p] = r[k];
      if (p < m) nxt[p] = p + 1 < m ? (uint16_t)(p + 1) : (uint16_t)kNoPos;
    }
  }
  wave_sync_lds();  // (every raw byte read before prv overwrites them)
  for (uint32_t k = 0; k < SW; k++) {
    const uint32_t p = a0 + k;
    if (p < m) prv[p] = p > 0 ? (uint16_t)(p - 1) : (uint16_t)kNoPos;
  }
  wave_sync_lds();
  lds_u32* dirty32 = (lds_u32*)dirty;
  dirty32[lane] = 0x01010101u;  // first round: every lane loads its groups
  uint32_t v[K];
  uint32_t gm[4] = {kNoRank, kNoRank, kNoRank, kNoRank};
  wave_sync_lds();
  uint32_t nr = 0;  // rounds (statistics: ctok_stats.long_rounds)
  for (;;) {
    nr++;
    const uint32_t dw = dirty32[lane];
    if (dw) {  // (re)load the changed groups' ranks and their minima
#pragma unroll
      for (int g = 0; g < 4; g++) {
        if (dw & (0xFFu << (8 * g))) {
          const uint4* src = (const uint4*)(rk + a0 + g * G);
          uint32_t mn = kNoRank;
#pragma unroll
          for (int q = 0; q < (int)R / 4; q++) {
            const uint4 x = (uint32_t)(4 * q) < G ? src[q] : make_uint4(kNoRank, kNoRank, kNoRank, kNoRank);
            v[g * R + 4 * q] = x.x;
            v[g * R + 4 * q + 1] = x.y;
            v[g * R + 4 * q + 2] = x.z;
            v[g * R + 4 * q + 3] = x.w;
            mn = min(min(mn, min(x.x, x.y)), min(x.z, x.w));
          }
          gm[g] = mn;
        }
      }
      dirty32[lane] = 0;
    }
    const uint32_t smin = min(min(gm[0], gm[1]), min(gm[2], gm[3]));
    const uint32_t r = uni(wave_min_full_u32(smin));
    if (r == kNoRank) break;
    const uint32_t nid = uni(new_id_of(t, r));
    // this segment's sites as a bit mask (bit g*R + k: position a0 + g*G + k), from the groups
    // whose minimum is r; the leftmost site decides the mode
    uint64_t sites = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      if (gm[g] == r) {
#pragma unroll
        for (int k = 0; k < (int)R; k++) sites |= (uint64_t)(v[g * R + k] == r) << (g * R + k);
      }
    }
    const uint32_t first = sites ? pos((uint32_t)__builtin_ctzll(sites)) : kNone;
    // every site holds the same pair (rank r's), so a lane tells (x, x) from its own first site
    // (no second wave reduction on the round's critical path)
    bool chain = false;
    if (sites) chain = tok[first] == tok[nxt[first]];
    const bool eager = serial_round(t, r);
    const bool chain_any = __ballot(chain) != 0;
    if (eager && chain_any) {
      const uint32_t lm = uni(wave_min_full_u32(first));
      sites = first == lm ? (sites & (~sites + 1)) : 0ull;  // the leftmost site only
    } else if (eager) {
      // eager merge (first_cascade): the sites up to the first whose sequential new pairs
      // include a lower rank; the left pair of a site whose left neighbour's left neighbour is
      // a site is (nid, nid), its right pair (nid, the next token as it is now)
      uint32_t c = kNone;
      for (uint64_t rest = sites; rest;) {
        const uint32_t p = pos((uint32_t)__builtin_ctzll(rest));
        rest &= rest - 1;
        const uint32_t pp = prv[p], q = nxt[p];
        const uint32_t nq = nxt[q];
        const uint32_t ppp = pp != kNoPos ? (uint32_t)prv[pp] : kNoPos;
        const bool left_site = ppp != kNoPos && rk[ppp] == r;
        Probe<false, HOT> pl, pr;
        pl.start(t, P, left_site ? nid : (pp != kNoPos ? (uint32_t)tok[pp] : 0u), nid, pp != kNoPos);
        pr.start(t, P, nid, nq != kNoPos ? (uint32_t)tok[nq] : 0u, nq != kNoPos);
        const uint32_t rl = pp != kNoPos ? pl.finish(t, sink) : kNoRank;
        const uint32_t rr = nq != kNoPos ? pr.finish(t, sink) : kNoRank;
        if (rl < r || rr < r) c = min(c, p);
      }
      const uint32_t cm = uni(wave_min_full_u32(c));
      if (cm != kNone) {
        uint64_t keep = 0;
        for (uint64_t rest = sites; rest;) {
          const uint32_t k = (uint32_t)__builtin_ctzll(rest);
          rest &= rest - 1;
          if (pos(k) <= cm) keep |= 1ull << k;
        }
        sites = keep;
      }
    } else if (chain && sites) {
      // (x, x) runs: the 1st, 3rd, ... site of a run (d = sites before p in its run)
      uint64_t keep = 0, rest = sites;
      uint32_t d = 0, last = kNone;
      while (rest) {
        const uint32_t k = (uint32_t)__builtin_ctzll(rest);
        rest &= rest - 1;
        const uint32_t p = pos(k);
        if (last != kNone && prv[p] == last) {
          d++;
        } else {  // run start, or a run entering from the previous segment: walk back
          d = 0;
          for (uint32_t q = prv[p]; q != kNoPos && rk[q] == r; q = prv[q]) d++;
        }
        last = p;
        if ((d & 1) == 0) keep |= 1ull << k;
      }
      sites = keep;
    }
    // Window rounds (t.window: token instances span exactly their strings' lengths; the argument
    // below is for a rank-monotone table -- every pair a merge makes ranks after it -- and holds for
    // any candidate whose merge is not eager; eager ones get the extra check further down).  Besides the sites of the
    // round's rank r, a pair c = (x, y) of rank rc > r merges now when no other pair starting in
    // its window [c - left(x), end(y) + right(y)) ranks <= rc, left(x) / right(y) being the
    // longest left / right side of any merge with x on the right / y on the left (Tables::wmeta).
    // Exact: the sequential loop (src/bpe.rs:88-153) takes merges in non-decreasing rank order,
    // so before c it can only touch x or y by merging some u into (u, x) or (y, v) at a rank <
    // rc; u (v) spans at most left(x) (right(y)) positions next to c, and the first merge
    // building it was a pair of today's tokens inside that span ranked below rc -- which the
    // window excludes.  So c is the first merge that touches x or y, and applying it now leaves
    // the rest of the sequence unchanged (every pair it makes ranks above rc).  Checked at group
    // granularity: c must be its group's only minimum, and every other group the window
    // overlaps must have a larger minimum (gmin, published here each round); a window over more
    // than kWinGroups groups is not checked.  Random-letter 4 KiB runs (C3): ~820 rounds -> ~30.
    uint64_t bsites = 0;
    if (t.window) {
      constexpr uint32_t kWinGroups = 16;
      lds_u32* gmin = S.gmin();
#pragma unroll
      for (int g = 0; g < 4; g++) gmin[4 * lane + g] = gm[g];
      uint32_t cp[4], cb[4];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        cp[g] = kNone;
        cb[g] = 0;
        if (gm[g] != kNoRank && gm[g] != r) {
          uint32_t eq = 0;
#pragma unroll
          for (int k = 0; k < (int)R; k++) eq |= (uint32_t)(v[g * R + k] == gm[g]) << k;
          if (__popc(eq) == 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(eq);
            cb[g] = g * R + k;
            cp[g] = a0 + g * G + k;
          }
        }
      }
      wave_sync_lds();
      uint32_t q[4], tc[4], tq[4], nq[4];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        q[g] = cp[g] != kNone ? (uint32_t)nxt[cp[g]] : kNoPos;
        tc[g] = cp[g] != kNone ? (uint32_t)tok[cp[g]] : 0u;
      }
#pragma unroll
      for (int g = 0; g < 4; g++) {
        tq[g] = q[g] != kNoPos ? (uint32_t)tok[q[g]] : 0u;
        nq[g] = q[g] != kNoPos ? (uint32_t)nxt[q[g]] : kNoPos;
      }
      uint32_t wl[4], wr[4];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        wl[g] = q[g] != kNoPos ? (t.wmeta[tc[g]] & 0xFFFFu) : 0u;
        wr[g] = q[g] != kNoPos ? (t.wmeta[tq[g]] >> 16) : 0u;
      }
      uint32_t lo_x[4], end_x[4];  // window bounds widened for eager candidates (below)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        lo_x[g] = kNone;
        end_x[g] = 0;
      }
      if (!t.proper) {
        // Not rank-monotone (tiktoken-style lists): a candidate whose merge is eager -- some merge
        // consuming its token n ranks below it -- also needs its new pairs with today's
        // neighbours, (u, n) and (n, v), to rank above it, and its window widened to u's and v's
        // own windows ([u - left(u), end(v) + right(v))), so that neither neighbour can change
        // before the sequential loop reaches it; then nothing it makes is taken earlier than the
        // sequential loop would take it.  A non-eager candidate needs neither: every pair its
        // token n makes, with any neighbour, ranks above it (the monotone argument).  Model and
        // random non-monotone tables: tests/window_model.py, tests/test_window_rule.py.
        bool eg[4];
        uint32_t pu[4], tu[4], tv[4], nv[4], nn[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
          eg[g] = q[g] != kNoPos && serial_round(t, gm[g]);
          pu[g] = eg[g] ? (uint32_t)prv[cp[g]] : kNoPos;
          nn[g] = eg[g] ? new_id_of(t, gm[g]) : 0u;
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
          tu[g] = pu[g] != kNoPos ? (uint32_t)tok[pu[g]] : 0u;
          tv[g] = eg[g] && nq[g] != kNoPos ? (uint32_t)tok[nq[g]] : 0u;
          nv[g] = eg[g] && nq[g] != kNoPos ? (uint32_t)nxt[nq[g]] : kNoPos;
        }
        Probe<false, HOT> PL[4], PR[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
          PL[g].start(t, P, tu[g], nn[g], pu[g] != kNoPos);
          PR[g].start(t, P, nn[g], tv[g], eg[g] && nq[g] != kNoPos);
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
          if (!eg[g]) continue;
          const uint32_t rl = pu[g] != kNoPos ? PL[g].finish(t, sink) : kNoRank;
          const uint32_t rr = nq[g] != kNoPos ? PR[g].finish(t, sink) : kNoRank;
          if (rl <= gm[g] || rr <= gm[g]) {
            q[g] = kNoPos;  // (not a candidate this round)
            continue;
          }
          if (pu[g] != kNoPos) {
            const uint32_t wlu = t.wmeta[tu[g]] & 0xFFFFu;
            lo_x[g] = pu[g] >= wlu ? pu[g] - wlu : 0u;
          }
          if (nq[g] != kNoPos) end_x[g] = (nv[g] == kNoPos ? m : nv[g]) + (t.wmeta[tv[g]] >> 16);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; g++) {
        if (q[g] == kNoPos) continue;
        const uint32_t c = cp[g];
        const uint32_t lo = min(c >= wl[g] ? c - wl[g] : 0u, lo_x[g]);
        const uint32_t end = min(max((nq[g] == kNoPos ? m : nq[g]) + wr[g], end_x[g]), m);
        const uint32_t h0 = unit(lo), h1 = unit(end - 1), own = unit(c);
        if (h1 - h0 >= kWinGroups) continue;
        bool ok = true;
        for (uint32_t h = h0; h <= h1; h++)
          if (h != own && (uint32_t)gmin[h] <= gm[g]) {
            ok = false;
            break;
          }
        if (ok) bsites |= 1ull << cb[g];
      }
      sites |= bsites;
    }
    // A lane's sites go four at a time, the LDS reads (and in phase B the pair lookups, global
    // loads included) of the four in flight together: no read of a phase depends on a write of
    // the same phase (a site's right neighbour q is never a site; the left neighbour pp of a site
    // may be a site, whose phase-A writes the barrier orders first).
    constexpr int kB = 4;
    auto take = [&](uint64_t& rest, uint32_t (&p)[kB]) {
#pragma unroll
      for (int i = 0; i < kB; i++) {
        p[i] = rest ? pos((uint32_t)__builtin_ctzll(rest)) : kNone;
        rest &= rest - 1;
      }
    };
    // One pass (the common round: every site holds a pair (a, b) with a != b, all of them merge,
    // and no lane holds more than kB): the new pairs' tokens are read from the state before the
    // merges -- a site's right pair is (nid, the token after its right neighbour, nid when that
    // is a site itself), its left pair (the token before it, or nid with the site before that
    // when that one merges into it) -- so their lookups, global loads included, are in flight
    // while the merges are written, instead of after a second walk of the list.
    if (!eager && !chain_any && __ballot(__popcll(sites) > (uint32_t)kB || bsites != 0) == 0) {
      uint32_t p[kB], q[kB], pp[kB], nq[kB], ppp[kB], tpp[kB], rnq[kB], tnq[kB], rppp[kB];
      uint64_t rest = sites;
      take(rest, p);
#pragma unroll
      for (int i = 0; i < kB; i++) {
        q[i] = p[i] != kNone ? (uint32_t)nxt[p[i]] : kNoPos;
        pp[i] = p[i] != kNone ? (uint32_t)prv[p[i]] : kNoPos;
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        nq[i] = q[i] != kNoPos ? (uint32_t)nxt[q[i]] : kNoPos;
        ppp[i] = pp[i] != kNoPos ? (uint32_t)prv[pp[i]] : kNoPos;
        tpp[i] = pp[i] != kNoPos ? (uint32_t)tok[pp[i]] : 0u;
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        rnq[i] = nq[i] != kNoPos ? (uint32_t)rk[nq[i]] : kNoRank;
        tnq[i] = nq[i] != kNoPos ? (uint32_t)tok[nq[i]] : 0u;
        rppp[i] = ppp[i] != kNoPos ? (uint32_t)rk[ppp[i]] : kNoRank;
      }
      Probe<false, HOT> R[kB], L[kB];
      uint32_t lpos[kB];
#pragma unroll
      for (int i = 0; i < kB; i++) {
        const bool left_site = rppp[i] == r;  // (rank r: a site, which takes pp in)
        lpos[i] = left_site ? ppp[i] : pp[i];
        R[i].start(t, P, nid, rnq[i] == r ? nid : tnq[i], p[i] != kNone && nq[i] != kNoPos);
        L[i].start(t, P, left_site ? nid : tpp[i], nid, p[i] != kNone && pp[i] != kNoPos);
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        if (p[i] == kNone) continue;
        tok[p[i]] = nid;
        tok[q[i]] = kDead;
        rk[q[i]] = kNoRank;
        nxt[p[i]] = (uint16_t)nq[i];
        if (nq[i] != kNoPos) prv[nq[i]] = (uint16_t)p[i];
        dirty[unit(q[i])] = 1;
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        if (p[i] == kNone) continue;
        const uint32_t rr = R[i].finish(t, err), rl = L[i].finish(t, err);
        rk[p[i]] = nq[i] != kNoPos ? rr : kNoRank;
        dirty[unit(p[i])] = 1;
        if (pp[i] != kNoPos) {
          rk[lpos[i]] = rl;
          dirty[unit(lpos[i])] = 1;
        }
      }
      wave_sync_lds();
      continue;
    }
    // phase A: every selected site merges with its right neighbour (window rounds: each site
    // with its own rank's new id; no site is another site's right neighbour, whose rank this
    // phase overwrites)
    for (uint64_t rest = sites; rest;) {
      uint32_t p[kB], q[kB], nq[kB], np[kB];
      take(rest, p);
#pragma unroll
      for (int i = 0; i < kB; i++) {
        q[i] = p[i] != kNone ? (uint32_t)nxt[p[i]] : kNoPos;
        np[i] = nid;
        if (t.window && p[i] != kNone) np[i] = (uint32_t)rk[p[i]];
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        nq[i] = p[i] != kNone ? (uint32_t)nxt[q[i]] : kNoPos;
        if (t.window && p[i] != kNone) np[i] = new_id_of(t, np[i]);
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        if (p[i] == kNone) continue;
        tok[p[i]] = np[i];
        tok[q[i]] = kDead;
        rk[q[i]] = kNoRank;
        nxt[p[i]] = (uint16_t)nq[i];
        if (nq[i] != kNoPos) prv[nq[i]] = (uint16_t)p[i];
        dirty[unit(q[i])] = 1;
      }
    }
    wave_sync_lds();
    // phase B: the new pairs' ranks.  When the left neighbour pp is itself a site, its right-pair
    // lookup and this site's left-pair lookup are the same pair (nid, nid) and write the same rank.
    for (uint64_t rest = sites; rest;) {
      uint32_t p[kB], q[kB], pp[kB], tq[kB], tp[kB], ts[kB];
      take(rest, p);
#pragma unroll
      for (int i = 0; i < kB; i++) {
        q[i] = p[i] != kNone ? (uint32_t)nxt[p[i]] : kNoPos;
        pp[i] = p[i] != kNone ? (uint32_t)prv[p[i]] : kNoPos;
        ts[i] = nid;
        if (t.window && p[i] != kNone) ts[i] = (uint32_t)tok[p[i]];
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        tq[i] = q[i] != kNoPos ? (uint32_t)tok[q[i]] : 0u;
        tp[i] = pp[i] != kNoPos ? (uint32_t)tok[pp[i]] : 0u;
      }
      Probe<false, HOT> R[kB], L[kB];
#pragma unroll
      for (int i = 0; i < kB; i++) {
        R[i].start(t, P, ts[i], tq[i], q[i] != kNoPos);
        L[i].start(t, P, tp[i], ts[i], pp[i] != kNoPos);
      }
#pragma unroll
      for (int i = 0; i < kB; i++) {
        if (p[i] == kNone) continue;
        const uint32_t rr = R[i].finish(t, err), rl = L[i].finish(t, err);
        rk[p[i]] = q[i] != kNoPos ? rr : kNoRank;
        dirty[unit(p[i])] = 1;
        if (pp[i] != kNoPos) {
          rk[pp[i]] = rl;
          dirty[unit(pp[i])] = 1;
        }
      }
    }
    wave_sync_lds();
    // (no per-round read of the panic flag: a panicking pair ranks as kNoRank, so the loop still
    // ends, and the host discards the batch -- a global load per round would double its latency)
  }
  // surviving tokens in position order (rows of 64 positions, 16 rows' LDS reads at a time)
  uint32_t c = 0;
  for (uint32_t i0 = 0; i0 < m; i0 += 16 * 64) {
    uint32_t tv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t i = i0 + (uint32_t)j * 64 + lane;
      tv[j] = i < m ? (uint32_t)tok[i] : kDead;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t bal = __ballot(tv[j] != kDead);
      if (tv[j] != kDead) out[c + __popcll(bal & lanemask_lt())] = tv[j];
      c = uni(c + __popcll(bal));
    }
  }
  if (rounds) *rounds += nr;
  return c;
}

// Long-piece order.  k_long_len: a wavefront per long piece finds its length (parked in
// long_cnt until a tier overwrites it with the piece's id count) and counts the bucket of each
// piece > kDenseMax B (workgroup histogram in LDS, one global add per non-empty bucket);
// k_long_order: the buckets' exclusive scan (every workgroup computes it, workgroup 0 stores it)
// and the scatter of those pieces' list indices, longest bucket first (LDS ranks within a
// 256-piece step, one global reservation per bucket and step).  The segmented tiers take their
// pieces from their own range of long_ord through a counter: the longest pieces start first and
// a wave that finishes early takes the next one, so a tier's makespan is about its total rounds
// over its waves (with a static stride one wave could draw several of the longest pieces).
// Pieces <= kDenseMax B (many, short: a counter per piece would be a contended atomic each) are
// dealt to the dense tier by a static stride over the long list.
constexpr uint32_t kDenseMax = 256;

// (lwn[li]: the piece's length when the global-memory tier takes it (> gmin bytes), else 0; its
// scan places the pieces' state in lw, the scan of long_cnt places their ids in lids)
__global__ __launch_bounds__(256) void k_long_len(Work w, uint32_t* lwn, uint32_t gmin) {
  __shared__ uint32_t s_hist[kLhBuckets];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_long = uni(long_count(w));
  const uint32_t n_waves = gridDim.x * 4;
  if (threadIdx.x < (uint32_t)kLhBuckets) s_hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t li = uni(blockIdx.x * 4 + (threadIdx.x >> 6)); li < n_long; li += n_waves) {
    const uint64_t e = w.long_list[li];
    const uint32_t s = uni((uint32_t)e);
    const uint32_t kn = uni(long_len(e));  // (k_segment's, when the piece ended within its look-ahead)
    const uint32_t n = kn ? kn : uni(piece_end(w, s) - s);
    if (lane == 0) {
      w.long_cnt[li] = n;
      lwn[li] = n > gmin ? n : 0u;
      if (n > kDenseMax) atomicAdd(&s_hist[long_bucket(n)], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kLhBuckets && s_hist[threadIdx.x])
    atomicAdd(&w.long_hist[kLhHist + threadIdx.x], s_hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_long_order(Work w) {
  __shared__ uint32_t s_scan[kLhBuckets + 1], s_cnt[kLhBuckets], s_base[kLhBuckets];
  const uint32_t tid = threadIdx.x;
  const uint32_t n_long = long_count(w);
  if (tid == 0) {
    uint32_t a = 0;
    for (int d = 0; d < kLhBuckets; d++) {
      s_scan[d] = a;
      a += w.long_hist[kLhHist + d];
    }
    s_scan[kLhBuckets] = a;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid <= (uint32_t)kLhBuckets) w.long_hist[kLhScan + tid] = s_scan[tid];
  if (s_scan[kLhBuckets] == 0) return;  // no piece > kDenseMax B
  for (uint32_t b0 = blockIdx.x * 256; b0 < n_long; b0 += gridDim.x * 256) {
    if (tid < (uint32_t)kLhBuckets) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t li = b0 + tid;
    const uint32_t n = li < n_long ? w.long_cnt[li] : 0u;
    const uint32_t d = long_bucket(n);
    uint32_t r = 0;
    if (n > kDenseMax) r = atomicAdd(&s_cnt[d], 1u);
    __syncthreads();
    if (tid < (uint32_t)kLhBuckets && s_cnt[tid]) s_base[tid] = atomicAdd(&w.long_hist[kLhFill + tid], s_cnt[tid]);
    __syncthreads();
    if (n > kDenseMax) w.long_ord[s_scan[d] + s_base[d] + r] = li;
    __syncthreads();
  }
}

// One wavefront per piece of (LO, 64K] bytes; NW waves per workgroup, each taking the tier's
// pieces (a range of long_ord, longest first) from a counter.  LDS: the merge-table image (HOT:
// hot table + Bloom filter, 96 KiB; else the Bloom filter, 32 KiB) and one slice per wave.
template <int K, uint32_t LO, int NW, bool HOT, bool SEG>
__global__ __launch_bounds__(64 * NW) void k_bpe_wave(Work w, Tables t) {
  constexpr uint32_t kSlice = SEG ? SegSlice<K>::kBytes : WaveSlice<K>::kBytes;
  constexpr uint32_t HI = 64u * K;
  static_assert(HI <= 4096 && LO % 64 == 0 && LO < HI, "tier bounds: multiples of the 64 B buckets");
  extern __shared__ __attribute__((aligned(16))) uint4 s_dyn[];
  __shared__ int32_t s_b2id[256];
  constexpr uint32_t kImg = HOT ? kLdsImageBytes / 16 : kBloomWords / 4;  // uint4 units
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wid = uni(tid >> 6);
  static_assert(SEG ? LO >= kDenseMax : HI <= kDenseMax, "ordered tiers: > kDenseMax B; dense tier: <= kDenseMax B");
  const uint32_t n_long = uni(long_count(w));
  const uint32_t lo = SEG ? uni(w.long_hist[kLhScan + kLhBuckets - HI / 64]) : 0u;
  const uint32_t hi = SEG ? uni(w.long_hist[kLhScan + kLhBuckets - LO / 64]) : n_long;
  // (a workgroup past the tier's piece count has nothing to take: return before the image load;
  // the dense tier's workgroups check that they meet a piece of the tier)
  if (lo >= hi || blockIdx.x * NW >= hi - lo) return;
  if constexpr (!SEG) {
    __shared__ uint32_t s_any;
    if (tid == 0) s_any = 0;
    __syncthreads();
    for (uint32_t li = blockIdx.x * NW + wid; li < n_long; li += gridDim.x * NW) {
      if (w.long_cnt[li] <= HI) {
        if (lane == 0) s_any = 1;
        break;
      }
    }
    __syncthreads();
    if (s_any == 0) return;
  }
  // (HOT: hot table + the filter of the other pairs; else the filter of all pairs, stored after
  // the image)
  const uint4* img = HOT ? t.lds_image : t.lds_image + kLdsImageBytes / 16;
  for (uint32_t i = tid; i < kImg; i += 64 * NW) s_dyn[i] = img[i];
  for (uint32_t i = tid; i < 256; i += 64 * NW) s_b2id[i] = t.byte2id[i];
  __syncthreads();
  const PairLds P = HOT ? PairLds{(const lds_u64*)s_dyn, (const lds_u32*)(s_dyn + kHotBuckets)}
                        : PairLds{nullptr, (const lds_u32*)s_dyn};
  lds_u32* slice = (lds_u32*)((__attribute__((address_space(3))) uint8_t*)(s_dyn + kImg) + (size_t)wid * kSlice);
  uint32_t* err = &w.counters[kCtrErr];
  uint32_t rounds = 0;  // this wave's rounds over its pieces (statistics; one atomic at the end)
  for (uint32_t step = uni(blockIdx.x * NW + wid);; step += gridDim.x * NW) {
    uint32_t li;
    if constexpr (SEG) {
      // every lane takes part (lane 0 adds 1, the others 0): no divergent branch around the
      // atomic, whose structurised form (a divergent loop exit) once re-ran a piece forever
      const uint32_t k = uni(atomicAdd(&w.long_hist[kLhTake + HI / 64], lane == 0 ? 1u : 0u));
      if (k >= hi - lo) break;
      li = uni(w.long_ord[lo + k]);
    } else {
      if (step >= n_long) break;
      li = step;
    }
    const uint32_t n = uni(w.long_cnt[li]);
    if (!SEG && n > HI) continue;
    const uint64_t e = w.long_list[li];
    const uint32_t s = uni((uint32_t)e);
    const uint32_t o = uni(long_ord(e));
    uint32_t cnt;
    uint32_t* sink = &w.counters[kCtrSink];
    uint32_t* out = w.lids + w.long_pos[li];
    if constexpr (SEG) cnt = bpe_wave_seg<K, HOT>(t, P, s_b2id, w.text + s, n, SegSlice<K>{slice}, out, err, sink, &rounds);
    else cnt = bpe_wave_dense<K, HOT>(t, P, s_b2id, w.text + s, n, WaveSlice<K>{slice}, out, err, sink, &rounds);
    if (lane == 0) {
      const uint32_t tile = s / kTile;
      w.long_cnt[li] = cnt;
      w.mrec[(size_t)tile * kTileSlots + o] = kRecLong | li;
      atomicAdd(&w.tile_tok[tile], cnt);
    }
  }
  if (lane == 0 && rounds) atomicAdd(&w.counters[kCtrRounds], rounds);
}

template <int K, uint32_t LO, int NW, bool HOT, bool SEG>
static hipError_t launch_wave(const Work& w, const Tables& t, uint32_t grid, hipStream_t s) {
  static LdsAttr attr;
  const size_t slice = SEG ? SegSlice<K>::kBytes : WaveSlice<K>::kBytes;
  const size_t lds = (HOT ? kLdsImageBytes : kBloomWords * 4) + (size_t)NW * slice;
  HIPCHK(lds_attr_once(attr, (const void*)k_bpe_wave<K, LO, NW, HOT, SEG>, lds));
  k_bpe_wave<K, LO, NW, HOT, SEG><<<grid, 64 * NW, lds, s>>>(w, t);
  return hipGetLastError();
}

// Long-piece preparation (side stream): lengths and the tiers' order (k_long_len, k_long_order),
// then the places of every piece's ids in lids (scan of the lengths: ids <= bytes) and of the
// global-memory tier's state in lw (scan of lwn).  long_pos[n_long] / lw_pos[n_long] hold the
// totals, which the host reads back to size lids and lw before it launches the tiers.
hipError_t launch_long_prep(const Work& w, const Tables& t, hipStream_t s, uint32_t n_long, uint32_t* lwn,
                            uint32_t* tmp, uint64_t tmp_cap) {
  if (n_long == 0) return hipSuccess;
  auto cap = [](uint32_t want, uint32_t most) { return std::max(1u, std::min(want, most)); };
  const bool added = t.n_at != 0 || t.dbg == 7;
  HIPCHK(hipMemsetAsync(w.long_hist, 0, kLhWords * sizeof(uint32_t), s));
  k_long_len<<<cap((n_long + 3) / 4, 4 * w.n_cus), 256, 0, s>>>(w, lwn, added ? kLdsPos : kWaveMax);
  if (!added) k_long_order<<<cap((n_long + 255) / 256, w.n_cus), 256, 0, s>>>(w);
  HIPCHK(hipGetLastError());
  HIPCHK(scan_u32(w.long_cnt, w.long_pos, n_long, nullptr, tmp, tmp_cap, s));
  return scan_u32(lwn, w.lw_pos, n_long, nullptr, tmp, tmp_cap, s);
}

// any_gmem: some long piece is longer than the LDS tiers take (launch_long_prep's global-memory
// state total is non-zero); without one the global-memory tier is not launched (it would still
// find every long piece's end to skip it: 0.33 ms on C5)
hipError_t launch_bpe_long(const Work& w, const Tables& t, hipStream_t s, uint32_t n_long, bool any_c3, bool any_gmem) {
  auto cap = [](uint32_t want, uint32_t most) { return std::max(1u, std::min(want, most)); };
  if (t.n_at != 0 || t.dbg == 7) {
    // added tokens can match inside pieces: the linked-list kernel with the added-token split.
    // One wavefront per workgroup (32 KiB of LDS each): a long-piece workgroup fits on a CU next
    // to a merge-pass workgroup (96 KiB), so this pass overlaps them instead of taking CUs away
    if (n_long == 0) return hipSuccess;
    const size_t lds = 4 * kLdsPos * sizeof(uint32_t);
    k_bpe_long<false><<<cap(n_long, 512), 64, lds, s>>>(w, t);
    if (any_gmem) k_bpe_long<true><<<cap((n_long + 3) / 4, 128), 256, 0, s>>>(w, t);
    return hipGetLastError();
  }
  if (n_long) {
    // dense wave tiers: <= 256 B (4 waves per workgroup, Bloom filter only, 43 KiB of LDS: fits
    // next to a merge-pass workgroup), 257..1024 B (segmented, 2 waves per workgroup with the
    // whole image) and 1025..4096 B (segmented, 2 waves with the Bloom filter); longer pieces:
    // GMEM linked list.  Grids: at most one wave per long piece.  (launch_long_prep first: the
    // lengths, the longest-first order of the segmented tiers' pieces, the id places.)
    // The long list holds pieces > kMedMax B and pieces whose end lies past the tile's look-ahead
    // (>= 63 B: they can be shorter than kMedMax), and a tile's class-0 pieces past its list's
    // capacity, so the first tier starts at 1 B.
    // <= 256 B: 16 waves per workgroup, one workgroup per CU (75 KiB of LDS).  A round is a chain
    // of LDS and global round trips, so waves per CU is the lever: C5 31.4 -> 34.5 GB/s against
    // 4 waves x 2 workgroups per CU (which could share a CU with a wide-vocabulary merge pass;
    // profiles/r03/v36_ab_dense_waves.txt)
    // (The A/B launches that lost, CTOK_DBG_MODE 9, 10, 12 and 16, are kept as profiles/kernels_split/patches/
    // long_tier_ab_arms.diff; their results: profiles/r02/v14_ab_long_tiers.txt, r03/v36_*, r03/v37_*, r06/v50_v51_*.)
    HIPCHK((launch_wave<4, 0, 16, false, false>(w, t, cap((n_long + 15) / 16, w.n_cus), s)));
    if (t.dbg == 15) {  // A/B: 257..1024 B, 8 waves per CU with the Bloom filter only
      HIPCHK((launch_wave<16, 256, 8, false, true>(w, t, cap((n_long + 7) / 8, w.n_cus), s)));
    } else {
      HIPCHK((launch_wave<16, 256, 2, true, true>(w, t, cap((n_long + 1) / 2, w.n_cus), s)));
    }
    // 1025..4096 B: two waves per CU with the Bloom filter only (32 + 2 x 53 KiB) beat one wave
    // with the hot table (96 + 53 KiB): C3 10.3 -> 5.25 ms (profiles/r02/v14_ab_long_tiers.txt)
    HIPCHK((launch_wave<64, 1024, 2, false, true>(w, t, cap((n_long + 1) / 2, w.n_cus), s)));
    if (any_gmem) k_bpe_long<true><<<cap((n_long + 3) / 4, 128), 256, 0, s>>>(w, t);
    HIPCHK(hipGetLastError());
  }
  // 33..64 B register pass, side-stream instance (see k_bpe_mid): it shares class 3 with the main
  // instance as the long tiers free CUs; with no long pieces the main instance alone runs it
  if (!any_c3 || n_long == 0) return hipSuccess;
  // (kernels.hip's case 4 is launch_mid<C, 3>(w, t, s); t.n_at != 0 returned at the top of this function)
  return launch_bpe_class(w, t, 4, s);
}

}  // namespace ctok_dev
