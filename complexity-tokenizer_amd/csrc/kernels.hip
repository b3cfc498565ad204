// Encode path, stage 2: the merge passes over the per-tile class lists -- k_bpe_generic (added
// tokens, dropped bytes), k_bpe_short (<= 8 B, 9..16 B, 17..32 B packed), k_bpe_mid (17..32 B,
// 33..64 B), k_bpe_sparse (few 33..64 B pieces) (DESIGN.md sections 4.2, 4.2b and 4.4).  (The
// file's name is from when it held every stage; the others are segment.hip, long.hip, emit.hip,
// scan.hip, nfc.hip.)
#include "dev_common.h"
#include "pair_lookup_dev.h"

#include "chunk_sort_hd.h"
#include "merge_packed_hd.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// Merge passes over the per-tile class lists.  Workgroup b takes K consecutive tiles and treats
// their lists as one concatenated list (prefix of the K counts in LDS); entry q -> its tile by a
// binary search over those K offsets.  Token counts are summed per tile in LDS and added to
// tile_tok with one atomic per (workgroup, tile); no two workgroups share a (class, tile).

// s_tsum[l] starts at tile t0 + l's region base for class cls (tregion, cls >= 0) or at 0: the
// merge passes allocate their ids from it (and add the difference to tile_tok at the flush).
// (K <= 256 tiles: the first K/64 waves scan 64 counts each, then add the earlier waves' totals;
// the workgroup has at least K threads)
template <int K>
__device__ __forceinline__ uint32_t tile_share_init(const uint32_t* counts, uint32_t n_tiles, uint32_t t0,
                                                    uint32_t* s_pre, uint32_t* s_tsum, const uint2* tregion = nullptr,
                                                    int cls = -1, uint32_t* s_tbase = nullptr) {
  static_assert(K >= 1 && K <= 256 && (K & (K - 1)) == 0, "K: power of two <= 256");
  constexpr uint32_t kW = (K + 63) / 64;
  __shared__ uint32_t s_wsum[4];
  const uint32_t l = threadIdx.x, wv = l >> 6;
  const bool in = l < K && t0 + l < n_tiles;
  uint32_t c = 0, inc = 0;
  if (wv < kW) {
    c = in ? counts[t0 + l] : 0u;
    inc = wave_incl_scan(c);
    if (kW > 1 && (l & 63) == 63) s_wsum[wv] = inc;
  }
  if constexpr (kW > 1) __syncthreads();
  if (wv < kW) {
#pragma unroll
    for (uint32_t v = 0; v + 1 < kW; v++) inc += v < wv ? s_wsum[v] : 0u;
    if (l < K) {
      s_pre[l] = inc - c;
      uint32_t b0 = 0;
      if (cls > 0 && in) b0 = region_base(tregion[t0 + l], cls);
      s_tsum[l] = b0;
      if (s_tbase) s_tbase[l] = b0;
    }
    if (l == (K < 64 ? 63u : (uint32_t)K - 1)) s_pre[K] = inc;
  }
  __syncthreads();
  return s_pre[K];
}

template <int K>
__device__ __forceinline__ uint32_t tile_of(const uint32_t* s_pre, uint32_t q) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = K / 2; step >= 1; step >>= 1)
    if (s_pre[lo + step] <= q) lo += step;
  return lo;
}

template <int K>
__device__ __forceinline__ void tile_share_flush(const Work& w, uint32_t t0, uint32_t t1, const uint32_t* s_tsum,
                                                 const uint32_t* s_tbase = nullptr, int cls = -1) {
  __syncthreads();
  if (threadIdx.x < K && t0 + threadIdx.x < t1) {
    const uint32_t v = s_tsum[threadIdx.x] - (s_tbase ? s_tbase[threadIdx.x] : 0u);
    if (v) atomicAdd(&w.tile_tok[t0 + threadIdx.x], v);
    if (cls >= 0 && v) w.rend[(size_t)cls * w.n_tiles + t0 + threadIdx.x] = s_tsum[threadIdx.x];
  }
}

constexpr int kTilesGeneric = 2;  // tiles per workgroup, generic pass over list0

// Generic thread-per-piece kernel (LDS working arrays; handles dropped bytes and added tokens).
// MID = false: every piece of list0 (launched instead of the register passes when the tokenizer
// has added tokens that can match inside a piece); MID = true: the pieces the register passes
// found to contain a byte whose char is not in the vocab (mid_list).
// MID pieces can be up to kMedMax bytes (class 3 finds them too): 64 slots, 128 threads.
template <bool MID>
__global__ __launch_bounds__(MID ? 128 : 256) void k_bpe_generic(Work w, Tables t) {
  if (spec_failed(w)) return;
  constexpr uint32_t NT = MID ? 128 : 256;
  constexpr uint32_t SLOTS = MID ? kMedMax : kShortMax;
  __shared__ uint32_t s_tok[SLOTS * NT];
  __shared__ uint32_t s_rk[SLOTS * NT];
  __shared__ int32_t s_b2id[256];
  __shared__ uint32_t s_pre[kTilesGeneric + 1], s_tsum[kTilesGeneric];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < 256; i += NT) s_b2id[i] = t.byte2id[i];
  uint32_t* err = &w.counters[kCtrErr];
  uint32_t E, t0 = 0;
  if (MID) {
    __syncthreads();
    E = min(w.counters[kCtrDropped], w.mid_cap);
  } else {
    t0 = blockIdx.x * kTilesGeneric;
    E = tile_share_init<kTilesGeneric>(w.tcls, w.n_tiles, t0, s_pre, s_tsum);
  }
  const uint32_t stride = MID ? gridDim.x * NT : NT;
  for (uint32_t q = (MID ? blockIdx.x * NT : 0) + tid; q < E; q += stride) {
    uint32_t s, o, n, tile, kt = 0;  // o: the piece's ordinal (its mrec slot)
    if (MID) {
      const uint64_t e = w.mid_list[q];
      s = (uint32_t)e;
      o = (uint32_t)(e >> 32) & 0xFFFu;
      n = (uint32_t)(e >> 48);
      tile = s / kTile;
    } else {
      kt = tile_of<kTilesGeneric>(s_pre, q);
      tile = t0 + kt;
      const uint32_t e = w.list0[(size_t)tile * w.k0 + (q - s_pre[kt])];
      s = tile * kTile + (e & 0xFFFu);
      o = ent_ord(e);
      n = ent_len(e);
    }
    const uint8_t* bytes = w.text + s;
    // ids go to the tile's region of the piece's length class, after what the merge passes used
    // there (the region holds the bytes of every piece of the class: ids <= bytes)
    const uint32_t cl = n <= 8 ? 0u : n <= 16 ? 1u : n <= 32 ? 2u : 3u;
    const uint32_t pos = atomicAdd(&w.rend[(size_t)(MID ? cl : 0u) * w.n_tiles + tile], n);
    uint32_t* out = w.scratch + (size_t)tile * kTileSlots + pos;
    uint32_t cnt = 0;
    if (t.n_at == 0) {
      cnt = bpe_short<NT>(t, bytes, n, s_b2id, s_tok, s_rk, tid, out, err);
    } else {
      // added-token split of the word (src/huggingface/mod.rs:566-610), on raw bytes
      uint32_t pos = 0;
      while (pos < n) {
        int32_t best = -1;
        uint32_t blen = 0;
        for (uint32_t k = 0; k < t.n_at; k++) {
          const uint32_t m = t.at_off[k + 1] - t.at_off[k];
          if (AddedMatch::find(t, k, bytes + pos, n - pos) == 0 && (best < 0 || m > blen)) { best = (int32_t)k; blen = m; }
        }
        if (best >= 0) { out[cnt++] = t.at_id[best]; pos += blen; continue; }
        uint32_t nxt = n - pos;
        for (uint32_t k = 0; k < t.n_at; k++) {
          const int64_t f = AddedMatch::find(t, k, bytes + pos, n - pos);
          if (f > 0 && (uint32_t)f < nxt) nxt = (uint32_t)f;
        }
        cnt += bpe_short<NT>(t, bytes + pos, nxt, s_b2id, s_tok, s_rk, tid, out + cnt, err);
        pos += nxt;
      }
    }
    w.mrec[(size_t)tile * kTileSlots + o] = rec_short(cnt, pos);
    if (MID) atomicAdd(&w.tile_tok[tile], cnt);
    else atomicAdd(&s_tsum[kt], cnt);
  }
  if (!MID) tile_share_flush<kTilesGeneric>(w, t0, w.n_tiles, s_tsum);
}

// ------------------------------------------------------------------------------------------
// BPE fast path: pieces of <= N bytes merged by one thread with the tokens and pair ranks in
// registers (fully unrolled, compile-time slot indices; no LDS for the working set, so occupancy
// is set by VGPRs alone).  All first-probe loads of the initial pairs issue back to back.

template <int N> struct LdsClass;
template <> struct LdsClass<8> { static constexpr int cls = 0; static constexpr uint32_t cap = kCap0; };
template <> struct LdsClass<16> { static constexpr int cls = 1; static constexpr uint32_t cap = kCap1; };
template <> struct LdsClass<32> { static constexpr int cls = 2; static constexpr uint32_t cap = kCap2; };
template <> struct LdsClass<64> { static constexpr int cls = 3; static constexpr uint32_t cap = kCap3; };

template <int N>
__device__ __forceinline__ const uint32_t* class_list(const Work& w) {
  return N == 8 ? w.list0 : N == 16 ? w.list1 : N == 32 ? w.list2 : w.list3;
}
template <int N>
__device__ __forceinline__ uint32_t class_cap(const Work& w) {
  return N == 8 ? w.k0 : LdsClass<N>::cap;
}

// The merge loop on the first N register slots of tk / rk (compile-time indices only, so the
// arrays stay in registers): branch-free over the slots, the lowest (rank, position) pair is
// merged, the slots right of it shift left by one, the two new pairs' ranks are looked up.
// Returns true when it stopped because the piece shrank to <= stop tokens (the caller continues
// on fewer slots), false when no pair can merge.  Slots >= m hold kDead / kNoRank.
template <int N, bool COMPACT, bool HOT, bool NARROW>
__device__ __forceinline__ bool merge_slots(const Tables& t, const PairLds& P, uint32_t* tk, uint32_t* rk,
                                            uint32_t& m, uint32_t stop, uint32_t* err) {
  for (;;) {
    if (m <= stop) return true;
    uint32_t key = ~0u;  // rank << 6 | position: one v_min per slot (ranks < 2^22, N <= 64)
#pragma unroll
    for (int k = 0; k < N - 1; k++) key = min(key, (rk[k] << 6) | (uint32_t)k);
    const uint32_t best = key >> 6, bi = key & 63u;
    if (best == kNoRank) return false;
    const uint32_t nid = COMPACT ? best : t.rank_newid[best];
    uint32_t L = 0, R = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
      L = ((uint32_t)k + 1 == bi) ? tk[k] : L;
      R = ((uint32_t)k == bi + 2) ? tk[k] : R;
    }
    const bool has_l = bi > 0, has_r = bi + 2 < m;
    Probe<NARROW, HOT> pl, pr;
    pl.start(t, P, L, nid, has_l);
    pr.start(t, P, nid, R, has_r);
#pragma unroll
    for (int k = 0; k < N; k++) {  // ascending: tk[k+1] is read before it is overwritten
      const uint32_t nxt_t = k + 1 < N ? tk[k + 1] : kDead;
      const uint32_t nxt_r = k + 1 < N ? rk[k + 1] : kNoRank;
      const bool gt = (uint32_t)k > bi;
      tk[k] = gt ? nxt_t : ((uint32_t)k == bi ? nid : tk[k]);
      rk[k] = gt ? nxt_r : rk[k];
    }
    m--;
    const uint32_t rl = has_l ? pl.finish(t, err) : kNoRank;
    const uint32_t rr = has_r ? pr.finish(t, err) : kNoRank;
#pragma unroll
    for (int k = 0; k < N - 1; k++)
      rk[k] = ((uint32_t)k + 1 == bi) ? rl : (((uint32_t)k == bi) ? rr : rk[k]);
  }
}

// The last tier (<= 8 tokens) with the working state in LDS instead of registers: positions stay
// fixed, a live mask says which slots still hold a token, and slot s keeps the key
// rank << 3 | s of the pair its token starts (~0 when the slot is dead or last).  A merge then
// reads the keys (four ds_read2st64, a v_min tree), writes three keys and one token, and reads its
// two neighbours by index; the register tiers' N-wide select / shift chains (~100 VALU per merge
// at N = 8) are gone.  Tokens are u16 (narrow vocabularies: every id < 2^16), so 1024 threads'
// state (48 B each) fits beside the 96 KiB image.  Pair lookups use the 32-bit-key tables.
//   keys:   s_key[s * NT + tid] (u32; read two at a time with ds_read2st64)
//   tokens: s_tok[s * NT + tid] (u16)
// Semantics are merge_slots': the lowest (rank, position) pair merges (src/bpe.rs:118-149).

// out_of(m) returns where the piece's m ids go (called once, after the last merge).
// merge_lds8_run: the loop on a state already in LDS (merge_lds8 stores it from u32 registers,
// the packed 16-slot tier from its u16 pairs).
template <bool COMPACT, bool HOT, uint32_t NT, typename OutOf>
__device__ __forceinline__ uint32_t merge_lds8_run(const Tables& t, const PairLds& P, uint32_t m, lds_u32* s_key,
                                                   lds_u16* s_tok, uint32_t* err, OutOf&& out_of) {
  const uint32_t tid = threadIdx.x;
  // live slots, with a sentinel at bit 8 (so every "next live" search finds a bit)
  uint32_t lv = ((1u << m) - 1u) | 0x100u;
  for (;;) {
    uint32_t kk[8];
#pragma unroll
    for (int k = 0; k < 8; k++) kk[k] = s_key[k * NT + tid];
    const uint32_t best = min(min(min(kk[0], kk[1]), min(kk[2], kk[3])), min(min(kk[4], kk[5]), min(kk[6], kk[7])));
    if (best >= (kNoRank << 3)) break;
    const uint32_t bi = best & 7u, r = best >> 3;
    // (ids < 2^16: the mask lets the hashes use 24-bit multiplies)
    const uint32_t nid = (COMPACT ? r : t.rank_newid[r]) & 0xFFFFu;
    const uint32_t p = bi + 1 + (uint32_t)__builtin_ctz(lv >> (bi + 1));  // the right token's slot
    const uint32_t q = p + 1 + (uint32_t)__builtin_ctz(lv >> (p + 1));    // the token after it (8: none)
    const bool has_r = q < 8;
    const uint32_t lo = lv & ((1u << bi) - 1u);
    const bool has_l = lo != 0;
    const uint32_t pv = 31u - (uint32_t)__builtin_clz(lo | 1u);           // the token before
    const uint32_t L = s_tok[pv * NT + tid], R = s_tok[min(q, 7u) * NT + tid];
    s_tok[bi * NT + tid] = (uint16_t)nid;
    s_key[p * NT + tid] = ~0u;
    lv &= ~(1u << p);
    m--;
    Probe<true, HOT> pl, pr;
    pl.start(t, P, L, nid, has_l);
    pr.start(t, P, nid, R, has_r);
    const uint32_t rl = pl.finish(t, err), rr = pr.finish(t, err);
    if (has_l) s_key[pv * NT + tid] = (rl << 3) | pv;
    s_key[bi * NT + tid] = has_r ? (rr << 3) | bi : ~0u;
  }
  // live tokens in slot order to out[0 .. m)
  uint32_t* out = out_of(m);
#pragma unroll
  for (int k = 0; k < 8; k++)
    if ((lv >> k) & 1u) out[__popc(lv & ((1u << k) - 1u))] = s_tok[k * NT + tid];
  return m;
}

template <bool COMPACT, bool HOT, uint32_t NT, typename OutOf>
__device__ __forceinline__ uint32_t merge_lds8(const Tables& t, const PairLds& P, const uint32_t* tk, const uint32_t* rk,
                                               uint32_t m, lds_u32* s_key, lds_u16* s_tok, uint32_t* err,
                                               OutOf&& out_of) {
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    s_key[k * NT + tid] = (uint32_t)k + 1 < m ? (rk[k] << 3) | (uint32_t)k : ~0u;
    s_tok[k * NT + tid] = (uint16_t)tk[k];
  }
  return merge_lds8_run<COMPACT, HOT, NT>(t, P, m, s_key, s_tok, err, out_of);
}

// The packed tiers (merge_packed_hd.h) over the pass's tables: the two lookups of a step as
// Probe<true, HOT>, their loads in flight while the step moves its slots.  Compact tables only
// (Tables::short_packed): a value is the merged token's id.
template <bool HOT>
struct Lookup16 {
  const Tables& t;
  const PairLds& P;
  uint32_t* err;
  Probe<true, HOT> pl, pr;
  bool has_l = false, has_r = false;
  __device__ __forceinline__ uint32_t new_id(uint32_t v) const { return v; }
  __device__ __forceinline__ void start(uint32_t L, uint32_t nid, uint32_t R, bool hl, bool hr) {
    has_l = hl;
    has_r = hr;
    pl.start(t, P, L, nid, hl);
    pr.start(t, P, nid, R, hr);
  }
  // (kNoRank's low 16 bits are mpk::kNone; every other value is < 0xFFFF: Tables::short_packed)
  __device__ __forceinline__ void finish(uint32_t& rl, uint32_t& rr) {
    rl = (has_l ? pl.finish(t, err) : kNoRank) & 0xFFFFu;
    rr = (has_r ? pr.finish(t, err) : kNoRank) & 0xFFFFu;
  }
};

template <int K0, int K1, uint32_t NT>
__device__ __forceinline__ void lds8_store_packed(const uint32_t (&T)[8], const uint32_t (&R)[8], lds_u32* s_key,
                                                  lds_u16* s_tok) {
  if constexpr (K0 < K1) {
    s_key[K0 * NT + threadIdx.x] = mpk::lds8_key<K0>(R);
    s_tok[K0 * NT + threadIdx.x] = (uint16_t)mpk::half<K0>(T);
    lds8_store_packed<K0 + 1, K1, NT>(T, R, s_key, s_tok);
  }
}
template <int K0, int K1, int ND>
__device__ __forceinline__ void store_packed_ids(const uint32_t (&T)[ND], uint32_t m, uint32_t* out) {
  if constexpr (K0 < K1) {
    if ((uint32_t)K0 < m) out[K0] = mpk::half<K0>(T);
    store_packed_ids<K0 + 1, K1>(T, m, out);
  }
}

// A piece with a byte char absent from the vocabulary (dropped by the reference) is left to the
// generic pass: piece at byte s, ordinal o, n bytes appended to mid_list, the overflow bit when full.
__device__ __forceinline__ void defer_to_generic(const Work& w, uint32_t s, uint32_t o, uint32_t n) {
  const uint32_t mi = atomicAdd(&w.counters[kCtrDropped], 1u);
  if (mi < w.mid_cap)
    w.mid_list[mi] = (uint64_t)s | ((uint64_t)o << 32) | ((uint64_t)n << 48);
  else
    atomicOr(&w.counters[kCtrOverflow], 1u);
}

// Workgroup-shared scratch of a merge pass.
// (KT: the most tiles per chunk of the passes that share it)
template <uint32_t SORTCAP, int KT = 64>
struct PassLds {
  uint32_t pre[KT + 1], tsum[KT], tbase[KT], stat[2], bcnt[csort::kMaxBuckets], bfill[csort::kMaxBuckets], chunk, take, next;
  uint16_t perm[SORTCAP];  // the chunk's first SORTCAP entries ordered by length bucket
};

// Counting sort of the chunk's first Es <= SORTCAP list entries by csort::code (chunk_sort_hd.h)
// into S.perm; the order within a bucket is free.  Each entry is read once: thread tid owns
// entries tid, tid + NT, ... (unrolled in groups of four whose tile bisections and list loads are
// all in flight together) and takes its rank within the bucket from one returning
// add on the bucket's workgroup counter (ds_add_rtn_u32; S.bcnt, zero on entry), keeps code and
// rank packed in a register, and after the counters' scan by the first wave stores the entry
// number at base + rank.  (Counters per wave would not be faster -- the LDS serialises the lanes of
// one instruction that hit one address, not the waves -- and would cost 1 KiB of the sort buffer;
// a ballot per bucket costs its instructions once per bucket, 8 or 16 here.)
template <int N, int K, uint32_t NT, uint32_t SORTCAP, class PL>
__device__ __forceinline__ void chunk_sort(PL& S, const uint32_t* list, uint32_t c0, uint32_t cap, uint32_t Es,
                                           uint32_t mode) {
  static_assert(SORTCAP <= 65536, "perm holds u16 entry numbers, a rank fits 16 bits");
  constexpr uint32_t G = 4, EPT = (SORTCAP + G * NT - 1) / (G * NT) * G;  // entries per thread, whole groups
  uint32_t tid = threadIdx.x;
  // (opaque: what is derived from it is computed here, per chunk, instead of being hoisted out of
  // the chunk loop and held in registers through the piece loop, which has none to spare)
  asm volatile("" : "+v"(tid));
  uint32_t cr[EPT];  // code << 16 | rank (compile-time indices only)
#pragma unroll
  for (uint32_t j = 0; j < EPT; j++) cr[j] = 0;
#pragma unroll
  for (uint32_t g = 0; g < EPT; g += G) {
    if (g * NT < Es) {  // workgroup-uniform
      uint32_t e[G];
#pragma unroll
      for (uint32_t j = 0; j < G; j++) {
        // (no branch: the group's bisections interleave; a thread past the end reads the last entry)
        const uint32_t q = min(tid + (g + j) * NT, Es - 1);
        const uint32_t kt = tile_of<K>(S.pre, q);
        e[j] = list[(size_t)(c0 + kt) * cap + (q - S.pre[kt])];
      }
#pragma unroll
      for (uint32_t j = 0; j < G; j++) {
        if (tid + (g + j) * NT < Es) {
          const uint32_t c = csort::code(N, mode, ent_len(e[j]));
          cr[g + j] = (c << 16) | atomicAdd(&S.bcnt[c], 1u);
        }
      }
    }
  }
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the bucket sizes
    const uint32_t c = tid < csort::kMaxBuckets ? S.bcnt[tid] : 0u;
    const uint32_t inc = wave_incl_scan(c);
    if (tid < csort::kMaxBuckets) S.bfill[tid] = inc - c;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < EPT; j++) {
    const uint32_t q = tid + j * NT;
    if (q < Es) S.perm[S.bfill[cr[j] >> 16] + (cr[j] & 0xFFFFu)] = (uint16_t)q;
  }
  __syncthreads();
}

// Merge pass over one length class (N = 8, 16, 32 slots), run by a persistent grid:
// workgroups take chunks of w.unit-tile units from a counter (up to KT / w.unit units at once when the
// previous chunk left most of the workgroup idle: sparse classes) (counters[ctr_chunk(class)]) and walk the chunk's
// class lists as one concatenated list (see tile_share_init).  Thread per piece, tokens and pair
// ranks in registers (fully unrolled, compile-time slots).
// `load` fills the workgroup's LDS tables (image, byte -> id); it runs at the first chunk with
// work, so a workgroup that finds only empty lists never reads the 32..96 KiB image (`loaded`
// is shared by the passes of one kernel).
// L8: the <= 8-token tier runs in LDS (merge_lds8, narrow vocabularies; s_key / s_tok its state).
// PK (N = 16 or 32, L8): the 16-slot tier, and at N = 32 the 32-slot tier before it, keep tokens
// and values as u16 pairs (merge_packed_hd.h; tables whose values all fit,
// Tables::short_packed).
// LA: the pipeline loads the next piece's text one block ahead (N / 4 + 1 registers held through the
// merges); without it only the list entry is looked ahead and a piece loads its own text.
template <int N, bool COMPACT, bool HOT, uint32_t NT, uint32_t SORTCAP, bool L8 = false, int KT = 64, bool PK = false,
          bool LA = true, typename Load, int SKT>
__device__ __forceinline__ void class_pass(const Work& w, const Tables& t, const PairLds& P, const int32_t* s_b2id,
                                           PassLds<SORTCAP, SKT>& S, bool& loaded, Load&& load,
                                           lds_u32* s_key = nullptr, lds_u16* s_tok = nullptr) {
  using LC = LdsClass<N>;
  constexpr int K = KT;
  static_assert(KT <= (int)NT, "a thread per chunk tile");
  static_assert(KT <= SKT, "the shared scratch holds the pass's chunk");
  const uint32_t tid = threadIdx.x;
  uint32_t* err = &w.counters[kCtrErr];
  const uint32_t* list = class_list<N>(w);
  const uint32_t cap = class_cap<N>(w);
  const uint32_t* counts = w.tcls + (size_t)LC::cls * w.n_tiles;
  uint32_t st_bytes = 0, st_ids = 0;
  if (tid < 2) S.stat[tid] = 0;
  // The chunk's entries are walked by length bucket (chunk_sort_hd.h: exact byte lengths in the
  // 9..16 B and 17..32 B passes): a wavefront's pieces then have the same trip counts in the tiers,
  // and few of its lanes idle while the longest piece finishes.  Longest bucket first, so that the
  // short merge chains are the ones at the chunk's barrier (shortest first: +0.08 ms on C4).
  // (Work::chunk_sort selects the A/B arms; it is a kernel argument, read per chunk outside the
  // piece loop.)
  const uint32_t mode = w.chunk_sort;
  // chunks of K tiles dealt dynamically (one atomic per chunk, taken by thread 0 and broadcast
  // through LDS): workgroups that start late, or whose CU is shared, take fewer chunks
  __syncthreads();
  uint32_t take = 1;  // units of the next chunk (workgroup-uniform)
  const uint32_t U = w.unit;
  for (;;) {
    if (tid == 0) {
      S.chunk = atomicAdd(&w.counters[ctr_chunk(LC::cls)], take);
      S.take = take;
      S.next = 0;
    }
    if (tid < csort::kMaxBuckets) S.bcnt[tid] = 0;  // (chunk_sort's counters)
    __syncthreads();
    const uint32_t c0 = S.chunk * U;
    if (c0 >= w.n_tiles) break;
    const uint32_t tb1 = min(w.n_tiles, c0 + U * S.take);
    const uint32_t E = tile_share_init<K>(counts, tb1, c0, S.pre, S.tsum, w.tregion, LC::cls, S.tbase);
    if (E && !loaded) {  // E is workgroup-uniform (read from LDS after a barrier)
      load();
      loaded = true;
      __syncthreads();
    }
    // The first Es entries are walked in S.perm's order, the rest in list order after them: a
    // dense chunk a little over SORTCAP keeps its order for all but the tail.  Unsorted (Es = 0)
    // is the <= 8 B pass, by default: its exact order removes 13 % of the pass's VALU instructions
    // on C4 (the model: lane use in merge_lds8_run 0.77 -> 0.96) but none of its time -- its waves
    // wait more instead -- and costs the sort: k_bpe_short 3.41 -> 3.43 ms
    // (profiles/chunk_sort/ab_summary.txt).
    uint32_t Es = 0;
    if constexpr (N > 32) {
      // 33..64 B: four buckets of width 8 by the two-read sort, all or nothing (untouched: no
      // English-like corpus has such a pass to measure it on)
      if (E <= SORTCAP) {
        Es = uni(E);
        auto bucket = [&](uint32_t n) { return csort::bucket(N, false, n); };
        if (tid < 4) { S.bcnt[tid] = 0; S.bfill[tid] = 0; }
        __syncthreads();
        for (uint32_t q = tid; q < E; q += NT) {  // bucket sizes (one LDS add per wave and bucket)
          const uint32_t kt = tile_of<K>(S.pre, q);
          const uint32_t b = bucket(ent_len(list[(size_t)(c0 + kt) * cap + (q - S.pre[kt])]));
#pragma unroll
          for (uint32_t bb = 0; bb < 4; bb++) {
            const uint64_t m = __ballot(b == bb);
            if (m && (threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1) atomicAdd(&S.bcnt[bb], (uint32_t)__popcll(m));
          }
        }
        __syncthreads();
        if (tid == 0) {
          uint32_t acc = 0;
          for (int bb = 0; bb < 4; bb++) {
            const uint32_t c = S.bcnt[bb];
            S.bfill[bb] = acc;
            acc += c;
          }
        }
        __syncthreads();
        for (uint32_t q = tid; q < E; q += NT) {  // scatter entry numbers into bucket order
          const uint32_t kt = tile_of<K>(S.pre, q);
          const uint32_t b = bucket(ent_len(list[(size_t)(c0 + kt) * cap + (q - S.pre[kt])]));
#pragma unroll
          for (uint32_t bb = 0; bb < 4; bb++) {
            const uint32_t slot = wave_append(&S.bfill[bb], b == bb);
            if (b == bb) S.perm[slot] = (uint16_t)q;
          }
        }
        __syncthreads();
      }
    } else if (csort::sorts(N, mode)) {
      Es = uni(min(E, SORTCAP));  // (a scalar, as E is workgroup-uniform: it lives through the piece loop)
      chunk_sort<N, K, NT, SORTCAP>(S, list, c0, cap, Es, mode);
    }
    auto entry = [&](uint32_t i, uint32_t& kt) {
      const uint32_t q = i < Es ? (uint32_t)S.perm[i] : i;
      kt = tile_of<K>(S.pre, q);
      return list[(size_t)(c0 + kt) * cap + (q - S.pre[kt])];
    };
    auto start_of = [&](uint32_t e, uint32_t kt) { return (c0 + kt) * kTile + (e & 0xFFFu); };
    // one piece: list entry e of chunk tile kt, its first N bytes in wv
    // `hook` runs before the piece's first store (the pipeline below waits there for its
    // look-ahead loads, not behind the stores at its next step)
    auto body = [&](uint32_t e, uint32_t kt, const uint32_t* wv, auto&& hook) {
        const uint32_t tile = c0 + kt;
        const uint32_t s = tile * kTile + (e & 0xFFFu);
        const uint32_t o = ent_ord(e);
        const uint32_t n = ent_len(e);
        // ids go to the next free slots of the tile's region for this class (dense: a wave's
        // stores fill whole lines), the record points at them
        uint32_t pos = 0;
        auto out_of = [&](uint32_t mm) {
          pos = atomicAdd(&S.tsum[kt], mm);
          return w.scratch + (size_t)tile * kTileSlots + pos;
        };
        auto record = [&](uint32_t m) {
          CTOK_CHECK_REC(m >= 1 && m <= n && pos + m <= (uint32_t)kTileSlots && o < (uint32_t)kTileSlots,
                         "[ctok check] class pass N=%d PK=%d tile %u: record m=%u n=%u pos=%u ordinal=%u\n", N, (int)PK,
                         tile, m, n, pos, o);
          w.mrec[(size_t)tile * kTileSlots + o] = rec_short(m, pos);
          st_bytes += n;
          st_ids += m;
        };
        if constexpr (PK) {
          static_assert((N == 16 || N == 32) && L8 && COMPACT,
                        "the packed tiers are the 9..16 B and 17..32 B passes', ahead of merge_lds8, on compact tables");
          // packed tokens straight from the byte -> id table, packed values from the byte-pair
          // table (no entry of it panics and every value fits 16 bits: Tables::short_packed;
          // kNoRank's low half is mpk::kNone)
          constexpr int ND = N / 2;
          uint32_t T[ND], R[ND], bytes[N];
          bool missing = false;
#pragma unroll
          for (int k = 0; k < N; k++) bytes[k] = byte_of(wv[k >> 2], k);
#pragma unroll
          for (int d = 0; d < ND; d++) {
            const int32_t i0 = s_b2id[bytes[2 * d]], i1 = s_b2id[bytes[2 * d + 1]];
            missing |= (((uint32_t)(2 * d) < n) & (i0 < 0)) | (((uint32_t)(2 * d + 1) < n) & (i1 < 0));
            T[d] = mpk::pack2((uint32_t)i0, (uint32_t)i1);
          }
          if (missing) {  // a byte char absent from the vocab is dropped: generic path
            hook();
            defer_to_generic(w, s, o, n);
            return;
          }
          {
            uint32_t v[N];
#pragma unroll
            for (int k = 0; k < N - 1; k++) v[k] = t.pair0[(bytes[k] << 8) | bytes[k + 1]];
            v[N - 1] = kNoRank;
#pragma unroll
            for (int k = 0; k < N - 1; k++) v[k] = (uint32_t)k + 1 < n ? v[k] : kNoRank;
#pragma unroll
            for (int d = 0; d < ND; d++) R[d] = mpk::pack2(v[2 * d], v[2 * d + 1]);
          }
          uint32_t m = n;
          Lookup16<HOT> lk{t, P, err};
          if constexpr (N == 32) {
            // 32 slots down to <= 16 tokens, then the 16-slot tier on the low 8 + 8 dwords
            bool more = mpk::tier(T, R, m, 16u, lk);
            uint32_t T8[8], R8[8];
            mpk::low_half(T, T8);
            mpk::low_half(R, R8);
            if (more) more = mpk::tier(T8, R8, m, 8u, lk);
            hook();
            if (more) {
              lds8_store_packed<0, 8, NT>(T8, R8, s_key, s_tok);
              m = merge_lds8_run<COMPACT, HOT, NT>(t, P, m, s_key, s_tok, err, out_of);
            } else if (m > 16) {
              store_packed_ids<0, N>(T, m, out_of(m));
            } else {
              store_packed_ids<0, 16>(T8, m, out_of(m));
            }
          } else {
            const bool more = mpk::tier(T, R, m, 8u, lk);
            hook();
            if (more) {
              lds8_store_packed<0, 8, NT>(T, R, s_key, s_tok);
              m = merge_lds8_run<COMPACT, HOT, NT>(t, P, m, s_key, s_tok, err, out_of);
            } else {
              store_packed_ids<0, N>(T, m, out_of(m));
            }
          }
          record(m);
          return;
        }
        uint32_t tk[N], rk[N];
        bool missing = false;
        {
#pragma unroll
          for (int k = 0; k < N; k++) {
            const int32_t id = s_b2id[byte_of(wv[k >> 2], k)];
            missing |= ((uint32_t)k < n) & (id < 0);
            tk[k] = (uint32_t)id;
          }
        }
        if (missing) {  // a byte char absent from the vocab is dropped: generic path
          hook();
          defer_to_generic(w, s, o, n);
          return;
        }
        // initial pair ranks: every initial pair is a byte pair, one load each from the 256 x 256
        // byte-pair table (L2-resident), all in flight together
        {
          uint32_t bytes[N];
#pragma unroll
          for (int k = 0; k < N; k++) bytes[k] = byte_of(wv[k >> 2], k);
#pragma unroll
          for (int k = 0; k < N - 1; k++) rk[k] = t.pair0[(bytes[k] << 8) | bytes[k + 1]];
#pragma unroll
          for (int k = 0; k < N - 1; k++) {
            const bool live = (uint32_t)k + 1 < n;
            if (live && rk[k] != kNoRank && value_panics(t, rk[k])) atomicOr(err, kErrPanic);
            rk[k] = (live && !(rk[k] != kNoRank && value_panics(t, rk[k]))) ? rk[k] : kNoRank;
          }
        }
        rk[N - 1] = kNoRank;
        uint32_t m = n;
        // tiers: N slots while the piece has more than N/2 tokens, then N/2, ... down to 8 slots
        bool more = true;
        if constexpr (N >= 64) more = merge_slots<64, COMPACT, HOT, L8>(t, P, tk, rk, m, 32, err);
        if constexpr (N >= 32) {
          if (more) more = merge_slots<32, COMPACT, HOT, L8>(t, P, tk, rk, m, 16, err);
        }
        if constexpr (N >= 16) {
          if (more) more = merge_slots<16, COMPACT, HOT, L8>(t, P, tk, rk, m, 8, err);
        }
        hook();
        if (L8 && more) {
          m = merge_lds8<COMPACT, HOT, NT>(t, P, tk, rk, m, s_key, s_tok, err, out_of);
        } else {
          if (!L8 && more) merge_slots<8, COMPACT, HOT, L8>(t, P, tk, rk, m, 0, err);
          uint32_t* out = out_of(m);
#pragma unroll
          for (int k = 0; k < N; k++)
            if ((uint32_t)k < m) out[k] = tk[k];
        }
        record(m);
    };
    if constexpr (N > 32) {
      // 64 slots: no registers to spare for a pipeline; a static stride over the chunk
      for (uint32_t i = tid; i < E; i += NT) {
        uint32_t kt;
        const uint32_t e = entry(i, kt);
        uint32_t wv[N / 4];
        load_words<N / 4>(w.text, start_of(e, kt), w.n_bytes, wv);
        body(e, kt, wv, [] {});
      }
    } else {
      // Each wavefront takes blocks of 64 entries from S.next (one LDS atomic per block): a wave
      // whose pieces merge quickly takes more blocks, so the chunk's waves finish together
      // instead of each owning a fixed stride of the chunk (which cost 8% (<= 8 B) .. 15%
      // (9..16 B) of the pass at the chunk barrier).  Software pipeline over a wave's blocks b0,
      // b1, b2: the list entry is loaded two blocks ahead and the piece's text dwords one block
      // ahead, so the merges of one piece hide the two dependent global loads of the next.  The
      // look-ahead registers are only loaded here (aligned at their use) and are waited for
      // inside the piece's body before its stores (`hook`): vmcnt counts loads and stores
      // together in issue order, so a wait for them at the top of the next step would also wait
      // for the stores.
      const uint32_t lane = tid & 63;
      auto take = [&]() -> uint32_t {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(&S.next, 64u);
        return uni((uint32_t)__shfl((int)b, 0, 64));
      };
      constexpr int kPw = N / 4;
      uint32_t e0 = 0, kt0 = 0, e1 = 0, kt1 = 0;
      uint32_t d0[kPw + 1], sh0 = 0;  // the next piece's text dwords (unaligned) and its byte shift
#pragma unroll
      for (int k = 0; k <= kPw; k++) d0[k] = 0;
      const uint32_t last = (w.n_bytes - 1) & ~3u;
      auto issue_words = [&](uint32_t s) {
        const uint32_t a0 = s & ~3u;
#pragma unroll
        for (int k = 0; k <= kPw; k++) d0[k] = *reinterpret_cast<const uint32_t*>(w.text + min(a0 + 4 * k, last));
        sh0 = s & 3u;
      };
      auto hook = [&]() {
        static_assert(kPw <= 8, "hook operands");
        if constexpr (!LA) asm volatile("" ::"v"(e1));
        else if constexpr (kPw == 2) asm volatile("" ::"v"(d0[0]), "v"(d0[1]), "v"(d0[2]), "v"(e1));
        else if constexpr (kPw == 4)
          asm volatile("" ::"v"(d0[0]), "v"(d0[1]), "v"(d0[2]), "v"(d0[3]), "v"(d0[4]), "v"(e1));
        else
          asm volatile("" ::"v"(d0[0]), "v"(d0[1]), "v"(d0[2]), "v"(d0[3]), "v"(d0[4]), "v"(d0[5]), "v"(d0[6]),
                       "v"(d0[7]), "v"(d0[8]), "v"(e1));
      };
      uint32_t b0 = take();
      uint32_t b1 = b0 < E ? take() : E;
      if constexpr (LA) {
        if (b0 + lane < E) {
          e0 = entry(b0 + lane, kt0);
          issue_words(start_of(e0, kt0));
        }
        if (b1 + lane < E) e1 = entry(b1 + lane, kt1);
        hook();
        while (b0 < E) {  // wave-uniform
          const uint32_t i = b0 + lane;
          const uint32_t b2 = b1 < E ? take() : E;
          const uint32_t e = e0, kt = kt0;
          uint32_t wv[kPw];
#pragma unroll
          for (int k = 0; k < kPw; k++) wv[k] = __builtin_amdgcn_alignbyte(d0[k + 1], d0[k], sh0);
          e0 = e1;
          kt0 = kt1;
          if (b1 + lane < E) issue_words(start_of(e0, kt0));
          if (b2 + lane < E) e1 = entry(b2 + lane, kt1);
          b0 = b1;
          b1 = b2;
          if (i < E) body(e, kt, wv, hook);
          else hook();
        }
      } else {
        // one stage: the list entry one block ahead (e1), the piece's own text loaded at its turn
        if (b0 + lane < E) e1 = entry(b0 + lane, kt1);
        while (b0 < E) {  // wave-uniform
          const uint32_t i = b0 + lane;
          const uint32_t b2 = b1 < E ? take() : E;
          const bool live = i < E;
          const uint32_t e = live ? e1 : 0u, kt = live ? kt1 : 0u;  // (idle lanes read the chunk's first bytes)
          uint32_t wv[kPw];
          load_words<kPw>(w.text, start_of(e, kt), w.n_bytes, wv);
          if (b1 + lane < E) e1 = entry(b1 + lane, kt1);
          b0 = b1;
          b1 = b2;
          if (live) body(e, kt, wv, hook);
          else hook();
        }
      }
    }
    tile_share_flush<K>(w, c0, tb1, S.tsum, S.tbase, LC::cls);
    // size the next chunk for about two entries per thread (up to K tiles): sparse classes take
    // several units at once, dense ones one; never more than a fair share of the units left, so
    // the last chunks stay small (C2: 504 units for 256 workgroups)
    const uint32_t units = (w.n_tiles + U - 1) / U, next = S.chunk + S.take;
    const uint32_t share = next < units ? (units - next) / gridDim.x : 0u;
    take = min(min((uint32_t)K / U, max(1u, share)), N <= 16 ? 64u : max(1u, (2 * NT * S.take + E) / (E + 1)));
    __syncthreads();
  }
  // statistics: bytes merged and ids produced by this pass (algorithmic bytes for the roofline)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    st_bytes += (uint32_t)__shfl_xor((int)st_bytes, o, 64);
    st_ids += (uint32_t)__shfl_xor((int)st_ids, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicAdd(&S.stat[0], st_bytes);
    atomicAdd(&S.stat[1], st_ids);
  }
  __syncthreads();
  if (tid == 0) {
    atomicAdd(&w.counters[ctr_stat(LC::cls)], S.stat[0]);
    atomicAdd(&w.counters[ctr_stat(LC::cls) + 1], S.stat[1]);
  }
  __syncthreads();
}

// (Round 5 also built a lane-group variant of this pass -- 8 / 16 lanes per piece, -DCTOK_SHORT_LG:
// 4.3x slower, VALU-issue bound; DESIGN.md 4.2.  It is kept out of this file as
// profiles/r05/patches/short_lane_group.diff.)

// Pieces of <= 16 bytes (classes 0 and 1): one workgroup per CU holding the whole LDS image
// (hot table + Bloom filter); a workgroup moves on to class 1 as soon as class 0 has no chunk
// left, with no kernel boundary in between.  NARROW (every id < 2^16): 1024 threads, the last
// tier's state in LDS (merge_lds8); else 1024 threads, all tiers in registers.
// Narrow: the workgroup size and the sort buffer share the LDS left beside the image with
// merge_lds8's 48 B per thread; 1024 threads with a 7168-entry sort buffer (LDS 163,648 B) take
// k_bpe_short 3.57 -> 3.51 ms on C4 against 960 with 8192 (profiles/r04/v12_ab_short_nt1024_c4.txt).
// (Compile-time knobs for A/B builds.)
#ifndef CTOK_SHORT_NT
#define CTOK_SHORT_NT 1024
#endif
#ifndef CTOK_SHORT_SORTCAP
#define CTOK_SHORT_SORTCAP 7168
#endif
template <bool NARROW> struct ShortCfg {
  static constexpr uint32_t NT = NARROW ? CTOK_SHORT_NT : 1024;
  static constexpr uint32_t SORTCAP = NARROW ? CTOK_SHORT_SORTCAP : kSortCap;
};
// tiles per chunk of the <= 16 B passes (dense classes: ~100 + ~60 pieces per tile on C4; 128
// tiles per chunk measured 3% slower, profiles/r02/v30_ab_short_kt128.txt)
constexpr int kShortKT = 64;

// PK16 (narrow compact tables with Tables::short_packed): the 9..16 B pass's 16-slot tier on u16 pairs.
// PK32 (Tables::mid_packed == 2): the instance can also take the 17..32 B class as a third pass
// on the packed 32-slot tier (passes bit 2), in the same workgroups with the image, the byte -> id
// table and merge_lds8's state already in LDS.  It does so when the call has no long piece -- the
// situation in which the host would otherwise put k_bpe_mid<2> on the idle side stream -- and it
// reads that from the long-piece counter, final since k_segment completed; the host reads the same
// counter in the report and launches k_bpe_mid<2> only when this kernel left the class alone
// (mid_folded).  The class is sparse, so the pass takes k_bpe_mid's chunks of up to kMidKT tiles:
// the shared scratch grows by 2.3 KB, taken from the sort buffer (kFoldSortCut entries of u16).
constexpr int kMidKT = 256;
constexpr uint32_t kFoldSortCut = 3 * (kMidKT - kShortKT) * 4 / 2;
template <bool COMPACT, bool NARROW, bool PK16 = false, bool PK32 = false>
__global__ __launch_bounds__(1024) void k_bpe_short(Work w, Tables t, uint32_t passes) {
  static_assert((NARROW && COMPACT) || !PK16, "the packed tier needs the narrow tables and compact values");
  static_assert(PK16 || !PK32, "the third pass is the packed instance's");
  if (w.report && blockIdx.x == 0 && threadIdx.x < 64) write_report(w);  // (k_report's work: see emit.hip)
  if (spec_failed(w)) return;
  constexpr uint32_t NT = ShortCfg<NARROW>::NT;
  constexpr uint32_t SORTCAP = ShortCfg<NARROW>::SORTCAP - (PK32 ? kFoldSortCut : 0u);
  extern __shared__ __attribute__((aligned(16))) uint4 s_img[];
  __shared__ int32_t s_b2id[256];
  __shared__ PassLds<SORTCAP, PK32 ? kMidKT : kShortKT> S;
  __shared__ uint32_t s_key[NARROW ? 8 * NT : 1];
  __shared__ uint16_t s_tok[NARROW ? 8 * NT : 1];
  const uint32_t tid = threadIdx.x;
  const uint4* img = NARROW ? t.lds16_image : t.lds_image;
  auto load = [&] {
    for (uint32_t i = tid; i < kLdsImageBytes / 16; i += NT) s_img[i] = img[i];
    for (uint32_t i = tid; i < 256; i += NT) s_b2id[i] = t.byte2id[i];
  };
  bool loaded = false;
  const PairLds P{(const lds_u64*)s_img, (const lds_u32*)(s_img + kHotBuckets)};
  lds_u32* sk = (lds_u32*)s_key;
  lds_u16* st = (lds_u16*)s_tok;
  WgRec::begin(w.wgrec, 0);
  // passes: bit 0 the <= 8 B class, bit 1 the 9..16 B class (both, except in the timing A/B
  // CTOK_DBG_MODE=30, which launches them as two kernels to time them apart)
  if (passes & 1u)
    class_pass<8, COMPACT, true, NT, SORTCAP, NARROW, kShortKT>(w, t, P, s_b2id, S, loaded, load, sk, st);
  if (passes & 2u)
    class_pass<16, COMPACT, true, NT, SORTCAP, NARROW, kShortKT, PK16>(w, t, P, s_b2id, S, loaded, load, sk, st);
  if constexpr (PK32) {
    if (passes & 4u) {  // (kernel argument: uniform)
      // one read for the workgroup, handed round through LDS: every thread takes the same branch,
      // so all 1024 reach class_pass's barriers or none does.  (S.next is free here: the passes
      // above end with a barrier, and class_pass writes it only after its first one.)
      if (tid == 0) S.next = (mid_folded(t, w.counters[kCtrLong]) && w.counters[kCtrAnyMid] != 0) ? 1u : 0u;
      __syncthreads();
      const uint32_t fold = S.next;
      if (fold)
        class_pass<32, COMPACT, true, NT, SORTCAP, NARROW, kMidKT, true, false>(w, t, P, s_b2id, S, loaded, load, sk, st);
    }
  }
  WgRec::end(w.wgrec, 0, loaded ? 1u : 0u);
}

// ------------------------------------------------------------------------------------------
// Sparse 33..64 B class (round 6).  On English-like text class 3 is a few pieces per thousand
// tiles (C4: ~600 pieces in 322k tiles; C2 or a 1/8 C4 shard: ~70), and the register pass
// (k_bpe_mid<3>: a thread per piece over 64 slots, ~1,300 VALU per merge) then costs one thread's
// whole merge chain: 90 us on C2, 190 us on C4 for a few kilobytes.  k_segment queues each tile's
// class-3 pieces in one of 64 shards (Work::c3q; a shard per tile % 64, so its atomics spread
// over 64 counters); when the report counts at most Work::c3_max of them, the host launches
// k_bpe_sparse instead of the register pass: its waves take the queue's pieces one at a time from
// a counter and merge each on the whole wavefront (merge_wave64), its ids into the tile's class-3
// region (reserved from rend, as the dropped-byte pass does) and its merged record in mrec --
// what the register pass would write.  (Round 6's first build gathered the list in a kernel of
// its own, on a stream forked after k_segment; k_segment appending to one list -- one atomic per
// tile on one counter -- took C5's k_segment from 1.7 to 5.9 ms; folding the pass into the 17..32
// B pass's workgroups put its merge chains at that pass's end, +20..40 us on a 1/8 C4 shard; waves
// scanning 64-tile chunks of the class counts themselves left a dense chunk's pieces to one wave:
// C5-NFC's sub-batch 2.4 -> 17 ms.)

// The merge loop of one <= 64-token piece on a whole wavefront: lane k holds token k (positions
// stay put) and the value of the pair its token starts (kNoRank when it starts none); the live
// mask lv (wave-uniform, in SGPRs) marks the lanes that still hold a token.  A merge is a 64-lane
// minimum of value << 6 | lane (the lowest value, leftmost on ties: src/bpe.rs:118-149, as
// merge_slots), its neighbours found with scalar bit scans of lv, the two new pairs looked up at
// once by lanes 0 and 1, and three selects -- a chain of ~40 instructions and one LDS probe per
// merge where the register pass spends ~1,300 on one lane.  Returns the token count.
template <bool COMPACT, bool NARROW>
__device__ __forceinline__ uint32_t merge_wave64(const Tables& t, const PairLds& P, uint32_t& tok, uint32_t rk,
                                                 uint64_t& lv, uint32_t* err) {
  const uint32_t lane = threadIdx.x & 63;
  for (;;) {
    const uint32_t best = wave_min_full_u32((rk << 6) | lane);
    const uint32_t r = best >> 6, bi = best & 63u;
    if (r == kNoRank) break;
    const uint32_t nid = COMPACT ? r : uni(t.rank_newid[r]);
    const uint64_t right = lv & ~((2ull << bi) - 1ull);  // live lanes past bi (bi < 63: it starts a pair)
    const uint32_t p = (uint32_t)__builtin_ctzll(right);  // the right token
    const uint64_t after = right & (right - 1ull);
    const bool has_r = after != 0;
    const uint32_t q = has_r ? (uint32_t)__builtin_ctzll(after) : 0u;  // the token after it
    const uint64_t left = lv & ((1ull << bi) - 1ull);
    const bool has_l = left != 0;
    const uint32_t pv = has_l ? 63u - (uint32_t)__builtin_clzll(left) : 0u;  // the token before
    const uint32_t L = __builtin_amdgcn_readlane(tok, pv), R = __builtin_amdgcn_readlane(tok, q);
    uint32_t v = kNoRank;
    if (lane < 2) {  // lane 0: (L, nid), lane 1: (nid, R)
      Probe<NARROW, true> pr;
      pr.start(t, P, lane == 0 ? L : nid, lane == 0 ? nid : R, lane == 0 ? has_l : has_r);
      v = pr.finish(t, err);
    }
    const uint32_t rl = __builtin_amdgcn_readlane(v, 0), rr = __builtin_amdgcn_readlane(v, 1);
    tok = lane == bi ? nid : tok;
    rk = (has_l && lane == pv) ? rl : rk;
    rk = lane == bi ? (has_r ? rr : kNoRank) : rk;
    rk = lane == p ? kNoRank : rk;
    lv &= ~(1ull << p);
  }
  return (uint32_t)__popcll(lv);
}

// One wave's share of the sparse class-3 pass (see above): n pieces in the sharded queue c3q
// (shard i: pieces c3pre[i] .. c3pre[i + 1] - 1 of the pass, at c3q + i * cap); P / s_b2id: the
// workgroup's LDS image.
template <bool COMPACT, bool NARROW>
__device__ __forceinline__ void sparse_c3(const Work& w, const Tables& t, const PairLds& P, const int32_t* s_b2id,
                                          uint32_t n) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t cap = w.c3_max / kC3Shards;
  const uint32_t pre = w.c3pre[lane];  // (kC3Shards == 64: shard `lane`'s first piece)
  uint32_t* err = &w.counters[kCtrErr];
  uint32_t st_bytes = 0, st_ids = 0;
  for (;;) {
    // (every lane takes part, lane 0 adding 1: no divergent branch around the atomic)
    const uint32_t k = uni(atomicAdd(&w.counters[kCtrC3Take], lane == 0 ? 1u : 0u));
    if (k >= n) break;
    // its shard: the last one starting at or before k (empty shards share their successor's start)
    const uint32_t sh = 63u - (uint32_t)__builtin_clzll(__ballot(pre <= k));
    const uint32_t qe = uni(w.c3q[(size_t)sh * cap + (k - __builtin_amdgcn_readlane(pre, sh))]);
    const uint32_t tile = qe >> 7;
    const uint32_t e = uni(w.list3[(size_t)tile * kCap3 + (qe & 127u)]);
    const uint32_t s = tile * kTile + (e & 0xFFFu), o = ent_ord(e), len = ent_len(e);
    // lane k: byte k, its token, the value of the byte pair it starts (the 256 x 256 table)
    const uint32_t b0 = lane < len ? w.text[s + lane] : 0u;
    const uint32_t b1 = lane + 1 < len ? w.text[s + lane + 1] : 0u;
    const int32_t id = s_b2id[b0];
    if (__ballot(lane < len && id < 0)) {  // a byte char absent from the vocab: the generic pass drops it
      if (lane == 0) defer_to_generic(w, s, o, len);
      continue;
    }
    uint32_t rk = lane + 1 < len ? t.pair0[(b0 << 8) | b1] : kNoRank;
    if (rk != kNoRank && value_panics(t, rk)) {
      atomicOr(err, kErrPanic);
      rk = kNoRank;
    }
    uint32_t tok = (uint32_t)id;
    uint64_t lv = len >= 64 ? ~0ull : (1ull << len) - 1ull;
    const uint32_t m = merge_wave64<COMPACT, NARROW>(t, P, tok, rk, lv, err);
    uint32_t pos = 0;
    if (lane == 0) pos = atomicAdd(&w.rend[3ull * w.n_tiles + tile], m);
    pos = uni(pos);
    if ((lv >> lane) & 1u) w.scratch[(size_t)tile * kTileSlots + pos + __popcll(lv & lanemask_lt())] = tok;
    CTOK_CHECK_REC(m >= 1 && m <= len && pos + m <= (uint32_t)kTileSlots,
                   "[ctok check] sparse class 3 tile %u: record m=%u n=%u pos=%u\n", tile, m, len, pos);
    if (lane == 0) {
      w.mrec[(size_t)tile * kTileSlots + o] = rec_short(m, pos);
      atomicAdd(&w.tile_tok[tile], m);
    }
    st_bytes += len;
    st_ids += m;
  }
  if (lane == 0 && st_bytes) {  // statistics: bytes merged / ids produced by class 3
    atomicAdd(&w.counters[ctr_stat(3)], st_bytes);
    atomicAdd(&w.counters[ctr_stat(3) + 1], st_ids);
  }
}

constexpr int kSparseWaves = 16;  // waves per k_bpe_sparse workgroup (beside the 96 KiB image: one per CU)

template <bool COMPACT, bool NARROW>
__global__ __launch_bounds__(64 * kSparseWaves) void k_bpe_sparse(Work w, Tables t, uint32_t n) {
  if (spec_failed(w)) return;
  WgRec::begin(w.wgrec, 3);
  extern __shared__ __attribute__((aligned(16))) uint4 s_dyn[];
  __shared__ int32_t s_b2id[256];
  const uint32_t tid = threadIdx.x;
  const uint4* img = NARROW ? t.lds16_image : t.lds_image;
  for (uint32_t i = tid; i < kLdsImageBytes / 16; i += 64 * kSparseWaves) s_dyn[i] = img[i];
  for (uint32_t i = tid; i < 256; i += 64 * kSparseWaves) s_b2id[i] = t.byte2id[i];
  __syncthreads();
  const PairLds P{(const lds_u64*)s_dyn, (const lds_u32*)(s_dyn + kHotBuckets)};
  sparse_c3<COMPACT, NARROW>(w, t, P, s_b2id, n);
  __syncthreads();
  WgRec::end(w.wgrec, 3, 1);
}


// Pieces of 17..32 bytes (CLS = 2, on the main stream after k_bpe_short) or 33..64 bytes (CLS = 3,
// e.g. runs of CJK letters, 3 bytes each): 512-thread workgroups (two waves per SIMD at <= 256
// VGPRs: 32 or 64 register slots per thread) with the whole LDS image.  One class per kernel:
// the fully unrolled 64- and 32-slot loops together overflow the instruction cache.
// Class 3 is launched twice, once on the side stream after the long-piece tiers and once on the
// main stream after class 2; both instances take chunks from the same counter, so a handful of
// class-3 pieces (long merge chains) is done by the side instance in the shadow of the main
// stream's passes, and a large class 3 (multilingual text) is shared by both as CUs free up.
// Most tiles per chunk of the 17..32 B / 33..64 B passes: these classes can be sparse (C4: ~5
// class-2 pieces per tile), where 64 tiles left most of a 512-thread workgroup idle per chunk.
// NT: threads per workgroup.  The 17..32 B pass runs at 768 (three waves per SIMD at 168 VGPRs,
// 152 KiB of LDS) when the call has no long pieces -- on C4 0.60 -> 0.55 ms --, else at 512: with
// long pieces the side stream's tiers share the CUs, and 768 made C5 slower (+0.12 ms,
// profiles/r05/v17_ab_mid768_c4_c5.txt).
template <int CLS> struct MidCfg { static constexpr int KT = kMidKT; };

// PK (CLS = 2, Tables::mid_packed): the 32- and 16-slot tiers on u16 pairs (merge_packed_hd.h).
template <bool COMPACT, int CLS, bool NARROW, uint32_t NT = 512, bool PK = false>
__global__ __launch_bounds__(NT) void k_bpe_mid(Work w, Tables t) {
  static_assert(!PK || (CLS == 2 && NARROW && COMPACT), "the packed tiers need the narrow tables and compact values");
  if (spec_failed(w)) return;
  constexpr int KT = MidCfg<CLS>::KT;
  extern __shared__ __attribute__((aligned(16))) uint4 s_img[];
  __shared__ int32_t s_b2id[256];
  __shared__ PassLds<kSortCap, KT> S;
  __shared__ uint32_t s_key[NARROW ? 8 * NT : 1];
  __shared__ uint16_t s_tok[NARROW ? 8 * NT : 1];
  // (the image is loaded up front: a lazy load pushes the 64-slot pass into scratch; the kernel
  // returns at once when k_segment found no piece of its class)
  if constexpr (CLS == 2) WgRec::begin(w.wgrec, 1);  // (not in the 64-slot pass: it is at its register limit)
  if (w.counters[CLS == 2 ? kCtrAnyMid : kCtrAnyC3] == 0) {
    if constexpr (CLS == 2) WgRec::end(w.wgrec, 1, 0);
    return;
  }
  // every chunk already taken (the other instance of class 3 got there first): one read for the
  // whole workgroup, so its waves leave together (a wave that stayed would find thread 0 gone)
  __shared__ uint32_t s_left;
  if (threadIdx.x == 0)
    s_left = (uint64_t)__atomic_load_n(&w.counters[ctr_chunk(CLS)], __ATOMIC_RELAXED) * w.unit < w.n_tiles;
  __syncthreads();
  if (!s_left) {
    if constexpr (CLS == 2) WgRec::end(w.wgrec, 1, 0);
    return;
  }
  const uint32_t tid = threadIdx.x;
  const uint4* img = NARROW ? t.lds16_image : t.lds_image;
  for (uint32_t i = tid; i < kLdsImageBytes / 16; i += NT) s_img[i] = img[i];
  for (uint32_t i = tid; i < 256; i += NT) s_b2id[i] = t.byte2id[i];
  bool loaded = true;
  const PairLds P{(const lds_u64*)s_img, (const lds_u32*)(s_img + kHotBuckets)};
  class_pass<CLS == 2 ? 32 : 64, COMPACT, true, NT, kSortCap, NARROW, KT, PK>(w, t, P, s_b2id, S, loaded, [] {},
                                                                             (lds_u32*)s_key, (lds_u16*)s_tok);
  if constexpr (CLS == 2) WgRec::end(w.wgrec, 1, 1);
}

template <bool C, int CLS, bool NW, bool PK = false>
static hipError_t launch_mid_t(const Work& w, const Tables& t, hipStream_t s, const Lx& x) {
  static LdsAttr attr;
  HIPCHK(lds_attr_once(attr, (const void*)k_bpe_mid<C, CLS, NW, 512, PK>, kLdsImageBytes));
  if (!w.n_tiles) return hipSuccess;
  const uint32_t grid = min((w.n_tiles + w.unit - 1) / w.unit, w.n_cus);
  if constexpr (CLS == 2) {
    if (w.mid_wide) {
      static LdsAttr attr768;
      HIPCHK(lds_attr_once(attr768, (const void*)k_bpe_mid<C, CLS, NW, 768, PK>, kLdsImageBytes));
      launch_lx(x, k_bpe_mid<C, CLS, NW, 768, PK>, grid, 768, kLdsImageBytes, s, w, t);
      return hipGetLastError();
    }
  }
  launch_lx(x, k_bpe_mid<C, CLS, NW, 512, PK>, grid, 512, kLdsImageBytes, s, w, t);
  return hipGetLastError();
}
template <bool C, int CLS>
static hipError_t launch_mid(const Work& w, const Tables& t, hipStream_t s, const Lx& x = {}) {
  if constexpr (C && CLS == 2) {
    if (t.narrow && t.mid_packed) return launch_mid_t<true, 2, true, true>(w, t, s, x);
  }
  return t.narrow ? launch_mid_t<C, CLS, true>(w, t, s, x) : launch_mid_t<C, CLS, false>(w, t, s, x);
}

template <bool C, bool NW, bool PK = false, bool PK32 = false>
static hipError_t launch_short_t(const Work& w, const Tables& t, hipStream_t s, const Lx& x) {
  static LdsAttr attr;
  HIPCHK(lds_attr_once(attr, (const void*)k_bpe_short<C, NW, PK, PK32>, kLdsImageBytes));
  if (!w.n_tiles) return hipSuccess;
  // (Work::short_wgs: fewer workgroups than CUs leave CUs to the side stream's passes from the start)
  const uint32_t grid = min((w.n_tiles + w.unit - 1) / w.unit, w.short_wgs ? min(w.short_wgs, w.n_cus) : w.n_cus);
  if (t.dbg == 30) {  // a launch per pass: the first records x.start, the last x.stop
    const uint32_t last = PK32 ? 4u : 2u;
    for (uint32_t pass = 1u; pass <= last; pass <<= 1)
      launch_lx(Lx{pass == 1u ? x.start : nullptr, pass == last ? x.stop : nullptr}, k_bpe_short<C, NW, PK, PK32>, grid,
                ShortCfg<NW>::NT, kLdsImageBytes, s, w, t, pass);
  } else {
    launch_lx(x, k_bpe_short<C, NW, PK, PK32>, grid, ShortCfg<NW>::NT, kLdsImageBytes, s, w, t, PK32 ? 7u : 3u);
  }
  return hipGetLastError();
}
template <bool C>
static hipError_t launch_short(const Work& w, const Tables& t, hipStream_t s, const Lx& x) {
  if constexpr (C) {
    if (t.narrow && t.short_packed && t.mid_packed == 2) return launch_short_t<true, true, true, true>(w, t, s, x);
    if (t.narrow && t.short_packed) return launch_short_t<true, true, true>(w, t, s, x);
  }
  return t.narrow ? launch_short_t<C, true>(w, t, s, x) : launch_short_t<C, false>(w, t, s, x);
}

template <bool C, bool NW>
static hipError_t launch_sparse_t(const Work& w, const Tables& t, uint32_t n_pieces, hipStream_t s, const Lx& x) {
  static LdsAttr attr;
  HIPCHK(lds_attr_once(attr, (const void*)k_bpe_sparse<C, NW>, kLdsImageBytes));
  const uint32_t grid = std::max(1u, std::min((n_pieces + kSparseWaves - 1) / kSparseWaves, w.n_cus));  // (a wave per piece at most)
  launch_lx(x, k_bpe_sparse<C, NW>, grid, 64 * kSparseWaves, kLdsImageBytes, s, w, t, n_pieces);
  return hipGetLastError();
}

hipError_t launch_c3_sparse(const Work& w, const Tables& t, uint32_t n_pieces, hipStream_t s, Lx x) {
  if (!n_pieces || n_pieces > w.c3_max || !w.n_tiles) return hipSuccess;
  if (t.compact)
    return t.narrow ? launch_sparse_t<true, true>(w, t, n_pieces, s, x) : launch_sparse_t<true, false>(w, t, n_pieces, s, x);
  return t.narrow ? launch_sparse_t<false, true>(w, t, n_pieces, s, x) : launch_sparse_t<false, false>(w, t, n_pieces, s, x);
}

hipError_t launch_bpe_class(const Work& w, const Tables& t, int cls, hipStream_t s, Lx x) {
  if (t.n_at != 0) {  // every <= 32 B piece is in list0
    if (cls == 0 && w.n_tiles)
      launch_lx(x, k_bpe_generic<false>, (w.n_tiles + kTilesGeneric - 1) / kTilesGeneric, 256, 0, s, w, t);
    return hipGetLastError();
  }
  switch (cls) {
    case 0: return t.compact ? launch_short<true>(w, t, s, x) : launch_short<false>(w, t, s, x);  // classes 0 and 1
    case 2: return t.compact ? launch_mid<true, 2>(w, t, s, x) : launch_mid<false, 2>(w, t, s, x);
    case 4: return t.compact ? launch_mid<true, 3>(w, t, s, x) : launch_mid<false, 3>(w, t, s, x);  // main-stream instance
    case 3:  // pieces with dropped bytes, found by the merge passes (none when every byte's char is in the vocab)
      if (t.all_bytes) return hipSuccess;
      launch_lx(x, k_bpe_generic<true>, 64, 128, 0, s, w, t);
      return hipGetLastError();
    default:
      return hipSuccess;
  }
}

}  // namespace ctok_dev
