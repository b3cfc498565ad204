// Encode path, stage 4: the report and emission -- k_report, k_emit, k_tokoff, and the output
// helpers of the host-buffer pipeline k_shift_u64, k_wire16 (DESIGN.md sections 4.2b and 4.5).
#include "dev_common.h"

namespace ctok_dev {

// The call's report (Work::report): k_segment's counters, the class-3 count among them, into
// pinned host words, then the call's sequence number (write_report).  k_bpe_short's first wave
// writes it as that kernel starts (its packet waited for k_segment); this one-wave kernel does it
// when k_bpe_short does not run (added tokens, no tiles).  The host polls the word instead of
// copying the counters on a second stream forked by an event after k_segment; having seen it, it
// knows k_segment has completed, so what it launches next -- on any stream -- needs no fork event.
__global__ __launch_bounds__(64) void k_report(Work w) {
  write_report(w);
}

hipError_t launch_report(const Work& w, hipStream_t s) {
  k_report<<<1, 64, 0, s>>>(w);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// emission.  tile_tok is scanned to each tile's first id (tile_doc to its first document); then
// one wavefront per tile walks the tile's piece records in rounds of 256 pieces: lane l takes
// pieces 256 r + 4 l .. + 3 (one 8- or 16-byte prec load and their pdoc bits), a wave scan
// numbers the round's merged pieces (their mrec slots: consecutive, so the mrec loads are dense
// too), a second scan gives each piece's first id within the tile, and the ids are staged in LDS
// and stored as whole lines: a whole-piece hit's id is its record, a merged piece's ids are
// copied from scratch (or lids).  Loads run ahead: the records two rounds ahead, the merged
// records one round ahead.  A doc-start piece writes tok_off directly when no document is empty,
// else leaves its first id within the tile in tcnt for k_tokoff.

constexpr int kEmitWaves = 4;  // tiles per k_emit workgroup
constexpr uint32_t kEmitStage = 1024;  // ids of one round staged in LDS (4 KiB per wave)

// one lane's four piece records of a round (u16 or u32) and their doc-start bits
template <typename RT>
struct EmitRecs {
  using V = typename std::conditional<sizeof(RT) == 2, uint2, uint4>::type;
  V v;
  uint32_t d;
  __device__ uint32_t rec(int k) const {
    if constexpr (sizeof(RT) == 2) {
      const uint32_t x = k < 2 ? v.x : v.y;
      return (k & 1) ? x >> 16 : x & 0xFFFFu;
    } else {
      return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
    }
  }
};

template <typename RT>
__global__ __launch_bounds__(64 * kEmitWaves) void k_emit(Work w, uint32_t* __restrict__ ids, uint64_t ids_cap,
                                                         uint64_t* __restrict__ tok_off) {
  // (a lean list overflowed: some pieces were never listed, so their merged records were never
  // written -- the host runs the call again with the safe capacities, and this pass must not
  // gather through records no pass wrote)
  if (spec_failed(w) || uni(w.counters[kCtrOverflow]) != 0) return;
  constexpr uint32_t kMerged = sizeof(RT) == 2 ? kRecMerged16 : kRecMerged32;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t tile = uni(blockIdx.x * kEmitWaves + (threadIdx.x >> 6));
  if (tile >= w.n_tiles) return;
  const uint32_t np = uni(w.tile_np[tile]);
  const uint64_t base = uni(w.tile_tok[tile]);
  // no empty documents: the n-th doc-start piece of the tile starts document tile_doc[tile] + n,
  // so tok_off is written here (k_tokoff then only writes tok_off[n_docs])
  const bool direct = uni(w.counters[kCtrEmptyDocs]) == 0;
  const RT* prec = (const RT*)w.prec + (size_t)tile * kTileSlots;
  const uint32_t* mrec = w.mrec + (size_t)tile * kTileSlots;
  const uint32_t* pdoc = w.pdoc + (size_t)tile * (kTileSlots / 32);
  uint32_t* tcnt = w.tcnt + (size_t)tile * kTileSlots;
  const uint32_t* src0 = w.scratch + (size_t)tile * kTileSlots;
  using Recs = EmitRecs<RT>;
  // (no arithmetic on the loaded values here: a use right after the load would wait for it)
  auto load = [&](uint32_t j0) {
    Recs x;
    if (j0 < np) {
      x.v = *reinterpret_cast<const typename Recs::V*>(prec + j0);
      x.d = pdoc[j0 >> 5];
    } else {
      x.v = {};
      x.d = 0;
    }
    return x;
  };
  // the doc-start bits of pieces j0 .. j0 + 3 (j0 % 4 == 0: they share a word)
  auto docs = [&](const Recs& x, uint32_t j0) {
    const uint32_t d = (x.d >> (j0 & 31)) & 15u;
    return j0 + 4 > np ? (j0 < np ? d & ((1u << (np - j0)) - 1u) : 0u) : d;
  };
  __shared__ uint32_t s_stage[kEmitWaves][kEmitStage];
  __shared__ uint32_t s_mrec[kEmitWaves][256];
  lds_u32* stage = (lds_u32*)s_stage[threadIdx.x >> 6];
  lds_u32* smr = (lds_u32*)s_mrec[threadIdx.x >> 6];
  // A round's numbering: one scan of (doc starts << 16 | merged pieces) gives this lane's first
  // merged ordinal and first document; the round's merged records (consecutive in mrec) are
  // loaded by the whole wave, 64 per instruction: the first 64 a round ahead of their use, more
  // (rare on English text) when they are used.
  uint32_t mrun = 0, dnext = uni(w.tile_doc[tile]);  // (wave-uniform)
  struct Ahead {
    uint32_t o, d, nm;  // this lane's first ordinal (within the round) and document; the round's merged pieces
    uint32_t m0;        // the round's first merged ordinal (wave-uniform)
    uint32_t q;         // mrec[m0 + lane]
  };
  auto number = [&](const Recs& x, uint32_t j0) {
    Ahead a;
    uint32_t nm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) nm += (j0 + k < np && x.rec(k) == kMerged) ? 1u : 0u;
    const uint32_t nd = (uint32_t)__popc(docs(x, j0));
    const uint32_t v = nm | (nd << 16);
    const uint32_t inc = wave_incl_scan(v);
    const uint32_t tot = uni(lane63(inc));
    a.o = (inc - v) & 0xFFFFu;
    a.d = dnext + ((inc - v) >> 16);
    a.nm = tot & 0xFFFFu;
    dnext = uni(dnext + (tot >> 16));
    a.m0 = mrun;
    a.q = lane < a.nm ? mrec[mrun + lane] : 0u;
    mrun = uni(mrun + a.nm);
    return a;
  };
  uint32_t run = 0;  // ids of the earlier rounds (wave-uniform)
  uint32_t r_first = 0;  // the current round's first id within the tile (wave-uniform)
  // (an empty asm reading loaded registers: the compiler waits for those loads there, not at a
  // later use behind the round's stores)
  auto touch = [](const Recs& x) {
    if constexpr (sizeof(RT) == 2) asm volatile("" ::"v"(x.v.x), "v"(x.v.y), "v"(x.d));
    else asm volatile("" ::"v"(x.v.x), "v"(x.v.y), "v"(x.v.z), "v"(x.v.w), "v"(x.d));
  };
  Recs cur = load(4 * lane);
  Ahead acur = number(cur, 4 * lane);
  Recs nx = load(256 + 4 * lane);
  touch(nx);
  if (acur.nm > 0) smr[lane] = acur.q;  // (the first round's; each round writes the next one's)
  for (uint32_t r0 = 0; r0 < np; r0 += 256) {
    const uint32_t j0 = r0 + 4 * lane;
    // this round's merged records into LDS, each lane's four from there
    // Waits: every load of the round is issued before the first wait (the scratch ids), which
    // then also covers the look-ahead loads; the look-ahead values are consumed before the
    // round's stores, so the next round starts without waiting for those stores (vmcnt counts
    // loads and stores together, in issue order).
    if (acur.nm > 64)  // (the round's merged records past the first 64: loaded now)
      for (uint32_t i = 64 + lane; i < acur.nm; i += 64) smr[i] = mrec[acur.m0 + i];
    if (acur.nm > 0) wave_sync_lds();
    uint32_t mv[4];
    {
      uint32_t o = acur.o;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool m = j0 + k < np && cur.rec(k) == kMerged;
        mv[k] = m ? smr[o] : 0u;
        o += m ? 1u : 0u;
      }
    }
    // the next round's numbering and merged records, the records of the round after it
    Ahead anx{};
    if (r0 + 256 < np) anx = number(nx, j0 + 256);
    const Recs nx2 = load(j0 + 512);
    // id counts and where the ids are; long pieces' from long_cnt / long_pos, in a wave-uniform
    // branch that waits for those loads itself
    uint32_t c[4];
    const uint32_t* sp[4];
    bool lng = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t r = cur.rec(k), v = mv[k];
      const bool merged = j0 + k < np && r == kMerged;
      c[k] = j0 + k >= np ? 0u : !merged ? 1u : (v & 0xFFFFu);
      sp[k] = src0 + (merged ? (v >> 16) & 0xFFFu : 0u);
      lng |= merged && (v & kRecLong);
    }
#ifdef CTOK_CHECK
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t v = mv[k];
      if (j0 + k < np && cur.rec(k) == kMerged) {
        if (v & kRecLong)
          CTOK_CHECK_REC((v & kRecLongMask) < long_count(w), "[ctok check] k_emit tile %u piece %u: long record %08x past %u\n",
                         tile, j0 + k, v, long_count(w));
        else
          CTOK_CHECK_REC((v & 0xFFFFu) <= (uint32_t)kMedMax && ((v >> 16) & 0xFFFu) + (v & 0xFFFFu) <= (uint32_t)kTileSlots,
                         "[ctok check] k_emit tile %u piece %u: merged record %08x out of range\n", tile, j0 + k, v);
      }
    }
#endif
    if (__ballot(lng)) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t v = mv[k];
        if (j0 + k < np && cur.rec(k) == kMerged && (v & kRecLong)) {
          c[k] = w.long_cnt[v & kRecLongMask];
          sp[k] = w.lids + w.long_pos[v & kRecLongMask];
        }
      }
      asm volatile("" ::"v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(sp[0]), "v"(sp[1]), "v"(sp[2]), "v"(sp[3]));
    }
    const uint32_t sum = c[0] + c[1] + c[2] + c[3];
    const uint32_t inc = wave_incl_scan(sum);
    const uint32_t o0 = run + inc - sum;  // this lane's first id within the tile
    run = uni(run + lane63(inc));
    // first ids: all loads of this lane's pieces in flight together
    uint32_t v0[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t r = cur.rec(k);
      v0[k] = r != kMerged ? r : (c[k] != 0 ? sp[k][0] : 0u);
    }
    // the round's ids: staged in LDS when they fit, then written out by the whole wave as 64
    // consecutive dwords per store (whole lines; the lanes' own runs are ~5 ids apart, so direct
    // stores touch a dozen partial lines each); else each lane stores its runs itself
    const uint32_t r_ids = run - r_first;
    const bool staged = r_ids <= kEmitStage;
    if (staged) {
      // first ids into the stage; a merged piece's further ids are copied by the whole wave from a
      // list of (scratch place, count, stage place) descriptors in smr (this round's merged
      // records were read above): one round trip for the round's copies instead of one per piece
      // position k, and the lanes share them evenly (a long piece's ids: its own lane)
      bool sk[4];
      uint32_t nd = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        sk[k] = c[k] > 1 && !(mv[k] & kRecLong);
        nd += sk[k] ? 1u : 0u;
      }
      const uint32_t dinc = wave_incl_scan(nd);
      uint32_t di = dinc - nd;
      const uint32_t n_desc = uni(lane63(dinc));
      uint32_t o = o0 - r_first;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t cj = c[k];
        if (cj > 0) stage[o] = v0[k];
        if (sk[k]) {
          smr[di++] = ((mv[k] >> 16) & 0xFFFu) | (cj << 12) | (o << 19);
        } else if (cj > 1) {
          const uint32_t* spk = sp[k];
          for (uint32_t m = 1; m < cj; m += 4) {
            uint32_t x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = m + i < cj ? spk[m + i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++)
              if (m + i < cj) stage[o + m + i] = x[i];
          }
        }
        o += cj;
      }
      if (n_desc) {
        wave_sync_lds();
        for (uint32_t q = lane; q < n_desc; q += 64) {
          const uint32_t d = smr[q];
          const uint32_t* spk = src0 + (d & 0xFFFu);
          const uint32_t cj = (d >> 12) & 0x7Fu, so = d >> 19;
          for (uint32_t m = 1; m < cj; m += 4) {
            uint32_t x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = m + i < cj ? spk[m + i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++)
              if (m + i < cj) stage[so + m + i] = x[i];
          }
        }
      }
    }
    // the look-ahead values in place before any store: the next round's merged records to LDS
    // (this round's were read above), the records it uses waited for here
    if (anx.nm > 0) smr[lane] = anx.q;
    touch(nx2);
    if (staged) {
      wave_sync_lds();
      const uint64_t d0 = base + r_first;
      for (uint32_t i = lane; i < r_ids; i += 64)
        if (d0 + i < ids_cap) ids[d0 + i] = stage[i];
    } else {
      uint32_t o = o0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t cj = c[k];
        const uint64_t dst = base + o;
        if (cj > 0 && dst < ids_cap) ids[dst] = v0[k];
        if (cj > 1) {  // merged / long piece: the rest of its ids, four loads in flight at a time
          const uint32_t* spk = sp[k];
          for (uint32_t m = 1; m < cj; m += 4) {
            uint32_t x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = m + i < cj ? spk[m + i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++)
              if (m + i < cj && dst + m + i < ids_cap) ids[dst + m + i] = x[i];  // the host reports CTOK_E_CAPACITY when short
          }
        }
        o += cj;
      }
    }
    // document starts / first ids (after the id stores: no load waits behind them)
    {
      const uint32_t dcur = docs(cur, j0);
      uint32_t dord = acur.d;  // this lane's first doc-start piece's document (direct mode)
      uint32_t o = o0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if ((dcur >> k) & 1u) {
          if (direct) tok_off[dord++] = base + o;
          else tcnt[j0 + k] = o;  // read by k_tokoff
        }
        if (w.keep_first && j0 + k < np) tcnt[j0 + k] = o;  // ctok_encode_offsets
        o += c[k];
      }
    }
    r_first = run;
    wave_sync_lds();  // (the next round's staging overwrites the buffer; its smr reads follow)
    cur = nx;
    nx = nx2;
    acur = anx;
  }
}

// tok_off[d] = first id of the piece that starts at doc_off[d] (every non-empty doc starts a
// piece; an empty doc shares the next doc's start, or the end of the text)
__device__ __forceinline__ void tokoff_one(const Work& w, uint64_t* __restrict__ tok_off, uint32_t d) {
  const uint64_t x = w.doc_off[d];
  uint64_t r;
  if (x >= w.n_bytes) {
    r = w.tile_tok[w.n_tiles];
  } else {
    const uint32_t g = (uint32_t)(x >> 6), b = (uint32_t)(x & 63);
    const uint32_t tile = (uint32_t)(x / kTile);
    uint32_t below = __popc(w.pbits[2 * g] & (b >= 32 ? ~0u : ((1u << b) - 1u)));
    if (b > 32) below += __popc(w.pbits[2 * g + 1] & ((1u << (b - 32)) - 1u));
    const uint32_t j = w.wpref[(size_t)tile * 64 + (g - tile * kTileWords)] + below;
    r = (uint64_t)w.tile_tok[tile] + w.tcnt[(size_t)tile * kTileSlots + j];
  }
  tok_off[d] = r;
}

__global__ void k_tokoff(Work w, uint64_t* __restrict__ tok_off) {
  if (w.host_res && blockIdx.x == 0) {  // the call's results into the host's pinned words
    if (threadIdx.x < (uint32_t)kNumCounters) ((uint32_t*)(w.host_res + 1))[threadIdx.x] = w.counters[threadIdx.x];
    if (threadIdx.x == 0) w.host_res[0] = w.tile_tok[w.n_tiles];
    __threadfence_system();
  }
  if (spec_failed(w)) return;
  if (w.counters[kCtrEmptyDocs] == 0) {  // k_emit wrote tok_off[0 .. n_docs)
    if (blockIdx.x == 0 && threadIdx.x == 0) tok_off[w.n_docs] = w.tile_tok[w.n_tiles];
    return;
  }
  for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d <= w.n_docs; d += gridDim.x * blockDim.x)
    tokoff_one(w, tok_off, d);
}

hipError_t launch_emit(const Work& w, uint32_t* ids, uint64_t ids_cap, uint64_t* tok_off, hipStream_t s,
                       bool count_pieces, bool empty_docs, Lx first, Lx last) {
  HIPCHK(scan_tiles(w, s, count_pieces, first));
  if (w.n_tiles) {
    const uint32_t nb = (w.n_tiles + kEmitWaves - 1) / kEmitWaves;
    if (w.rec16) k_emit<uint16_t><<<nb, 64 * kEmitWaves, 0, s>>>(w, ids, ids_cap, tok_off);
    else k_emit<uint32_t><<<nb, 64 * kEmitWaves, 0, s>>>(w, ids, ids_cap, tok_off);
  }
  // (grid-stride: with no empty document only tok_off[n_docs] is left to write)
  launch_lx(last, k_tokoff, empty_docs ? std::min<uint32_t>((w.n_docs + 1 + 255) / 256, 4096) : 1u, 256, 0, s, w,
            tok_off);
  return hipGetLastError();
}

// p[i] += delta (mod 2^64) for i < n: a host-buffer chunk's doc offsets made chunk-relative, its
// tok_off made batch-relative, on the device before the direct copies
__global__ __launch_bounds__(256) void k_shift_u64(uint64_t* __restrict__ p, uint64_t n, uint64_t delta) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] += delta;
}

// The 16-bit wire format of the host-buffer pipeline (ids16 tokenizers): ids[0, n_ids) as u16
// and tok_off[0, n_off) (chunk-relative, < 2^32) as u32, so the D2H copies move 2 B per id
// instead of 4.  Eight ids per thread: two 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void k_wire16(const uint32_t* __restrict__ ids, uint64_t n_ids, uint16_t* __restrict__ ids16,
                                                const uint64_t* __restrict__ toff, uint64_t n_off,
                                                uint32_t* __restrict__ toff32) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  const uint64_t n8 = n_ids / 8;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const uint4 a = reinterpret_cast<const uint4*>(ids)[2 * i], b = reinterpret_cast<const uint4*>(ids)[2 * i + 1];
    reinterpret_cast<uint4*>(ids16)[i] = make_uint4(a.x | (a.y << 16), a.z | (a.w << 16), b.x | (b.y << 16), b.z | (b.w << 16));
  }
  for (uint64_t i = 8 * n8 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_ids; i += stride) ids16[i] = (uint16_t)ids[i];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_off; i += stride) toff32[i] = (uint32_t)toff[i];
}

hipError_t wire16(const uint32_t* ids, uint64_t n_ids, uint16_t* ids16, const uint64_t* toff, uint64_t n_off,
                  uint32_t* toff32, hipStream_t s) {
  const uint64_t work = std::max<uint64_t>(n_ids / 8, n_off);
  const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((work + 255) / 256, 8192));
  k_wire16<<<g, 256, 0, s>>>(ids, n_ids, ids16, toff, n_off, toff32);
  return hipGetLastError();
}

hipError_t shift_u64(uint64_t* p, uint64_t n, uint64_t delta, hipStream_t s) {
  if (n == 0 || delta == 0) return hipSuccess;
  const uint32_t g = (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096);
  k_shift_u64<<<g, 256, 0, s>>>(p, n, delta);
  return hipGetLastError();
}

}  // namespace ctok_dev
