// Encode path, stage 1 (gfx950 / CDNA4): document starts and the pre-tokenizer -- k_clear,
// k_tilefirst, k_segment.  The later stages: kernels.hip, long.hip,
// emit.hip, scan.hip, nfc.hip; shared device helpers: dev_common.h.
//
// Reference path (Complexity-ML/complexity-tokenizer v0.3.3):
//   HuggingFaceTokenizer::encode_batch   src/huggingface/mod.rs:694-696
//   -> encode                            src/huggingface/mod.rs:551-613
//      NFC                               src/normalizers.rs:47
//      byte_level_pretokenize            src/pretokenizers.rs:158-185 (GPT2_PATTERN :11-15)
//      added-token split                 src/huggingface/mod.rs:566-675
//      BpeTokenizer::encode              src/bpe.rs:88-153
//
// Data layout in HBM (all offsets u32: one call covers < 4 GiB of text):
//   text[B] u8, doc_off[D+1] u64 (input) ->
//   tfirst (each tile's first document) ->
//   pbits: 1 bit per byte (piece start), 4 KiB tiles of 64 64-byte words ->
//   per tile: wpref (pieces before each word), class lists of pieces still to merge, prec[j]
//   (record of piece j: a whole-piece hit's id, u16 on narrow vocabularies), pdoc, tile_np,
//   tile_tok ->
//   per tile: scratch (the merged pieces' ids, by length-class region), mrec[k] (count and place
//   of the tile's k-th merged piece), tile_tok scanned to each tile's first id ->
//   ids[T] u32 + tok_off[D+1] u64 (output).
// No array is indexed by a global piece number, so no pass has to wait for a global piece count.
//
// The regex of GPT2_PATTERN is evaluated as a "piece starts here" predicate over code-point
// classes {White_Space, L, N, other} (derivation in DESIGN.md), bit-parallel on 64-bit masks.
#include "dev_common.h"
#include "seg_lane.h"
#include "seg_route_hd.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// doc-start bitmap

// Each tile's first document (k_segment finds the doc starts of its 64 words from it): tfirst[t] =
// the first doc d with doc_off[d] >= the tile's context word (t * kTile - 64), written by thread d
// for the tiles whose context word lies in (doc_off[d - 1], doc_off[d]] -- at most 64 of them
// (a document over ~250 KB leaves the rest at ~0 from k_clear, and k_segment searches for those);
// and the empty documents, counted into counters[kCtrEmptyDocs] (one atomic per wave).  It
// replaces a doc-start bitmap of n_bytes / 8 bytes, zeroed, written and read back every call.
__global__ __launch_bounds__(256) void k_tilefirst(const uint64_t* __restrict__ off, uint32_t n_docs, uint32_t n_tiles,
                                                   uint32_t* __restrict__ tfirst, uint32_t* __restrict__ counters) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  bool empty = false;
  if (d <= n_docs && n_tiles) {
    const uint64_t y = off[d];
    empty = d < n_docs && y == off[d + 1];
    // tiles t with off[d - 1] < t * kTile - 64 <= y (d = 0: every t with t * kTile - 64 <= y)
    const uint64_t t_lo = d ? (off[d - 1] + 64) / kTile + 1 : 0ull;
    const uint64_t t_hi = min((y + 64) / kTile, (uint64_t)n_tiles - 1);
    for (uint64_t t = t_lo; t <= t_hi && t < t_lo + 64; t++) tfirst[t] = d;
  } else if (d < n_docs) {
    empty = off[d] == off[d + 1];
  }
  const uint64_t me = __ballot(empty);
  if (me && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)me) - 1)
    atomicAdd(&counters[kCtrEmptyDocs], (uint32_t)__popcll(me));
}

// The same for one tile, by bisection (k_segment: a tile whose context word lies inside a document
// longer than k_tilefirst's 64 tiles).  Wave-uniform.
__device__ uint32_t tile_first_search(const uint64_t* off, uint32_t n_docs, uint32_t tile) {
  const uint64_t key = tile ? (uint64_t)tile * kTile - 64 : 0ull;
  uint32_t lo = 0, hi = n_docs;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (__builtin_amdgcn_readfirstlane((uint32_t)(off[mid] < key))) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Zeroes the call's counters (when asked) and the NFC watch bitmap (nfc_watch 2) in one launch.
__device__ __forceinline__ void clear_words(uint32_t* __restrict__ p, uint64_t n) {
  const uint64_t n4 = n / 4;
  uint4* p4 = reinterpret_cast<uint4*>(p);  // (hipMalloc'd: 256-byte aligned)
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256)
    p4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) p[4 * n4 + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(256) void k_clear(uint32_t* __restrict__ bits, uint64_t n, uint32_t* __restrict__ counters,
                                               uint32_t* __restrict__ tfirst, uint32_t n_tiles) {
  if (bits) clear_words(bits, n);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_tiles; i += gridDim.x * 256) tfirst[i] = ~0u;
  if (blockIdx.x == 0 && counters && threadIdx.x < (uint32_t)kCounterWords) counters[threadIdx.x] = 0u;
}

uint64_t nfc_bits_words(uint64_t n_bytes) { return (n_bytes + 2047) / 2048 + 8; }

hipError_t launch_docstart(const Work& w, hipStream_t s, bool zero_counters, Lx x, Lx x2) {
  const bool nfc = w.nfc_watch == 2;
  const uint64_t n = nfc ? nfc_bits_words(w.n_bytes) : 0;
  const uint64_t work = std::max<uint64_t>(n / 4, w.n_tiles);
  launch_lx(x, k_clear, (unsigned)std::min<uint64_t>((work + 255) / 256 + 1, 8ull * w.n_cus), 256, 0, s,
            nfc ? w.nfc_bits : nullptr, n, zero_counters ? w.counters : nullptr, w.tfirst, w.n_tiles);
  if (w.n_tiles) launch_lx(x2, k_tilefirst, (w.n_docs + 1 + 255) / 256, 256, 0, s, w.doc_off, w.n_docs, w.n_tiles, w.tfirst, w.counters);
  else if (w.n_docs)  // (no text: only the empty-document count)
    k_tilefirst<<<(w.n_docs + 255) / 256, 256, 0, s>>>(w.doc_off, w.n_docs, 0, w.tfirst, w.counters);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// pre-tokenizer: piece-start bitmap, bit-parallel, one 64-byte word per lane (k_segment below;
// the per-word logic is csrc/seg_lane.h).  Positions >= n_bytes read as doc starts (D), which
// closes every run at the end of the text.

// Whole-piece table lookup given the first probed slot e (at h): the vocab id, or kNone.
__device__ __forceinline__ uint32_t piece_probe(const Tables& t, uint4 e, uint32_t h, uint32_t lo, uint32_t hi,
                                                uint32_t n) {
  while (e.z != 0) {  // linear probing past the first slot (rare)
    if (e.x == lo && e.y == hi && e.z == n) return e.w;
    h = (h + 1) & t.piece_mask;
    e = t.piece_tab[h];
  }
  return kNone;
}

// The wave's LDS accesses before this point are ordered before those after it (its lanes hand
// data to each other through LDS without a workgroup barrier).
__device__ __forceinline__ void seg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// position of the k-th (0-based) set bit of x (k < popcount(x))
__device__ __forceinline__ uint32_t select_bit(uint64_t x, uint32_t k) {
  uint32_t pos = 0;
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  uint32_t c = __popc(lo);
  uint32_t v = lo;
  if (k >= c) { k -= c; v = hi; pos = 32; }
#pragma unroll
  for (int wdt = 16; wdt >= 1; wdt >>= 1) {
    const uint32_t m = (1u << wdt) - 1u;
    c = __popc(v & m);
    if (k >= c) { k -= c; v >>= wdt; pos += wdt; }
  }
  return pos;
}




// One wavefront per tile, kSegWaves tiles per workgroup, no workgroup barrier.  Lane l owns the
// 64-byte word g0 - 1 + l: lane 0 is the previous tile's last word (context only), lanes 1..62
// are the tile's words, lane 63 is the next tile's first word (look-ahead: where the tile's last
// piece ends; its bits 62-63 depend on a word no lane holds and are not used).
//  A. per lane: the word's class / byte masks by SWAR tests (csrc/seg_lane.h); non-ASCII code
//     points classified per code point; doc starts from the documents' offsets;
//  B. per lane: the piece-start predicate, the neighbouring words' masks by cross-lane shuffles;
//     then the doc-start bits by piece number (pdoc), once per tile, from each word's D & st;
//  C. thread per piece (piece j = the j-th start of the tile): length from the next start, then
//     routing: a piece of <= 8 bytes that is one self-encoding vocab token is finished here with
//     one whole-piece probe; every other piece is appended to its tile's class list (<= 8 B,
//     9..16 B, 17..32 B) or to the long list, so that the merge passes run dense, length-uniform
//     waves.  A round is kSegUnroll slots of 64 pieces; the round's merged pieces are compacted
//     in LDS and appended once per round (C4 k_segment 2.64 -> 2.52 ms, profiles/seg_routing/).
//     (The mask gathers on dot products and pdoc once per tile: 2.52 -> 2.38 ms, profiles/seg_front/.)
//     A round with at most 128 pieces runs a body of two slots instead of four ("live slots":
//     2.38 -> 2.16 ms, C5 1.65 -> 1.57 ms, profiles/seg_live/).
// (amdgpu_waves_per_eu(7): at most 72 VGPRs, 7 waves per SIMD; without it the compiler takes 72-73
// and this kernel runs at 6-7; C4 k_segment 2.78 -> 2.67 ms, 8 waves spill: 2.96 ms,
// profiles/r03/v30_ab_seg_waves_per_eu.txt)
// Diagnostic build only (-DCTOK_SEG_STAMPS): shader-clock stamps at k_segment's phase boundaries,
// one row of 8 u64 per tile in Work::stamps (read by the host with CTOK_STAMPS=1); the production
// build executes none.  Read the phases' shares, not the build's run time.
#ifdef CTOK_SEG_STAMPS
#define SEG_STAMP(k)                                                                              \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    unsigned long long t_;                                                                        \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                     \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (w.stamps && lane == 0) w.stamps[(size_t)tile * 8 + (k)] = t_;                            \
  } while (0)
#else
#define SEG_STAMP(k) do { } while (0)
#endif
// R16: u16 piece records (Work::rec16); a template parameter, not a branch on the flag: both store
// paths in one kernel cost 18 more spilled SGPRs
template <bool R16>
__global__ __launch_bounds__(64 * kSegWaves) __attribute__((amdgpu_waves_per_eu(7))) void k_segment(Work w, Tables t) {
  // one round's piece starts (later in the round a merged piece's class is marked on its start)
  __shared__ uint16_t s_pos_all[kSegWaves][64 * kSegUnroll + 8];
  // per wave: 3 spare words, the 4 bytes before the context word, the context word, the tile, the
  // look-ahead word, the 4 bytes after it, 3 spare words (rows of 1032 words: every lane's 64-byte
  // word starts 16-byte aligned for its four 16-byte stores)
  __shared__ __attribute__((aligned(16))) uint32_t s_text_all[kSegWaves][(kTileWords + 2) * 16 + 8];
  __shared__ uint64_t s_D_all[kSegWaves][64];
  constexpr uint32_t kSegLongCap = 32;  // long pieces staged per tile (the list entries)
  __shared__ uint64_t s_long_all[kSegWaves][kSegLongCap];
  __shared__ uint8_t s_buf_all[kSegWaves][kSegListBuf];  // a round's merged pieces (phase C)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wid = uni(threadIdx.x >> 6);
  const uint32_t tile = uni(blockIdx.x * kSegWaves + wid);
  if (tile >= w.n_tiles) return;
  uint16_t* s_pos = s_pos_all[wid];
  SEG_STAMP(0);
  const uint32_t B = w.n_bytes;
  const uint32_t t0 = tile * kTile;
  const int64_t g = (int64_t)tile * kTileWords - 1 + lane;  // this lane's word
  const bool first = lane == 0, last = lane == 63;

  // ---- A
  uint32_t x[16];
  uint64_t D, valid;
  {
    const int64_t x0 = g * 64;
    if (x0 >= 0 && x0 + 64 <= (int64_t)B) {
      const uint4* p = reinterpret_cast<const uint4*>(w.text + x0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint4 v = p[k];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
      }
      valid = ~0ull;
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) x[k] = 0;
      valid = 0;
      if (x0 >= 0 && x0 < (int64_t)B) {  // the text's last, partial word
        const uint32_t n = B - (uint32_t)x0;
        valid = (1ull << n) - 1;
        for (uint32_t i = 0; i < n; i++) x[i >> 2] |= (uint32_t)w.text[x0 + i] << (8 * (i & 3));
      }
    }
  }
  // the first 64 documents from the tile's first (k_tilefirst), loaded right behind the text
  // (their starts give the doc-start bits below; the mask work on the text runs meanwhile)
  uint32_t dfirst = uni(w.tfirst[tile]);
  if (dfirst == ~0u) dfirst = tile_first_search(w.doc_off, w.n_docs, tile);  // (inside a document > 250 KB)
  uint64_t xs0 = ~0ull, ys0 = ~0ull;
  if (dfirst + lane < w.n_docs) {
    xs0 = w.doc_off[dfirst + lane];
    ys0 = w.doc_off[dfirst + lane + 1];
  }
  seg::Masks m = seg::ascii_masks(x);
  // the masks are complete here: their gathers must not sink below the doc-start block, away from
  // the tests that feed them (96 flag dwords would then be live at once and spill)
  asm volatile("" : "+v"(m.W), "+v"(m.L), "+v"(m.N), "+v"(m.S), "+v"(m.Q), "+v"(m.NA));
  {  // doc-start bits of the 64 words [base, base + 4096): the non-empty documents starting there,
     // from the tile's first document on (k_tilefirst), 64 at a time (C4: one round)
    uint64_t* s_D = s_D_all[wid];
    s_D[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t base = (uint64_t)t0 - 64;  // (tile 0: -64, wrapping; the sums below wrap back)
    const uint64_t lim = (uint64_t)t0 + 4032;  // the window's end
    auto mark = [&](uint64_t xs, uint64_t ys) {  // (xs = ~0: no document)
      const bool in = xs < lim;
      if (in && xs != ys) {
        const uint64_t r = xs - base;
        atomicOr((unsigned long long*)&s_D[r >> 6], 1ull << (r & 63));
      }
      return in;
    };
    if (__ballot(mark(xs0, ys0)) == ~0ull) {  // every lane's doc started inside: look further (rare)
      for (uint32_t d = dfirst + 64;; d += 64) {
        const uint32_t i = d + lane;
        uint64_t xs = ~0ull, ys = ~0ull;
        if (i < w.n_docs) {
          xs = w.doc_off[i];
          ys = w.doc_off[i + 1];
        }
        if (__ballot(mark(xs, ys)) != ~0ull) break;
      }
    }
    seg_wave_sync();
    const int64_t x0 = g * 64;
    if (x0 < 0) D = 0;
    else if (x0 >= (int64_t)B) D = ~0ull;
    else D = s_D[lane] | ~valid;
  }
  // every lane's word in LDS: the tile's bytes (and the look-ahead word) for the whole-piece
  // probes (s_text: the tile's first byte), the context word too for the code point decoding below
  uint32_t* s_all = s_text_all[wid] + 4;  // (s_all[-1]: the 4 bytes before the context word)
  uint32_t* s_text = s_all + 16;
  // the context word's first code point can start in the word before it (its first byte is a
  // continuation byte): the 4 bytes before it
  if (first && (x[0] & 0xC0u) == 0x80u && g * 64 >= 4)
    s_all[-1] = *reinterpret_cast<const uint32_t*>(w.text + g * 64 - 4);
#pragma unroll
  for (int k = 0; k < 4; k++)
    *reinterpret_cast<uint4*>(s_all + lane * 16 + 4 * k) = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
  if (last) {  // the 4 bytes after the look-ahead word: a code point starting in its last bytes
               // runs into them (zero past the text)
    const int64_t xe = g * 64 + 64;
    uint32_t v = 0;
    if (xe + 4 <= (int64_t)B) {
      v = *reinterpret_cast<const uint32_t*>(w.text + xe);
    } else {
      for (int64_t i = xe; i < (int64_t)B && i < xe + 4; i++) v |= (uint32_t)w.text[i] << (8 * (uint32_t)(i - xe));
    }
    s_all[64 * 16] = v;
  }
  seg_wave_sync();
  SEG_STAMP(1);
  if (m.NA) {  // non-ASCII code points: classes and NFC flags from the two-level tables
    constexpr int kSegCp = 4;
    bool nfc_bad = false;
    auto set_class = [&](int cl, uint64_t bits) {
      if (cl == 0) m.W |= bits & m.NA;
      else if (cl == 1) m.L |= bits & m.NA;
      else if (cl == 2) m.N |= bits & m.NA;
    };
    // continuation bytes (10xxxxxx), SWAR over the word's dwords
    uint64_t cont = 0;
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
      const uint32_t c0 = x[k] & ~(x[k] << 1) & seg::kHi, c1 = x[k + 1] & ~(x[k + 1] << 1) & seg::kHi;
      cont |= (uint64_t)seg::pack8(c0, c1) << (4 * k);
    }
    cont &= m.NA;
    const uint64_t lead_cont = cont & ~(cont + 1);  // continuation bytes at the start of the word
    if (lead_cont) {  // a code point whose lead is in the previous word: classified on its own
      // the bytes before this word are staged just before it (the previous lane's word, or for
      // the context word s_all[-1]): the lead is 1..3 bytes back (at most 3 steps back, as a
      // walk over the text would take)
      const uint32_t pw = s_all[lane * 16 - 1];  // bytes x0 - 4 .. x0 - 1
      const int32_t back = ((pw >> 24) & 0xC0u) != 0x80u ? 1 : ((pw >> 16) & 0xC0u) != 0x80u ? 2 : 3;
      const int32_t a = (int32_t)lane * 64 - back;  // byte address in s_all (-3 .. -1 for the context word)
      const uint32_t v = __builtin_amdgcn_alignbyte(s_all[(a >> 2) + 1], s_all[a >> 2], (uint32_t)a & 3u);
      const uint32_t b0 = v & 255u, b1 = (v >> 8) & 0x3Fu, b2 = (v >> 16) & 0x3Fu, b3 = (v >> 24) & 0x3Fu;
      const int l = u8len((uint8_t)b0);
      const uint32_t c = l == 2 ? ((b0 & 0x1Fu) << 6) | b1
                       : l == 3 ? ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2
                       : l == 4 ? ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3 : b0;
      const int rc = t.cp_fast ? cp_range_class(c) : -1;
      const int cw = rc >= 0 ? rc : (cls_of(c, t) | (nfc16(t, c) != 0 ? 4 : 0));
      nfc_bad |= (cw & 4) != 0;
      set_class(cw & 3, lead_cont);
    }
    // every other code point starts at a lead byte in this word: decoded and looked up 8 at a
    // time, so the byte loads, then both first-level table loads, then both second-level table
    // loads of the 8 are in flight together (instead of a chain of dependent loads per code point)
    uint64_t leads = m.NA & ~cont;
    while (leads) {
      uint32_t pos[kSegCp], cp[kSegCp], len[kSegCp];
#pragma unroll
      for (int k = 0; k < kSegCp; k++) {
        pos[k] = leads ? (uint32_t)__builtin_ctzll(leads) : 64u;
        leads &= leads ? leads - 1 : 0ull;
      }
#pragma unroll
      for (int k = 0; k < kSegCp; k++) {
        // the code point's bytes from LDS (this lane's word and the next: s_all is contiguous;
        // valid UTF-8 never runs past the text, whose bytes past B read as zero)
        const uint32_t a = lane * 64 + min(pos[k], 63u);
        const uint32_t v = __builtin_amdgcn_alignbyte(s_all[(a >> 2) + 1], s_all[a >> 2], a & 3);
        const uint32_t b0 = v & 255u, b1 = (v >> 8) & 0x3Fu, b2 = (v >> 16) & 0x3Fu, b3 = (v >> 24) & 0x3Fu;
        const int l = u8len((uint8_t)b0);
        len[k] = (uint32_t)l;
        cp[k] = l == 2 ? ((b0 & 0x1Fu) << 6) | b1
              : l == 3 ? ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2
              : l == 4 ? ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3 : b0;
      }
      int rc[kSegCp];  // range-test class, -1: look it up
      uint32_t s1[kSegCp];
#pragma unroll
      for (int k = 0; k < kSegCp; k++) {
        rc[k] = t.cp_fast ? cp_range_class(cp[k]) : -1;
        const bool in = pos[k] < 64 && cp[k] < 0x110000 && rc[k] < 0;
        // BMP code points: class and NFC flag in one load from the direct table (cls_bmp); the
        // rare supplementary ones outside the fast ranges: two-level lookups in the branch below
        s1[k] = in && cp[k] < 0x10000 ? (uint32_t)t.cls_bmp[cp[k] >> 1] : 0u;
      }
#pragma unroll
      for (int k = 0; k < kSegCp; k++) {
        if (pos[k] >= 64) continue;
        const uint32_t c = cp[k];
        int cl = 3;
        bool nf = false;
        if (rc[k] >= 0) {
          cl = rc[k];
        } else if (c < 0x80) {
          cl = cls_ascii(c);
        } else if (c < 0x10000) {
          const uint32_t v = s1[k] >> ((c & 1u) * 4);
          cl = (int)(v & 3u);
          nf = (v & 4u) != 0;
        } else if (c < 0x110000) {
          cl = cls_of(c, t);
          nf = nfc16(t, c) != 0;
        }
        nfc_bad |= nf;
        const uint32_t p = pos[k];
        const uint64_t bits = (len[k] >= 64 - p ? ~0ull : ((1ull << len[k]) - 1)) << p;
        set_class(cl, bits);
      }
    }
    if (nfc_bad && w.nfc_watch) {
      atomicOr(&w.counters[kCtrNfcFlag], 1u);
      if (w.nfc_watch == 2 && g >= 0) atomicOr(&w.nfc_bits[g >> 5], 1u << (g & 31));  // (splice mode only)
    }
  }
  SEG_STAMP(2);
  // contraction letters only where an apostrophe could use them (this word's or the previous
  // word's last two bytes)
  // (every lane takes part in each shuffle: a lane that is inactive at a ds_bpermute hands its
  // neighbour zeros)
  uint64_t pQ = shfl_up64(m.Q);
  if (first) pQ = 0;
  seg::Letters lt{0, 0, 0, 0, 0};
  if (m.Q | (pQ >> 62)) lt = seg::letter_masks(x, m.NA);

  // ---- B
  uint64_t st;
  {
    uint64_t pW = shfl_up64(m.W), pL = shfl_up64(m.L), pN = shfl_up64(m.N);
    if (first) pW = pL = pN = 0;
    uint64_t nW = shfl_down64(m.W), nL = shfl_down64(m.L), nD = shfl_down64(D);
    seg::Letters nl{shfl_down64(lt.T1), shfl_down64(lt.R), shfl_down64(lt.Le), shfl_down64(lt.V), shfl_down64(lt.LL)};
    if (last) {
      nW = nL = nD = 0;
      nl = seg::Letters{0, 0, 0, 0, 0};
    }
    const uint64_t A = seg::attached(m, D, pW, nW, nD);
    uint64_t pA = shfl_up64(A);
    if (first) pA = 0;
    uint64_t C1, C2;
    seg::contractions(m, lt, D, A, pA, ~(pW | pL | pN), nL, nD, nl, C1, C2);
    uint64_t pC1 = shfl_up64(C1), pC2 = shfl_up64(C2);
    if (first) pC1 = pC2 = 0;
    st = seg::starts(m, D, pW, pL, pN, A, pA, C1, C2, pC1, pC2) & valid;
    if (last) st &= (1ull << 62) - 1;
    if (!first && !last) {  // piece-start bitmap
      const uint64_t gw = (uint64_t)g * 2;
      if (gw < w.n_words) w.pbits[gw] = (uint32_t)st;
      if (gw + 1 < w.n_words) w.pbits[gw + 1] = (uint32_t)(st >> 32);
    }
  }
  // documents starting in the tile: its words' doc-start bits within the text (summed at the end)
  const uint32_t nd = uni(wave_sum_full_u32((!first && !last) ? (uint32_t)__popcll(D & valid) : 0u));
  const uint32_t c = (!first && !last) ? (uint32_t)__popcll(st) : 0u;
  const uint32_t inc = wave_incl_scan(c);
  if (!first && !last) w.wpref[(size_t)tile * 64 + lane - 1] = (uint16_t)(inc - c);
  const uint32_t np = lane63(inc);
  // where the tile's last piece ends (look-ahead lane): 0xFFFF = unknown (longer than the
  // look-ahead can tell: a long piece)
  const uint32_t tile_end =
      uni((uint32_t)__shfl((int)(st ? (uint32_t)(kTileWords * 64 + __builtin_ctzll(st))
                                    : ((uint64_t)B <= (uint64_t)t0 + kTile + 62 ? (uint32_t)(B - t0) : 0xFFFFu)),
                           63, 64));
  // expansion state: the starts of this lane's word and the pieces of the tile before it
  const uint64_t stw = (!first && !last) ? st : 0ull;
  const uint32_t prew = inc - c;
  uint32_t wcur = 1;  // the first word lane that can hold the next window's first piece (wave-uniform)
  uint32_t* pdoc = w.pdoc + (size_t)tile * (kTileSlots / 32);
  {  // pdoc, bit j: piece j starts a document.  Each word lane ORs its doc starts' piece numbers
     // (about one start in 36 on C4) into a bitmap of kTileSlots bits, which the wave stores in one
     // coalesced pass.  The bitmap lies over s_D, dead since every lane holds its D.
    static_assert(kTileSlots == 64 * 64, "the pdoc bitmap of a tile: s_D's 64 u64 words");
    // (its own address arithmetic: phase A's &s_D[lane], kept alive down to here, was spilled)
    uint32_t dl = lane;
    asm volatile("" : "+v"(dl));
    uint64_t* s_doc = s_D_all[wid];
    s_doc[dl] = 0;
    seg_wave_sync();
    seg::doc_pieces(stw, D, prew, [&](uint32_t j) { atomicOr((uint32_t*)s_doc + (j >> 5), 1u << (j & 31)); });
    seg_wave_sync();
    if (lane * 64 < np) {
      const uint64_t dm = s_doc[dl];
      *reinterpret_cast<uint2*>(pdoc + 2 * lane) = make_uint2((uint32_t)dm, (uint32_t)(dm >> 32));
    }
  }

  SEG_STAMP(3);
  // ---- C: thread per piece, kSegUnroll pieces per lane per round with their LDS lookups and
  // table probes issued together (each round is one dependent global round trip)
  const bool generic = t.n_at != 0;  // added tokens can match inside pieces: no whole-piece shortcut
  using RecT = typename std::conditional<R16, uint16_t, uint32_t>::type;
  RecT* prec = (RecT*)w.prec + (size_t)tile * kTileSlots;
  uint32_t nm = 0;  // merged pieces so far (wave-uniform): the next ordinal
  uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;  // class-list lengths (wave-uniform)
  uint32_t nlong = 0;  // long pieces staged in s_long_all (wave-uniform)
  // this lane's bytes in class lists 0..2 (the id regions) and its whole-piece hits, two 16-bit
  // sums per register (a tile's are below 4096 each): by0 | by1 << 16, by2 | hits << 16
  uint32_t by01 = 0, by2h = 0;
  constexpr int U = kSegUnroll;
  constexpr uint32_t W = 64 * U;  // pieces per round
  static_assert(U == 4, "kSegUnroll: 4 (the probes of a round are unrolled by hand)");
  // The round's merged pieces, compacted in piece order: s_buf[k] = the round's k-th merged
  // piece (its index within the round), whose class is marked on its start in s_pos (seg_mark;
  // every slot has read the raw starts and ends by then).  The list appends run once per 64
  // compacted pieces (flush) instead of once per slot of 64 pieces of which ~9 are merged.
  static_assert(kSegListBuf == W && W <= 256, "s_buf: a whole round's pieces, one byte each");
  uint8_t* s_buf = s_buf_all[wid];
  uint32_t cnt = 0;  // entries in s_buf (wave-uniform); the first one's ordinal is nm
  // The walk over the compacted pieces, 64 per pass: class-0 spill, the four list appends, the
  // id-region byte sums and the long-piece staging.  Entry i has ordinal nm + i.
  auto flush = [&]() __attribute__((always_inline)) {
    const uint64_t below = lanemask_lt();
    for (uint32_t p0 = 0; p0 < cnt; p0 += 64) {
      const uint32_t i = p0 + lane, ord = nm + i;
      uint32_t bsl = 0, bn = 0;  // start; length (a long piece's: 0 when it ends past the look-ahead)
      uint32_t cl = 4;  // 0..2 class lists, 3 long, 4 none, 6 class list 3
      if (i < cnt) {
        const uint32_t k = s_buf[i];
        const uint32_t a = s_pos[k], el = s_pos[k + 1];  // (the next piece's start: marked or raw)
        bsl = seg_mark_start(a);
        cl = seg_mark_class(a);
        bn = el == 0xFFFFu ? 0u : seg_mark_start(el) - bsl;
      }
      uint64_t m0 = __ballot(cl == 0);
      // the tile's class-0 list is full: the rest of its class-0 pieces go to the long list (the
      // first w.k0 of the tile, in piece order, stay)
      if (n0 + (uint32_t)__popcll(m0) > w.k0) {
        if (cl == 0 && n0 + (uint32_t)__popcll(m0 & below) >= w.k0) cl = 3;
        m0 = __ballot(cl == 0);
      }
      const uint32_t e = list_entry(bsl, ord, bn);
      {  // the wave owns its tile's lists: running counts in scalar registers, no atomics
        const uint64_t m1 = __ballot(cl == 1), m2 = __ballot(cl == 2);
        const uint64_t m3 = __ballot(cl == 6);
        if (cl == 0) w.list0[(size_t)tile * w.k0 + n0 + __popcll(m0 & below)] = e;
        if (cl == 1) w.list1[(size_t)tile * kCap1 + n1 + __popcll(m1 & below)] = e;
        if (cl == 2) w.list2[(size_t)tile * kCap2 + n2 + __popcll(m2 & below)] = e;
        if (cl == 6) w.list3[(size_t)tile * kCap3 + n3 + __popcll(m3 & below)] = e;
        by01 += cl == 0 ? bn : cl == 1 ? bn << 16 : 0u;
        by2h += cl == 2 ? bn : 0u;
        n0 += __popcll(m0);
        n1 += __popcll(m1);
        n2 += __popcll(m2);
        n3 += __popcll(m3);
      }
      const uint64_t lm = __ballot(cl == 3);
      // long pieces staged in LDS; one global atomic for the tile's whole batch at the end (a
      // returned atomic per round on the shared counter stalled the wave for its round trip).
      // bn: the length when the piece ends within the look-ahead (0: k_long_len finds its end)
      const uint64_t le = (uint64_t)(t0 + bsl) | ((uint64_t)ord << 32) | ((uint64_t)bn << 44);
      if (lm && nlong + (uint32_t)__popcll(lm) <= kSegLongCap) {
        if (cl == 3) s_long_all[wid][nlong + __popcll(lm & below)] = le;
        nlong += (uint32_t)__popcll(lm);
      } else if (lm) {  // (past kSegLongCap long pieces in the tile: one global atomic per pass)
        const uint32_t leader = __ffsll((unsigned long long)lm) - 1;
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(&w.counters[kCtrLong], (uint32_t)__popcll(lm));
        b = __builtin_amdgcn_readlane(b, leader);
        const uint32_t li = b + __popcll(lm & below);
        if (cl == 3 && li < w.long_cap) w.long_list[li] = le;
        if (lane == leader && b + __popcll(lm) > w.long_cap) atomicOr(&w.counters[kCtrOverflow], 1u);
      }
    }
    nm += cnt;
    cnt = 0;
  };
  for (uint32_t j0 = 0; j0 < np; j0 += W) {
    // expansion of this round's window [j0, j0 + W]: s_pos[j - j0] = start of piece j (the
    // entry past the window is the next round's first piece, peeked, not consumed).
    // Half-words over the lanes: lane l takes half (l & 1) of word wb + (l >> 1), 32 words per
    // pass (a window of 256 pieces spans ~18 words of English text: one pass), and walks its
    // half's set bits -- a trip count of the busiest half (~10), against ten VALU per word of
    // the round-3 word-serial walk (C4 k_segment 2.72 -> 2.66 ms, profiles/r05/v16_*).
    for (uint32_t wb = wcur;; wb += 32) {  // (wave-uniform)
      const uint32_t wl = wb + (lane >> 1), src = min(wl, 63u);
      const uint32_t lo32 = (uint32_t)__shfl((int)(uint32_t)stw, (int)src, 64);
      const uint32_t hi32 = (uint32_t)__shfl((int)(uint32_t)(stw >> 32), (int)src, 64);
      const uint32_t pw = (uint32_t)__shfl((int)prew, (int)src, 64);
      const bool hi = (lane & 1) != 0;
      uint32_t bits = wl <= (uint32_t)kTileWords ? (hi ? hi32 : lo32) : 0u;
      uint32_t k = pw + (hi ? (uint32_t)__popc(lo32) : 0u);  // piece index of the half's first start
      if (k > j0 + W || k + (uint32_t)__popc(bits) <= j0) bits = 0;  // no piece of the window
      const uint32_t pos0 = (wl - 1) * 64 + (hi ? 32u : 0u);
      while (bits) {
        const uint32_t b = (uint32_t)__builtin_ctz(bits);
        if (k >= j0 && k <= j0 + W) s_pos[k - j0] = (uint16_t)(pos0 + b);
        bits &= bits - 1u;
        k++;
      }
      const uint32_t wn = wb + 32;  // the next pass's first word: needed when it starts a piece of the window
      if (wn > (uint32_t)kTileWords || uni(__builtin_amdgcn_readlane(prew, wn)) > j0 + W) break;
    }
    {  // the last word whose first piece index is within the window (the next window starts there)
      const uint64_t inw = __ballot(lane >= wcur && lane <= (uint32_t)kTileWords && prew <= j0 + W);
      if (inw) wcur = 63u - (uint32_t)__builtin_clzll(inw);
    }

    if (lane == 0 && np <= j0 + W) s_pos[np - j0] = (uint16_t)tile_end;
    seg_wave_sync();
    // Live slots: a round with at most two slots of pieces (a C4 tile's fifth round) runs a body
    // of two slots; it never touches slots 2 and 3 -- front, probe, record, store, mark,
    // compaction -- so it sees nothing that the round before left in them.
    const bool upper = uni((uint32_t)(j0 + 128 < np)) != 0;
    uint32_t sl[U], n[U], cls[U], plo[U], phi[U], h[U];
    auto front = [&](int u) __attribute__((always_inline)) {
      const uint32_t j = j0 + 64 * u + lane;
      sl[u] = 0;
      n[u] = 0;
      cls[u] = 4;  // 0..2 class lists, 3 long, 4 done (or inactive), 5 probe, 6 class list 3
      if (j < np) {
        sl[u] = s_pos[64 * u + lane];
        const uint32_t el = s_pos[64 * u + lane + 1];
        if (el == 0xFFFFu || el - sl[u] > (generic ? (uint32_t)kShortMax : (uint32_t)kMedMax)) {
          cls[u] = 3;
        } else {
          n[u] = el - sl[u];
          cls[u] = generic ? 0 : n[u] > 32 ? 6 : n[u] > 16 ? 2 : n[u] > 8 ? 1 : 5;
        }
      }
      const uint32_t a = sl[u] >> 2, sh = sl[u] & 3;
      const uint32_t d0 = s_text[a], d1 = s_text[a + 1], d2 = s_text[a + 2];
      const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
      const uint32_t nn = n[u];
      plo[u] = nn >= 4 ? w0 : w0 & ((1u << (8 * nn)) - 1u);
      phi[u] = nn >= 8 ? w1 : nn <= 4 ? 0u : w1 & ((1u << (8 * (nn - 4))) - 1u);
      h[u] = cls[u] == 5 ? piece_hash(plo[u], phi[u], nn) & t.piece_mask : t.piece_mask + 1;
    };
    // The slot's probe result becomes its record (hitv[u]) and its class after the probe.
    // (written as flag arithmetic: an if / else-if chain assigning cls[u] in each arm was
    // miscompiled by this hipcc in the unrolled loop)
    uint32_t hitv[U];
    auto record = [&](int u, const uint4 e) __attribute__((always_inline)) {
      uint32_t rec = kRecMerged32;  // a later pass produces the piece's ids (its mrec slot)
      if (cls[u] == 5) {
        const uint32_t id = piece_probe(t, e, h[u], plo[u], phi[u], n[u]);
        const bool hit = id != kNone;
        rec = hit ? id : kRecMerged32;
        by2h += hit ? 0x10000u : 0u;
        cls[u] = hit ? 4u : 0u;
      }
      hitv[u] = rec;
    };
    // every piece's record: whole coalesced lines (u16 on narrow vocabularies)
    auto store = [&](int u) __attribute__((always_inline)) {
      const uint32_t j = j0 + 64 * u + lane;
      if (j < np) prec[j] = (RecT)hitv[u];
    };
    // Two bodies, chosen by a wave-uniform branch; the full one is the round as it was.  In each,
    // the fronts of all its slots run together (their LDS reads overlap), then all first probes
    // are in flight together, and each slot's record is stored as soon as it is made: a wave waits
    // for a probe entry only where one of its lanes probes, and a slot without a probing lane never
    // waits at all.  (Measured the other way -- one body with slots 2 and 3 under `upper`, every
    // entry waited for at one point ahead of the stores -- C4 gained 0.11 ms more and C5 lost 0.07:
    // profiles/seg_live/.)  (The probes are spelled out: a loop over u around the probing loop
    // would not unroll, and the arrays would go to scratch.)
    if (upper) {
      front(0);
      front(1);
      front(2);
      front(3);
      const uint4 e0 = t.piece_tab[h[0]], e1 = t.piece_tab[h[1]], e2 = t.piece_tab[h[2]], e3 = t.piece_tab[h[3]];
      record(0, e0);
      store(0);
      record(1, e1);
      store(1);
      record(2, e2);
      store(2);
      record(3, e3);
      store(3);
    } else {
      front(0);
      front(1);
      const uint4 e0 = t.piece_tab[h[0]], e1 = t.piece_tab[h[1]];
      record(0, e0);
      store(0);
      record(1, e1);
      store(1);
    }
    // per slot only the compaction: the piece's class marked on its start, its index within the
    // round at its ordinal within the round
    auto compact = [&](int u) __attribute__((always_inline)) {
      const uint64_t mm = __ballot(cls[u] != 4);
      if (cls[u] != 4) {
        s_pos[64 * u + lane] = (uint16_t)seg_mark(sl[u], cls[u]);
        s_buf[cnt + (uint32_t)__popcll(mm & lanemask_lt())] = (uint8_t)(64 * u + lane);
      }
      cnt += (uint32_t)__popcll(mm);
    };
    seg_wave_sync();  // every slot's s_pos reads before the first mark lands on them
    compact(0);
    compact(1);
    if (upper) {
      compact(2);
      compact(3);
    }
    seg_wave_sync();
    flush();
    // every lane has read this round's s_pos before the next round's expansion overwrites it
    seg_wave_sync();
  }
  if (nlong) {  // the tile's staged long pieces: one reservation, coalesced entry stores
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(&w.counters[kCtrLong], nlong);
    b = __builtin_amdgcn_readfirstlane(b);
    seg_wave_sync();
    if (lane < nlong && b + lane < w.long_cap) w.long_list[b + lane] = s_long_all[wid][lane];
    if (lane == 0 && b + nlong > w.long_cap) atomicOr(&w.counters[kCtrOverflow], 1u);
  }
  SEG_STAMP(4);
  by01 = wave_sum_full_u32(by01);
  by2h = wave_sum_full_u32(by2h);
  const uint32_t by0 = by01 & 0xFFFFu, by1 = by01 >> 16, by2 = by2h & 0xFFFFu, hits = by2h >> 16;
  if (lane == 0) {
    w.tile_tok[tile] = hits;  // initial token count (the merge passes add theirs atomically)
    w.tile_doc[tile] = nd;
    w.tile_np[tile] = np;
    // id regions of the register passes (ids <= bytes per piece; all four fit in kTileSlots:
    // the lists hold pieces that start in the tile and end within its 62-byte look-ahead)
    w.tregion[tile] = make_uint2(by0 | ((by0 + by1) << 16), by0 + by1 + by2);
  }
  if (lane < kNumClasses)  // (the merge passes move them to the end of what they consumed)
    w.rend[(size_t)lane * w.n_tiles + tile] = lane == 0 ? 0u : lane == 1 ? by0 : lane == 2 ? by0 + by1 : by0 + by1 + by2;
  if (lane < kNumClasses)
    w.tcls[(size_t)lane * w.n_tiles + tile] = lane == 0 ? n0 : lane == 1 ? n1 : lane == 2 ? n2 : n3;
  if (lane == 0 && n2) w.counters[kCtrAnyMid] = 1;  // plain stores: every writer stores 1
  if (lane == 0 && n3) w.counters[kCtrAnyC3] = 1;
  // the sparse class-3 queue (k_bpe_sparse): the tile's class-3 entries into one of kC3Shards
  // shards, its count into the shard's counter (one counter for every tile: C5 k_segment
  // 1.7 -> 5.9 ms, its atomics serialised on one address); a shard that overflows its capacity
  // keeps counting, and the report then steers the call to the register pass
  if (n3 && w.c3_max) {
    const uint32_t sh = tile & (kC3Shards - 1), cap = w.c3_max / kC3Shards;
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(&w.counters[kNumCounters + sh], n3);
    b = __builtin_amdgcn_readfirstlane(b);
    for (uint32_t j = lane; j < n3; j += 64)
      if (b + j < cap) w.c3q[(size_t)sh * cap + b + j] = (tile << 7) | j;
  }
  SEG_STAMP(5);
#ifdef CTOK_SEG_STAMPS
  if (w.stamps && lane == 0) w.stamps[(size_t)tile * 8 + 6] = np;
#endif
}

hipError_t launch_segment(const Work& w, const Tables& t, hipStream_t s, Lx x) {
  const uint32_t grid = (w.n_tiles + kSegWaves - 1) / kSegWaves;
  if (w.n_tiles && w.rec16) launch_lx(x, k_segment<true>, grid, 64 * kSegWaves, 0, s, w, t);
  else if (w.n_tiles) launch_lx(x, k_segment<false>, grid, 64 * kSegWaves, 0, s, w, t);
  return hipGetLastError();
}

}  // namespace ctok_dev
