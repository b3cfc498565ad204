// Encode path: NFC -- the quick check k_nfc_check, the normaliser k_norm, and the splice of the
// re-encoded documents k_flag_*, k_gather_flagged, k_splice_* (opening).  The
// splice helpers come first, then the check and the normaliser.
#include "dev_common.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// NFC splice (ctok_encode.cpp nfc_splice): after a speculative pass over raw text flagged code
// points NFC may change, only the documents holding them are normalised and encoded again, as a
// sub-batch, and their ids replace the speculative pass's in the output.  rank[d] = flagged docs
// before d (exclusive scan of the NFC-check flags; doc d is flagged when rank[d + 1] > rank[d]).

// flag[d] = 1 when a 64-byte word overlapping doc d holds the start of a code point NFC might
// change (k_segment's nfc_bits; a word shared with a neighbour flags both docs: a superset, and
// NFC leaves an unflagged doc unchanged, so encoding it normalised gives the same ids)
__global__ __launch_bounds__(256) void k_flag_docs(const uint64_t* __restrict__ off, uint64_t n_docs,
                                                   const uint32_t* __restrict__ bits, uint32_t* __restrict__ flag) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256) {
    const uint64_t a = off[d], b = off[d + 1];
    uint32_t f = 0;
    if (b > a) {
      const uint64_t g0 = a >> 6, g1 = (b - 1) >> 6;  // words [g0, g1]
      for (uint64_t q = g0 >> 5; q <= (g1 >> 5) && !f; q++) {
        uint32_t m = bits[q];
        if (q == (g0 >> 5)) m &= ~0u << (g0 & 31);
        if (q == (g1 >> 5)) m &= (g1 & 31) == 31 ? ~0u : (2u << (g1 & 31)) - 1u;
        f = m != 0;
      }
    }
    flag[d] = f;
  }
}

// len[d] = bytes of doc d if it is flagged, else 0 (scanned to the sub-batch offsets)
__global__ __launch_bounds__(256) void k_flag_len(const uint64_t* __restrict__ off, const uint32_t* __restrict__ flag,
                                                  uint64_t n_docs, uint64_t* __restrict__ len) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256)
    len[d] = flag[d] ? off[d + 1] - off[d] : 0;
}

// one wavefront per flagged doc: its bytes to sub_text at sub_pos[d], its start to sub_off[rank[d]]
__global__ __launch_bounds__(256) void k_gather_flagged(const uint8_t* __restrict__ text, const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ rank, const uint64_t* __restrict__ sub_pos,
                                                        uint64_t n_docs, uint8_t* __restrict__ sub_text,
                                                        uint64_t* __restrict__ sub_off) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t d = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; d < n_docs; d += ((uint64_t)gridDim.x * 256) >> 6) {
    const uint32_t r = rank[d];
    if (rank[d + 1] == r) continue;  // (wave-uniform)
    const uint64_t a = off[d], n = off[d + 1] - a, p = sub_pos[d];
    if (lane == 0) sub_off[r] = p;
    for (uint64_t i = lane; i < n; i += 64) sub_text[p + i] = text[a + i];
  }
}

// cnt[d] = ids of doc d in the spliced output: the sub-batch's for a flagged doc, else the
// speculative pass's (scanned in place to the output tok_off)
__global__ __launch_bounds__(256) void k_splice_count(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ main_off,
                                                      const uint64_t* __restrict__ sub_off, uint64_t n_docs,
                                                      uint64_t* __restrict__ cnt) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256) {
    const uint32_t r = rank[d];
    cnt[d] = rank[d + 1] != r ? sub_off[r + 1] - sub_off[r] : main_off[d + 1] - main_off[d];
  }
}

// one wavefront per doc: its ids from the sub-batch or the speculative pass to out_off[d]
__global__ __launch_bounds__(256) void k_splice_copy(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ main_off,
                                                     const uint32_t* __restrict__ main_ids, const uint64_t* __restrict__ sub_off,
                                                     const uint32_t* __restrict__ sub_ids, const uint64_t* __restrict__ out_off,
                                                     uint64_t n_docs, uint32_t* __restrict__ ids, uint64_t ids_cap) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t d = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; d < n_docs; d += ((uint64_t)gridDim.x * 256) >> 6) {
    const uint32_t r = rank[d];
    const bool f = rank[d + 1] != r;
    const uint32_t* src = f ? sub_ids + sub_off[r] : main_ids + main_off[d];
    const uint64_t o = out_off[d], n = out_off[d + 1] - o;
    for (uint64_t i = lane; i < n; i += 64)
      if (o + i < ids_cap) ids[o + i] = src[i];
  }
}

hipError_t launch_flag_docs(const uint64_t* off, uint64_t n_docs, const uint32_t* nfc_bits, uint32_t* flag, hipStream_t s) {
  if (!n_docs) return hipSuccess;
  k_flag_docs<<<grid_for(n_docs), 256, 0, s>>>(off, n_docs, nfc_bits, flag);
  return hipGetLastError();
}

hipError_t launch_flag_len(const uint64_t* off, const uint32_t* flag, uint64_t n_docs, uint64_t* len, hipStream_t s) {
  if (!n_docs) return hipSuccess;
  k_flag_len<<<grid_for(n_docs), 256, 0, s>>>(off, flag, n_docs, len);
  return hipGetLastError();
}

hipError_t launch_gather_flagged(const uint8_t* text, const uint64_t* off, const uint32_t* rank, const uint64_t* sub_pos,
                                 uint64_t n_docs, uint8_t* sub_text, uint64_t* sub_off, hipStream_t s) {
  if (!n_docs) return hipSuccess;
  k_gather_flagged<<<grid_for(64 * n_docs, 1u << 20), 256, 0, s>>>(text, off, rank, sub_pos, n_docs, sub_text, sub_off);
  return hipGetLastError();
}

hipError_t launch_splice(const uint32_t* rank, const uint64_t* main_off, const uint32_t* main_ids, const uint64_t* sub_off,
                         const uint32_t* sub_ids, uint64_t n_docs, uint32_t* ids, uint64_t ids_cap, uint64_t* out_off,
                         uint64_t* tmp, uint64_t tmp_cap, hipStream_t s) {
  if (!n_docs) return hipSuccess;
  k_splice_count<<<grid_for(n_docs), 256, 0, s>>>(rank, main_off, sub_off, n_docs, out_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = scan_u64(out_off, n_docs, tmp, tmp_cap, s);
  if (e != hipSuccess) return e;
  k_splice_copy<<<grid_for(64 * n_docs, 1u << 20), 256, 0, s>>>(rank, main_off, main_ids, sub_off, sub_ids, out_off, n_docs, ids, ids_cap);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// NFC (src/normalizers.rs:47): quick check per chunk, exact normalisation per flagged doc.


__device__ __forceinline__ int dev_decode(const uint8_t* s, uint32_t n, uint32_t i, uint32_t* cp) {
  const uint8_t b = s[i];
  if (b < 0x80) { *cp = b; return 1; }
  const int len = u8len(b);
  if (i + len > n) { *cp = 0xFFFD; return 1; }
  if (len == 2) *cp = ((b & 0x1Fu) << 6) | (s[i + 1] & 0x3Fu);
  else if (len == 3) *cp = ((b & 0x0Fu) << 12) | ((s[i + 1] & 0x3Fu) << 6) | (s[i + 2] & 0x3Fu);
  else *cp = ((b & 0x07u) << 18) | ((s[i + 1] & 0x3Fu) << 12) | ((s[i + 2] & 0x3Fu) << 6) | (s[i + 3] & 0x3Fu);
  return len;
}

// one thread per 64-byte chunk; a doc is flagged when it holds any code point with
// NFC_QC != Yes or a non-zero combining class (a superset of the docs NFC changes)
__global__ void k_nfc_check(const uint8_t* __restrict__ text, uint64_t n_bytes, const uint64_t* __restrict__ off,
                            uint32_t n_docs, Tables t, uint32_t* doc_flag, uint32_t* counter) {
  const uint64_t c0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 64;
  if (c0 >= n_bytes) return;
  const uint64_t c1 = c0 + 64 < n_bytes ? c0 + 64 : n_bytes;
  bool ascii = true;
  if (c1 - c0 == 64) {
    const uint4* v = reinterpret_cast<const uint4*>(text + c0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint4 x = v[k];
      if ((x.x | x.y | x.z | x.w) & 0x80808080u) ascii = false;
    }
  } else {
    for (uint64_t i = c0; i < c1; i++) if (text[i] & 0x80) ascii = false;
  }
  if (ascii) return;
  for (uint64_t i = c0; i < c1;) {
    const uint8_t b = text[i];
    if ((b & 0xC0) == 0x80) { i++; continue; }
    uint32_t cp;
    const int len = dev_decode(text, (uint32_t)(n_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : n_bytes), (uint32_t)i, &cp);
    const uint16_t f = nfc16(t, cp);
    if (f != 0) {
      // doc of byte i: last d with off[d] <= i and off[d+1] > i
      uint32_t lo = 0, hi = n_docs;  // invariant off[lo] <= i < off[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
      }
      if (atomicOr(&doc_flag[lo], 1u) == 0u) atomicAdd(counter, 1u);
    }
    i += len;
  }
}

hipError_t launch_nfc_check(const uint8_t* text, uint64_t n_bytes, const uint64_t* doc_off, uint32_t n_docs,
                            const Tables& t, uint32_t* doc_flag, uint32_t* counter, hipStream_t s) {
  const uint64_t chunks = (n_bytes + 63) / 64;
  if (chunks) k_nfc_check<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(text, n_bytes, doc_off, n_docs, t, doc_flag, counter);
  return hipGetLastError();
}

#define SBASE 0xAC00u
#define LBASE 0x1100u
#define VBASE 0x1161u
#define TBASE 0x11A7u
#define LCOUNT 19u
#define VCOUNT 21u
#define TCOUNT 28u
#define NCOUNT (VCOUNT * TCOUNT)
#define SCOUNT (LCOUNT * NCOUNT)

__device__ int nfc_decompose(const Tables& t, uint32_t cp, uint32_t* o) {
  if (cp >= SBASE && cp < SBASE + SCOUNT) {
    const uint32_t s = cp - SBASE;
    o[0] = LBASE + s / NCOUNT;
    o[1] = VBASE + (s % NCOUNT) / TCOUNT;
    if (s % TCOUNT) { o[2] = TBASE + s % TCOUNT; return 3; }
    return 2;
  }
  int lo = 0, hi = (int)t.n_decomp - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t c = t.decomp_cp[mid];
    if (c == cp) {
      int k = 0;
      for (uint32_t j = t.decomp_off[mid]; j < t.decomp_off[mid + 1]; j++) o[k++] = t.decomp_data[j];
      return k;
    }
    if (c < cp) lo = mid + 1; else hi = mid - 1;
  }
  o[0] = cp;
  return 1;
}

__device__ uint32_t nfc_compose(const Tables& t, uint32_t a, uint32_t b) {
  if (a >= LBASE && a < LBASE + LCOUNT && b >= VBASE && b < VBASE + VCOUNT)
    return SBASE + ((a - LBASE) * VCOUNT + (b - VBASE)) * TCOUNT;
  if (a >= SBASE && a < SBASE + SCOUNT && (a - SBASE) % TCOUNT == 0 && b > TBASE && b < TBASE + TCOUNT)
    return a + (b - TBASE);
  const uint64_t key = ((uint64_t)a << 21) | b;
  int lo = 0, hi = (int)t.n_comp - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const uint64_t k = t.comp_key[mid];
    if (k == key) return t.comp_val[mid];
    if (k < key) lo = mid + 1; else hi = mid - 1;
  }
  return kNone;
}

// canonical ordering (stable by combining class) then canonical composition of buf[0, k) in place
// (UAX #15); returns the new count
__device__ uint32_t nfc_reorder_compose(const Tables& t, uint32_t* buf, uint32_t k) {
  for (uint32_t i = 1; i < k; i++) {
    const uint32_t c = buf[i];
    const int cc = nfc16(t, c) & 0xFF;
    if (!cc) continue;
    uint32_t j = i;
    while (j > 0) {
      const int pc = nfc16(t, buf[j - 1]) & 0xFF;
      if (pc <= cc || pc == 0) break;
      buf[j] = buf[j - 1];
      j--;
    }
    buf[j] = c;
  }
  if (k == 0) return 0;
  uint32_t starter = 0, comp = 1, sch = buf[0];
  int last = nfc16(t, sch) & 0xFF;
  if (last) last = 256;
  for (uint32_t i = 1; i < k; i++) {
    const uint32_t ch = buf[i];
    const int cc = nfc16(t, ch) & 0xFF;
    const uint32_t c = nfc_compose(t, sch, ch);
    if (c != kNone && (last < cc || last == 0)) { buf[starter] = c; sch = c; continue; }
    if (cc == 0) { starter = comp; sch = ch; }
    last = cc;
    buf[comp++] = ch;
  }
  return comp;
}

__device__ __forceinline__ uint32_t u8size(uint32_t cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }

// NFC of s[0, n) into buf (capacity 4n code points) by one wavefront; returns the code point
// count, *len_out its UTF-8 bytes, *first_out the first code point (0 if none).  A code point
// with nfc16 == 0 (ccc 0 and NFC_QC Yes) is a normalisation boundary: nothing after it combines
// with anything before it, and it is unchanged unless a following code point combines with it.
// So only the segments around unstable code points are normalised -- from the boundary before
// the first (popped back from the output) to the next boundary -- and everything else is copied.
// The wave walks the document in 64-byte windows: every lane decodes the code point starting at
// its byte and looks up its nfc16 (one round of loads per window instead of one per code point),
// the stable code points before the window's first unstable one are appended together, and lane
// 0 normalises the segment there (decomposition / composition table searches for a few code
// points).  Segment workspace in buf[2n ..).
__device__ uint32_t nfc_doc(const Tables& t, const uint8_t* s, uint32_t n, uint32_t* buf, uint64_t* len_out,
                            uint32_t* first_out) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t* tmp = buf + 2 * (size_t)n;
  uint32_t k = 0, first = 0, last = 0;  // wave-uniform: output count, first / last output code point
  uint64_t len = 0;
  bool lb = false;  // the last output code point is a boundary copied through
  for (uint32_t i = 0; i < n;) {
    const uint32_t p = i + lane;
    uint32_t cp = 0;
    bool st = false, un = false;
    if (p < n) {
      st = (s[p] & 0xC0) != 0x80;
      if (st) {
        dev_decode(s, n, p, &cp);
        un = nfc16(t, cp) != 0;
      }
    }
    const uint64_t S = __ballot(st), U = __ballot(st && un);
    const uint64_t keep = U ? S & ((1ull << __builtin_ctzll(U)) - 1ull) : S;  // stable, before the first unstable
    const bool mine = (keep >> lane) & 1ull;
    if (mine) buf[k + __popcll(keep & lanemask_lt())] = cp;
    if (keep) {
      if (k == 0) first = __builtin_amdgcn_readlane(cp, __builtin_ctzll(keep));
      last = __builtin_amdgcn_readlane(cp, 63 - __builtin_clzll(keep));
      k += (uint32_t)__popcll(keep);
      len += wave_sum_full_u32(mine ? u8size(cp) : 0u);  // (phase 1 writes u8size bytes per code point)
      lb = true;
    }
    if (!U) {
      i += 64;
      continue;
    }
    uint32_t j = i + (uint32_t)__builtin_ctzll(U);
    if (lane == 0) {
      uint32_t m = 0;
      if (lb) {  // the boundary before joins the segment
        k--;
        len -= u8size(last);
        m = nfc_decompose(t, last, tmp);
      }
      while (j < n) {
        uint32_t c;
        const int ll = dev_decode(s, n, j, &c);
        if (nfc16(t, c) == 0) break;  // the next boundary ends the segment
        m += nfc_decompose(t, c, tmp + m);
        j += ll;
      }
      m = nfc_reorder_compose(t, tmp, m);
      if (k == 0 && m) first = tmp[0];
      for (uint32_t q = 0; q < m; q++) {
        buf[k++] = tmp[q];
        len += u8size(tmp[q]);
      }
      if (m) last = tmp[m - 1];
    }
    k = __builtin_amdgcn_readlane(k, 0);
    j = __builtin_amdgcn_readlane(j, 0);
    first = __builtin_amdgcn_readlane(first, 0);
    last = __builtin_amdgcn_readlane(last, 0);
    len = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(len >> 32), 0) << 32) | __builtin_amdgcn_readlane((uint32_t)len, 0);
    lb = false;
    i = j;
  }
  *len_out = len;
  *first_out = k ? first : 0u;
  return k;
}


// phase 0: new_len[d] = normalised length (flagged docs: NFC code points left in cp_scratch)
// phase 1: write the normalised text at new_off[d] (new_len scanned into offsets)
// Normalisation (NFC of the flagged documents, optional prefix space), a wavefront per
// document: phase 0 sizes each output document, phase 1 (after a scan) writes it.  An unflagged
// document is copied by the whole wave (consecutive lanes, consecutive bytes); a flagged one is
// normalised by the wave (nfc_doc) into code points, which phase 1 writes as UTF-8.
constexpr int kNormWaves = 4;

__global__ __launch_bounds__(64 * kNormWaves) void k_norm(const uint8_t* __restrict__ text,
                                                          const uint64_t* __restrict__ off, uint32_t n_docs,
                                                          const uint32_t* __restrict__ doc_flag, int add_prefix,
                                                          int nfc, Tables t, uint32_t* cp_scratch, uint32_t* ncp,
                                                          uint64_t* newv, uint8_t* out, int phase) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t d = uni(blockIdx.x * kNormWaves + (threadIdx.x >> 6));
  if (d >= n_docs) return;
  const uint64_t a = off[d];
  const uint32_t n = (uint32_t)(off[d + 1] - a);
  const bool flagged = nfc && uni(doc_flag[d]) != 0;
  uint32_t* buf = cp_scratch + 4 * a;
  if (phase == 0) {
    uint64_t len;
    uint32_t first;
    if (flagged) {
      const uint32_t k = nfc_doc(t, text + a, n, buf, &len, &first);
      if (lane == 0) ncp[d] = k;
    } else {
      len = n;
      first = n ? text[a] : 0;
    }
    if (add_prefix && len > 0 && first != ' ') len += 1;  // src/pretokenizers.rs:163-167
    if (lane == 0) newv[d] = len;
    return;
  }
  uint8_t* o = out + newv[d];
  if (flagged) {  // the code points as UTF-8: a wave scan of their sizes places each lane's bytes
    const uint32_t k = ncp[d];
    const uint32_t pre = (add_prefix && k > 0 && buf[0] != ' ') ? 1u : 0u;
    if (pre && lane == 0) o[0] = ' ';
    uint64_t pos = pre;
    for (uint32_t q0 = 0; q0 < k; q0 += 64) {
      const uint32_t q = q0 + lane;
      const uint32_t c = q < k ? buf[q] : 0u, sz = q < k ? u8size(c) : 0u;
      const uint32_t inc = wave_incl_scan(sz);
      uint8_t* w8 = o + pos + (inc - sz);
      if (sz == 1) {
        w8[0] = (uint8_t)c;
      } else if (sz == 2) {
        w8[0] = (uint8_t)(0xC0 | (c >> 6)); w8[1] = (uint8_t)(0x80 | (c & 0x3F));
      } else if (sz == 3) {
        w8[0] = (uint8_t)(0xE0 | (c >> 12)); w8[1] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); w8[2] = (uint8_t)(0x80 | (c & 0x3F));
      } else if (sz == 4) {
        w8[0] = (uint8_t)(0xF0 | (c >> 18)); w8[1] = (uint8_t)(0x80 | ((c >> 12) & 0x3F));
        w8[2] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); w8[3] = (uint8_t)(0x80 | (c & 0x3F));
      }
      pos += lane63(inc);
    }
    return;
  }
  const uint32_t pre = (add_prefix && n > 0 && text[a] != ' ') ? 1u : 0u;
  if (pre && lane == 0) o[0] = ' ';
  for (uint32_t i = lane; i < n; i += 64) o[pre + i] = text[a + i];
}

hipError_t launch_norm(const uint8_t* text, const uint64_t* doc_off, uint32_t n_docs, const uint32_t* doc_flag,
                       int add_prefix, int nfc, const Tables& t, uint32_t* cp_scratch, uint32_t* ncp,
                       uint64_t* newv, uint8_t* out, int phase, hipStream_t s) {
  if (n_docs)
    k_norm<<<(n_docs + kNormWaves - 1) / kNormWaves, 64 * kNormWaves, 0, s>>>(text, doc_off, n_docs, doc_flag, add_prefix,
                                                                          nfc, t, cp_scratch, ncp, newv, out, phase);
  return hipGetLastError();
}

void upload_done() {}

}  // namespace ctok_dev
