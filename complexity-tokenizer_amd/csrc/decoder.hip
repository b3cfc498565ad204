// HIP kernels (gfx950) of the Decoder (decoder_hd.h: the reference's src/decoders.rs:30-243).
//
// Every op has one shape.  A thread owns one unit -- a byte of the documents' concatenation for the
// text rules, a token for WordPiece, BPE and CTC -- and finds its document by a binary search of the
// documents' offsets.  k_dc_units<false> sums what a workgroup's 256 units emit (unit_emit with no
// output), the host scans the workgroups' sums (scan_u64) and refuses 4 GiB, and k_dc_units<true>
// counts again, scans inside the workgroup and writes every unit's bytes at its place; the documents
// that start in the workgroup's tile get their new offsets from the same prefix.  The place behind the
// last unit is a unit that emits nothing, so the documents that start there have a workgroup too.
// What a unit cannot decide from its neighbourhood a kernel makes before: the kept range of a document
// (k_dc_range: Strip, trim_end), the first token that contributes to a WordPiece document
// (k_dc_wp_first), the literal matches (k_dc_cand marks candidates, k_dc_chain walks chains of
// overlapping ones from their first) and the spaces the clean-up deletes (k_dc_runs replays the eight
// passes on every run of set bytes from its first byte).  The ids entry gathers first: k_dc_keep flags
// the ids that have an entry, k_dc_len places their lengths, k_dc_gather copies their bytes.
// No kernel waits on another workgroup; within a kernel no thread reads what another writes; every
// loop is bounded by its document's, token's or pattern's length.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_common.h"  // ctok_dev::block_excl_scan
#include "decoder_hd.h"
#include "decoder_internal.h"

namespace ctok_dc {

using decoder::In;
using decoder::Step;

#define DC_CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

static uint32_t grid_for(uint64_t n_threads, uint32_t max_grid = 1u << 18) {
  const uint64_t g = (n_threads + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}
__device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }
__device__ __forceinline__ uint64_t gstride() { return (uint64_t)gridDim.x * kThreads; }

// ---- the batch's shape ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_dc_check(const uint64_t* tok_off, uint64_t n_tok, uint64_t n_bytes,
                                                       const uint64_t* doc_tok, uint64_t n_docs, uint32_t* flag) {
  const uint64_t top = n_tok > n_docs ? n_tok : n_docs;
  bool bad = false;
  for (uint64_t i = gid(); i <= top; i += gstride()) {
    if (i <= n_tok) {
      const uint64_t o = tok_off[i];
      bad |= (i == 0 && o != 0) || (i == n_tok && o != n_bytes) || o > n_bytes || (i < n_tok && tok_off[i + 1] < o);
    }
    if (i <= n_docs) {
      const uint64_t o = doc_tok[i];
      bad |= (i == 0 && o != 0) || (i == n_docs && o != n_tok) || o > n_tok || (i < n_docs && doc_tok[i + 1] < o);
    }
  }
  if (bad) atomicOr(flag, 1u);
}

hipError_t launch_check(const uint64_t* tok_off, uint64_t n_tok, uint64_t n_bytes, const uint64_t* doc_tok, uint64_t n_docs,
                        uint32_t* flag, hipStream_t s) {
  DC_CHK(hipMemsetAsync(flag, 0, 4, s));
  k_dc_check<<<grid_for((n_tok > n_docs ? n_tok : n_docs) + 1), kThreads, 0, s>>>(tok_off, n_tok, n_bytes, doc_tok, n_docs, flag);
  return hipGetLastError();
}

__global__ __launch_bounds__(kThreads) void k_dc_doc_off(const uint64_t* tok_off, const uint64_t* doc_tok, uint64_t n_docs,
                                                         uint64_t* doc_off) {
  for (uint64_t d = gid(); d <= n_docs; d += gstride()) doc_off[d] = tok_off[doc_tok[d]];
}

hipError_t launch_doc_off(const uint64_t* tok_off, const uint64_t* doc_tok, uint64_t n_docs, uint64_t* doc_off, hipStream_t s) {
  k_dc_doc_off<<<grid_for(n_docs + 1), kThreads, 0, s>>>(tok_off, doc_tok, n_docs, doc_off);
  return hipGetLastError();
}

__global__ __launch_bounds__(kThreads) void k_dc_iota(uint64_t* p, uint64_t n) {
  for (uint64_t i = gid(); i <= n; i += gstride()) p[i] = i;
}

hipError_t launch_iota(uint64_t* p, uint64_t n, hipStream_t s) {
  k_dc_iota<<<grid_for(n + 1), kThreads, 0, s>>>(p, n);
  return hipGetLastError();
}

// ---- preparation ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_dc_range(uint32_t prep, Step st, uint64_t start, uint64_t stop, In in, uint64_t* lo,
                                                       uint64_t* hi) {
  for (uint64_t d = gid(); d < in.n_docs; d += gstride()) {
    const uint64_t ds = in.doc_off[d], de = in.doc_off[d + 1];
    if (prep == decoder::P_STRIP) decoder::strip_range(in.bytes, st.a, st.a_len, start, stop, ds, de, &lo[d], &hi[d]);
    else decoder::trim_range(in.bytes, ds, de, &lo[d], &hi[d]);
  }
}

__global__ __launch_bounds__(kThreads) void k_dc_wp_first(Step st, In in, uint64_t* first) {
  for (uint64_t d = gid(); d < in.n_docs; d += gstride()) first[d] = decoder::wp_first(st, in, d);
}

__global__ __launch_bounds__(kThreads) void k_dc_cand(Step st, In in, uint8_t* cand) {
  for (uint64_t p = gid(); p < in.n; p += gstride()) {
    const uint64_t d = decoder::doc_of(in.doc_off, in.n_docs, p);
    cand[p] = decoder::rep_cand(st, in.bytes, in.doc_off[d + 1], p);
  }
}

__global__ __launch_bounds__(kThreads) void k_dc_chain(Step st, In in, const uint8_t* cand, uint8_t* mark) {
  for (uint64_t p = gid(); p < in.n; p += gstride()) {
    if (!cand[p]) continue;
    const uint64_t d = decoder::doc_of(in.doc_off, in.n_docs, p);
    decoder::rep_chain(st, cand, mark, in.doc_off[d], in.doc_off[d + 1], p);
  }
}

__global__ __launch_bounds__(kThreads) void k_dc_runs(In in, uint8_t* mark) {
  for (uint64_t p = gid(); p < in.n; p += gstride()) {
    if (!decoder::is_set_byte(in.bytes[p])) continue;
    const uint64_t d = decoder::doc_of(in.doc_off, in.n_docs, p);
    decoder::cleanup_run(in.bytes, mark, in.doc_off[d], in.doc_off[d + 1], p);
  }
}

hipError_t launch_prep(uint32_t prep, const Step& st, uint64_t start, uint64_t stop, const In& in, const Scratch& sc,
                       hipStream_t s) {
  switch (prep) {
    case decoder::P_STRIP:
    case decoder::P_TRIM:
      if (in.n_docs) k_dc_range<<<grid_for(in.n_docs), kThreads, 0, s>>>(prep, st, start, stop, in, sc.lo, sc.hi);
      return hipGetLastError();
    case decoder::P_WP_FIRST:
      if (in.n_docs) k_dc_wp_first<<<grid_for(in.n_docs), kThreads, 0, s>>>(st, in, sc.first);
      return hipGetLastError();
    case decoder::P_REPLACE:
      if (!in.n) return hipSuccess;
      DC_CHK(hipMemsetAsync(sc.mark, 0, in.n, s));
      k_dc_cand<<<grid_for(in.n), kThreads, 0, s>>>(st, in, sc.cand);
      DC_CHK(hipGetLastError());
      k_dc_chain<<<grid_for(in.n), kThreads, 0, s>>>(st, in, sc.cand, sc.mark);
      return hipGetLastError();
    case decoder::P_CLEANUP:
      if (!in.n) return hipSuccess;
      DC_CHK(hipMemsetAsync(sc.mark, 0, in.n, s));
      k_dc_runs<<<grid_for(in.n), kThreads, 0, s>>>(in, sc.mark);
      return hipGetLastError();
    default:
      return hipSuccess;
  }
}

// ---- count and write --------------------------------------------------------------------------------------

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_dc_units(Step st, In in, uint64_t* cnt_out, const uint64_t* pos, uint8_t* out,
                                                       uint64_t* out_off) {
  __shared__ uint64_t s_scan[17];
  __shared__ uint64_t s_pre[kWrite ? kThreads : 1];
  __shared__ uint64_t s_d0;
  const uint64_t nu = decoder::n_units(st, in);
  const uint64_t* uoff = decoder::unit_off(st, in);
  const uint64_t bs = (uint64_t)blockIdx.x * kThreads, u = bs + threadIdx.x;
  uint64_t d = 0, cnt = 0;
  if (u < nu) {
    d = decoder::doc_of(uoff, in.n_docs, u);
    cnt = decoder::unit_emit(st, in, d, u, nullptr);
  }
  uint64_t total;
  const uint64_t ex = ctok_dev::block_excl_scan<uint64_t>(cnt, s_scan, &total);
  if (!kWrite) {
    if (threadIdx.x == 0) cnt_out[blockIdx.x] = total;
    return;
  }
  const uint64_t base = pos[blockIdx.x], tail = decoder::tail_len(st);
  if (cnt) decoder::unit_emit(st, in, d, u, out + base + ex + d * tail);
  s_pre[threadIdx.x] = ex;
  if (threadIdx.x == 0) s_d0 = decoder::first_doc_from(uoff, in.n_docs, bs);
  __syncthreads();
  // the documents that start in this tile (the place behind the last unit belongs to the last tile)
  for (uint64_t dd = s_d0 + threadIdx.x; dd <= in.n_docs; dd += kThreads) {
    const uint64_t o = uoff[dd];
    if (o >= bs + kThreads) break;
    out_off[dd] = base + s_pre[o - bs] + dd * tail;
  }
}

// the tail every document gets (OP_INSERT): the replacement behind its text
__global__ __launch_bounds__(kThreads) void k_dc_tail(Step st, uint64_t n_docs, const uint64_t* out_off, uint8_t* out) {
  for (uint64_t d = gid(); d < n_docs; d += gstride()) decoder::put(out + out_off[d + 1] - st.b_len, st.b, st.b_len);
}

hipError_t launch_count(const Step& st, const In& in, uint64_t* blk, hipStream_t s) {
  k_dc_units<false><<<(uint32_t)unit_blocks(decoder::n_units(st, in)), kThreads, 0, s>>>(st, in, blk, nullptr, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t launch_write(const Step& st, const In& in, const uint64_t* blk, uint8_t* out, uint64_t* out_off, hipStream_t s) {
  k_dc_units<true><<<(uint32_t)unit_blocks(decoder::n_units(st, in)), kThreads, 0, s>>>(st, in, nullptr, blk, out, out_off);
  DC_CHK(hipGetLastError());
  if (decoder::tail_len(st) && in.n_docs) {
    k_dc_tail<<<grid_for(in.n_docs), kThreads, 0, s>>>(st, in.n_docs, out_off, out);
    return hipGetLastError();
  }
  return hipSuccess;
}

// ---- the gather of the ids entry --------------------------------------------------------------------------

__device__ __forceinline__ uint2 ent_of(const uint2* ent, uint64_t n_ent, uint32_t id) {
  return id < n_ent ? ent[id] : make_uint2(0u, 0xFFFFFFFFu);
}

__global__ __launch_bounds__(kThreads) void k_dc_keep(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent,
                                                      uint64_t* keep) {
  for (uint64_t j = gid(); j < n_ids; j += gstride()) keep[j] = ent_of(ent, n_ent, ids[j]).y != 0xFFFFFFFFu ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_dc_len(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent,
                                                     const uint64_t* pos, const uint64_t* ids_off, uint64_t n_docs, uint64_t* len,
                                                     uint64_t* doc_tok) {
  const uint64_t top = n_ids > n_docs + 1 ? n_ids : n_docs + 1;
  for (uint64_t j = gid(); j < top; j += gstride()) {
    if (j < n_ids) {
      const uint2 e = ent_of(ent, n_ent, ids[j]);
      if (e.y != 0xFFFFFFFFu) len[pos[j]] = e.y;
    }
    if (j <= n_docs) doc_tok[j] = pos[ids_off[j]];
  }
}

__global__ __launch_bounds__(kThreads) void k_dc_gather(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent,
                                                        const uint8_t* pool, const uint64_t* pos, const uint64_t* tok_off,
                                                        uint8_t* out) {
  for (uint64_t j = gid(); j < n_ids; j += gstride()) {
    const uint2 e = ent_of(ent, n_ent, ids[j]);
    if (e.y == 0xFFFFFFFFu) continue;
    decoder::put(out + tok_off[pos[j]], pool + e.x, e.y);
  }
}

hipError_t launch_gather_keep(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, uint64_t* keep, hipStream_t s) {
  if (n_ids) k_dc_keep<<<grid_for(n_ids), kThreads, 0, s>>>(ids, n_ids, ent, n_ent, keep);
  return hipGetLastError();
}

hipError_t launch_gather_len(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, const uint64_t* pos,
                             const uint64_t* ids_off, uint64_t n_docs, uint64_t* len, uint64_t* doc_tok, hipStream_t s) {
  k_dc_len<<<grid_for(n_ids > n_docs + 1 ? n_ids : n_docs + 1), kThreads, 0, s>>>(ids, n_ids, ent, n_ent, pos, ids_off, n_docs, len,
                                                                                  doc_tok);
  return hipGetLastError();
}

hipError_t launch_gather_write(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, const uint8_t* pool,
                               const uint64_t* pos, const uint64_t* tok_off, uint8_t* out, hipStream_t s) {
  if (n_ids) k_dc_gather<<<grid_for(n_ids), kThreads, 0, s>>>(ids, n_ids, ent, n_ent, pool, pos, tok_off, out);
  return hipGetLastError();
}

}  // namespace ctok_dc
