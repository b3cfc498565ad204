// HIP kernels (gfx950) of the PostProcessor (postproc_hd.h: the reference's src/postprocessors.rs:34-280).
//
// One shape: count, scan, refuse, write.  k_pp_count has a thread per row: it reads the row's two
// lengths and its has_pair, truncates in closed form and gives the row's processed length from the
// totals of its flat list; a wave maximum feeds the batch's longest row.  The host scans the lengths
// (scan_u64), reads the total and the longest row back and refuses 2^32 ids before anything is
// written.  The write kernels have a thread per output cell, consecutive lanes on consecutive cells:
// the cell finds its item by a binary search over the list's prefix tables, which a workgroup stages
// into LDS once and keeps over all the tiles it takes, then gathers one id and stores it.  The matrix
// form finds the row by a division, the ragged form by a search over the scanned offsets: a workgroup
// takes a run of consecutive tiles, two of its lanes find the rows of the run's first and last cell,
// and every thread searches between them, from the row of its last cell on.  No kernel waits on
// another workgroup; within a kernel no thread reads what another writes; every loop is a binary
// search or a stride over the grid.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "postproc_hd.h"
#include "postproc_internal.h"

namespace ctok_pp {

using postproc::Cell;
using postproc::In;
using postproc::List;
using postproc::Opts;
using postproc::Row;

#define PP_CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

constexpr uint32_t kMaxGrid = 2048;  // workgroups of a write kernel: each stages the tables once

static uint32_t grid_for(uint64_t n_threads, uint32_t max_grid) {
  const uint64_t g = (n_threads + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}
__device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }
__device__ __forceinline__ uint64_t gstride() { return (uint64_t)gridDim.x * kThreads; }

// ---- count ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_pp_count(In in, Opts o, DevProgram p, Row* __restrict__ rows, uint64_t* __restrict__ off,
                                                       uint64_t* meta) {
  bool bad = false;
  uint64_t longest = 0;
  for (uint64_t r = gid(); r < in.n_rows; r += gstride()) {
    Row row;
    const uint64_t len = postproc::count_row(in, o, p.single, p.pair, r, &row, &bad);
    rows[r] = row;
    off[r] = len;
    longest = len > longest ? len : longest;
  }
  // the wave's maximum, one atomic per wave that has a row
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t other = __shfl_xor((unsigned long long)longest, d, 64);
    longest = other > longest ? other : longest;
  }
  if ((threadIdx.x & 63) == 0 && longest) atomicMax((unsigned long long*)&meta[kMetaLongest], (unsigned long long)longest);
  if (bad) atomicOr((unsigned long long*)&meta[kMetaBad], 1ull);
}

hipError_t launch_count(const In& in, const Opts& o, const DevProgram& p, Row* rows, uint64_t* off, uint64_t* meta, hipStream_t s) {
  PP_CHK(hipMemsetAsync(meta, 0, kMetaN * sizeof(uint64_t), s));
  if (!in.n_rows) return hipMemsetAsync(off, 0, sizeof(uint64_t), s);
  k_pp_count<<<grid_for(in.n_rows, 1u << 16), kThreads, 0, s>>>(in, o, p, rows, off, meta);
  return hipGetLastError();
}

// ---- write ------------------------------------------------------------------------------------------------

// Both lists' prefix tables into the workgroup's LDS (6 bytes an entry, at most 2 * 4097 entries); the
// SPECIAL ids stay where they are, a cell reads at most one.
static size_t staged_bytes(const DevProgram& p) { return (size_t)(p.single.n + 1 + p.pair.n + 1) * 3 * sizeof(uint16_t); }

__device__ __forceinline__ void stage(const DevProgram& p, uint16_t* s_tab, List* single, List* pair) {
  const uint32_t n0 = p.single.n + 1, n1 = p.pair.n + 1;
  for (uint32_t i = threadIdx.x; i < n0; i += kThreads) {
    s_tab[i] = p.single.pa[i];
    s_tab[n0 + i] = p.single.pb[i];
    s_tab[2 * n0 + i] = p.single.ps[i];
  }
  uint16_t* t1 = s_tab + 3 * n0;
  for (uint32_t i = threadIdx.x; i < n1; i += kThreads) {
    t1[i] = p.pair.pa[i];
    t1[n1 + i] = p.pair.pb[i];
    t1[2 * n1 + i] = p.pair.ps[i];
  }
  *single = List{s_tab, s_tab + n0, s_tab + 2 * n0, p.single.val, p.single.n};
  *pair = List{t1, t1 + n1, t1 + 2 * n1, p.pair.val, p.pair.n};
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_pp_write_ragged(In in, DevProgram p, const Row* __restrict__ rows,
                                                              const uint64_t* __restrict__ off, uint64_t total,
                                                              uint32_t* __restrict__ out) {
  extern __shared__ uint16_t s_tab[];
  __shared__ uint64_t s_row[2];
  // a workgroup takes a run of consecutive tiles, so that the rows of its cells are one short range
  const uint64_t n_tiles = (total + kThreads - 1) / kThreads, per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const uint64_t t0 = blockIdx.x * per, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
  if (t0 >= t1) return;  // (the whole workgroup)
  List single, pair;
  stage(p, s_tab, &single, &pair);
  const uint64_t c_first = t0 * kThreads, c_last = (t1 * kThreads < total ? t1 * kThreads : total) - 1;
  // the rows of the run's first and last cell, by one lane each of two waves
  if (threadIdx.x == 0) s_row[0] = postproc::find_row(off, 0, in.n_rows - 1, c_first);
  if (threadIdx.x == 64) s_row[1] = postproc::find_row(off, 0, in.n_rows - 1, c_last);
  __syncthreads();
  uint64_t r = s_row[0];
  const uint64_t r_hi = s_row[1];
  for (uint64_t c = c_first + threadIdx.x; c <= c_last; c += kThreads) {
    r = postproc::find_row(off, r, r_hi, c);  // (a thread's cells go up, so its rows do)
    const Row row = rows[r];
    const List& l = postproc::row_has_pair(in, r) ? pair : single;
    const Cell cell = postproc::cell_of(l, row.na, row.nb, c - off[r]);
    __builtin_nontemporal_store(postproc::cell_id(in, r, cell), &out[c]);
  }
}

hipError_t launch_write_ragged(const In& in, const DevProgram& p, const Row* rows, const uint64_t* off, uint64_t total, uint32_t* out,
                               hipStream_t s) {
  if (!total) return hipSuccess;
  k_pp_write_ragged<<<grid_for(total, kMaxGrid), kThreads, staged_bytes(p), s>>>(in, p, rows, off, total, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(kThreads) void k_pp_write_matrix(In in, Opts o, DevProgram p, const Row* __restrict__ rows,
                                                              const uint64_t* __restrict__ off, Matrix m) {
  extern __shared__ uint16_t s_tab[];
  List single, pair;
  stage(p, s_tab, &single, &pair);
  for (uint64_t r = gid(); r < in.n_rows; r += gstride()) m.row_len[r] = (uint32_t)(off[r + 1] - off[r]);
  const uint32_t width = (uint32_t)m.width;
  const uint64_t cells = in.n_rows * m.width;  // below 2^32
  for (uint64_t c = gid(); c < cells; c += gstride()) {
    const uint32_t r = (uint32_t)c / width, col = (uint32_t)c - r * width;
    const uint64_t o0 = off[r], len = off[r + 1] - o0;
    const uint64_t j = postproc::matrix_cell(width, len, o.pad_left != 0, col);
    uint32_t id = o.pad_id, attention = 0, type = 0, special = 1;
    if (j != postproc::kNoCell) {
      const Row row = rows[r];
      const List& l = postproc::row_has_pair(in, r) ? pair : single;
      const Cell cell = postproc::cell_of(l, row.na, row.nb, j);
      id = postproc::cell_id(in, r, cell);
      attention = 1;
      type = cell.kind == postproc::IT_B;
      special = cell.kind == postproc::IT_SPECIAL;
    }
    __builtin_nontemporal_store(id, &m.ids[c]);
    __builtin_nontemporal_store(attention, &m.attention_mask[c]);
    __builtin_nontemporal_store(type, &m.token_type_ids[c]);
    __builtin_nontemporal_store(special, &m.special_tokens_mask[c]);
  }
}

hipError_t launch_write_matrix(const In& in, const Opts& o, const DevProgram& p, const Row* rows, const uint64_t* off, const Matrix& m,
                               hipStream_t s) {
  if (!in.n_rows) return hipSuccess;
  const uint64_t cells = in.n_rows * m.width;
  k_pp_write_matrix<<<grid_for(cells > in.n_rows ? cells : in.n_rows, kMaxGrid), kThreads, staged_bytes(p), s>>>(in, o, p, rows, off, m);
  return hipGetLastError();
}

}  // namespace ctok_pp
