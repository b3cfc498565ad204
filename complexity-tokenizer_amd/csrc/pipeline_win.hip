// HIP kernels (gfx950) of PipelineTokenizer's padded batches and overflowing stride windows behind
// include/ctok_pipeline.h: the rows an Encoding call left on the device become [n_windows, width] arrays
// of ids, attention mask, type ids, special mask, offsets, word ids and sequence ids without a trip
// through host memory.  The rules are pipeline_win_hd.h's, which tools/pipeline_win_check.cpp runs on the CPU.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   Encoding::truncate / truncate_with_stride / pad   src/encoding.rs:87-223
//   as called from encode_to_encoding_impl            src/huggingface/mod.rs:358-392
//   and Tokenizer.__call__                            src/bindings/tokenizer.rs:33-201
//
// Count, scan, refuse, write:
//   k_pw_plan     a thread per row: the row's window count, the wave maximum of the main windows, the lowest
//                 row the reference panics on
//   (scan_u64 over the counts: row_win)
//   k_pw_records  a thread per window -- one row can own thousands -- bisects row_win for its row
//   k_pw_write    a wavefront per window: the record and the row's numbers are read once per wave (they are
//                 the same in all 64 lanes), the lanes own consecutive columns, so every load and store of
//                 a cell is one contiguous run of the wave.  The offsets array is walked as 2 * width u64.
//                 An array that is not wanted costs a test of a wave-uniform pointer per window.
// The only hand-off between workgroups is the kernel boundary.  No MFMA: a gather and streaming writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pipeline_win_internal.h"

namespace ctok_pw {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;

static uint32_t grid_for(uint64_t n, uint32_t per_block, uint32_t max_grid) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

// the last r in [0, n) with off[r] <= x (off[0] <= x < off[n])
__device__ __forceinline__ uint64_t owner(const uint64_t* __restrict__ off, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool in_sorted(const uint32_t* __restrict__ list, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t v = list[mid];
    if (v == id) return true;
    if (v < id) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// Encoding::from_ids rows: `tokens` leaves out the ids that have no vocab string.  Only added tokens with
// ids outside the vocab are such ids, so the few threads that find one look up their row.
__global__ __launch_bounds__(kThreads) void k_pw_tokenless(const uint32_t* __restrict__ ids, uint64_t n_ids, const uint64_t* __restrict__ seq_off,
                                                           uint64_t n_rows, const uint32_t* __restrict__ table, uint32_t n_table,
                                                           uint32_t* tokenless) {
  for (uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x; g < n_ids; g += (uint64_t)gridDim.x * kThreads) {
    if (in_sorted(table, n_table, ids[g])) continue;
    atomicAdd(&tokenless[owner(seq_off, n_rows, g)], 1u);  // seq_off[n_rows] = n_ids > g
  }
}

struct RowLens {
  uint64_t P, n, t;
};

__device__ __forceinline__ RowLens row_lens(const Win& w, uint64_t r) {
  RowLens x;
  x.P = w.row_off[r + 1] - w.row_off[r];
  x.n = w.seq_off[r + 1] - w.seq_off[r];
  x.t = w.tokenless ? x.n - w.tokenless[r] : x.n;
  return x;
}

__global__ __launch_bounds__(kThreads) void k_pw_plan(Win w) {
  const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint64_t L = 0;
  if (r < w.n_rows) {
    const RowLens x = row_lens(w, r);
    w.row_win[r] = pwin::count(w.mode, x.P, w.m, w.stride);
    L = pwin::main_len(w.mode, x.P, w.m);
    if (pwin::panics(w.mode, x.P, x.t, w.m)) atomicMin(&w.rep[kRepPanic], (unsigned long long)r);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor((unsigned long long)L, o, 64);
    L = u > L ? u : L;
  }
  if ((threadIdx.x & 63) == 0 && L) atomicMax(&w.rep[kRepMain], (unsigned long long)L);
}

__global__ __launch_bounds__(kThreads) void k_pw_records(Win w) {
  for (uint64_t v = (uint64_t)blockIdx.x * kThreads + threadIdx.x; v < w.n_windows; v += (uint64_t)gridDim.x * kThreads) {
    // every row has a window, so row_win increases strictly; row_win[n_rows] = n_windows > v
    const uint64_t r = owner(w.row_win, w.n_rows, v);
    const uint64_t k = v - w.row_win[r];
    const RowLens x = row_lens(w, r);
    const uint64_t a = pwin::start(k, w.m, w.stride), e = pwin::end(w.mode, k, x.P, w.m, w.stride);
    const uint64_t enc = pwin::enc_len(k, e - a, w.target);
    w.win_row[v] = (uint32_t)r;
    w.win_len[v] = enc;
    if (w.win_start) w.win_start[v] = a;
    if (w.win_off_len) w.win_off_len[v] = w.offsets ? pwin::list_len(x.n, a, e) : 0;
    if (w.win_seq_len) w.win_seq_len[v] = pwin::list_len(x.n, a, e) + (enc - (e - a));
  }
}

__global__ __launch_bounds__(kThreads) void k_pw_write(Win w) {
  const uint32_t lane = threadIdx.x & 63;
  // (threadIdx.x >> 6 is the same in a wave's lanes, which the compiler cannot see by itself)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  const uint64_t width = w.width;
  for (uint64_t v = (uint64_t)blockIdx.x * kWaves + wave; v < w.n_windows; v += n_waves) {
    // once per wave: the record and the row's numbers
    const uint64_t r = w.win_row[v];
    const uint64_t k = v - w.row_win[r];
    const uint64_t base = w.row_off[r], P = w.row_off[r + 1] - base;
    const uint64_t sbase = w.seq_off[r], n = w.seq_off[r + 1] - sbase;
    const uint64_t na = w.n_a[r];
    const uint64_t a = pwin::start(k, w.m, w.stride), e = pwin::end(w.mode, k, P, w.m, w.stride);
    const uint64_t len = e - a;                                                 // ids
    const uint64_t lead = w.pad_left ? pwin::enc_len(k, len, w.target) - len : 0;  // padding cells in front
    const uint64_t lists = pwin::list_len(n, a, e);                             // entries of a list of n
    const uint64_t o = v * width;
    const uint32_t* __restrict__ src = w.ids + base + a;
    for (uint64_t c = lane; c < width; c += 64) {
      const bool in = c >= lead && c - lead < len;
      w.out_ids[o + c] = in ? src[c - lead] : w.pad_id;
    }
    if (w.out_attn)
      for (uint64_t c = lane; c < width; c += 64) w.out_attn[o + c] = c >= lead && c - lead < len ? 1u : 0u;
    if (w.out_type) {
      for (uint64_t c = lane; c < width; c += 64) {
        const bool in = c >= lead && c - lead < len;
        const uint64_t p = a + (c - lead);
        w.out_type[o + c] = !in ? 0u : w.type_ids ? w.type_ids[base + p] : (p >= na ? 1u : 0u);
      }
    }
    if (w.out_special) {
      for (uint64_t c = lane; c < width; c += 64) {
        const bool in = c >= lead && c - lead < len;
        w.out_special[o + c] = !in ? 1u : w.special_mask ? w.special_mask[base + a + (c - lead)] : 0u;
      }
    }
    // offsets and word ids are not moved by the padding: cell j is list element j
    const uint64_t offs = w.offsets ? lists : 0;
    if (w.out_offsets) {
      const uint64_t* __restrict__ so = w.offsets ? w.offsets + 2 * (sbase + a) : nullptr;
      for (uint64_t c = lane; c < 2 * width; c += 64) w.out_offsets[2 * o + c] = c < 2 * offs ? so[c] : 0ull;
    }
    if (w.out_word) {
      const uint32_t* __restrict__ sw = w.word_ids ? w.word_ids + sbase + a : nullptr;
      for (uint64_t c = lane; c < width; c += 64) w.out_word[o + c] = c < offs ? sw[c] : kNoneCell;
    }
    // sequence_ids: None for the padding, in front on a left pad
    if (w.out_seq) {
      for (uint64_t c = lane; c < width; c += 64) {
        const bool in = c >= lead && c - lead < lists;
        w.out_seq[o + c] = in ? (a + (c - lead) >= na ? 1u : 0u) : kNoneCell;
      }
    }
  }
}

hipError_t launch_tokenless(const uint32_t* ids, uint64_t n_ids, const uint64_t* seq_off, uint64_t n_rows, const uint32_t* table,
                            uint32_t n_table, uint32_t* tokenless, hipStream_t s) {
  if (n_ids && n_rows) k_pw_tokenless<<<grid_for(n_ids, kThreads, 8192), kThreads, 0, s>>>(ids, n_ids, seq_off, n_rows, table, n_table, tokenless);
  return hipGetLastError();
}

hipError_t launch_plan(const Win& w, hipStream_t s) {
  if (w.n_rows) k_pw_plan<<<(uint32_t)((w.n_rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(w);
  return hipGetLastError();
}

hipError_t launch_records(const Win& w, hipStream_t s) {
  if (w.n_windows) k_pw_records<<<grid_for(w.n_windows, kThreads, 8192), kThreads, 0, s>>>(w);
  return hipGetLastError();
}

// at most 2048 workgroups of four wavefronts: 8 per CU, all resident at once
hipError_t launch_write(const Win& w, hipStream_t s) {
  if (w.n_windows && w.width) k_pw_write<<<grid_for(w.n_windows, kWaves, 2048), kThreads, 0, s>>>(w);
  return hipGetLastError();
}

}  // namespace ctok_pw
