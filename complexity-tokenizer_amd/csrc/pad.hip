// HIP kernels (gfx950 / CDNA4) for the padded batch encode: encoded ids -> Encoding rows as
// [rows, width] arrays of ids, attention mask, type ids and special-tokens mask.
//
// Reference path (Complexity-ML/complexity-tokenizer v0.3.3):
//   Tokenizer.__call__ / encode_batch_with_padding / encode_batch_to_encoding
//                                          src/bindings/tokenizer.rs:46-201, :326-371
//   encode_to_encoding_impl                src/huggingface/mod.rs:358-392 (merge pair, process(ids,
//                                          None), masks extended by the added count, mark_special)
//   encode_batch_with_padding              src/huggingface/mod.rs:483-509
//   Encoding::from_ids / merge / truncate / pad   src/encoding.rs:45-131, :240-253
//
// Per row: n = ids of the row (pair: na + nb), P = the processed length (n times each $A item +
// one per special item), L = min(P, max_len) when truncating, then pad to the target.  Cell i of
// the content: the processed id, attention 1, type id (i < n ? i >= na : 0 -- the pair's ids are
// type 1, the post-processor's additions type 0), special mask (i >= n, or the id is a special
// token when marking).  Padding cells: pad id, attention 0, type 0, special 1.  A pure gather +
// streaming write: HBM-bound, one thread per output cell, consecutive lanes -> consecutive cells.
//
// Overflowing stride windows (k_win_len, k_win_rows): rows longer than max_len as the windows of
//   Encoding::truncate_with_stride         src/encoding.rs:175-223
// reached from __call__(truncation, stride) (src/bindings/tokenizer.rs:102-112) and
// encode_with_truncation (src/huggingface/mod.rs:348-392); the arithmetic is window_hd.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ctok_internal.h"
#include "window_hd.h"

namespace ctok_dev {

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

struct PadRow {
  uint64_t base;  // first id of the row in w.ids
  uint32_t n, na;
  uint64_t P, L;
};

__device__ __forceinline__ PadRow pad_row(const PadWork& w, uint32_t r, uint32_t nA, uint32_t nS) {
  PadRow x;
  const uint32_t a = w.pairs ? 2 * r : r;
  x.base = w.tok_off[a];
  const uint64_t ea = w.tok_off[a + 1];
  const uint64_t e = w.pairs ? w.tok_off[a + 2] : ea;
  x.na = (uint32_t)(ea - x.base);
  x.n = (uint32_t)(e - x.base);
  x.P = w.use_tpl ? (uint64_t)nA * x.n + nS : x.n;
  x.L = (w.truncate && x.P > w.max_len) ? w.max_len : x.P;
  return x;
}

__device__ __forceinline__ void count_items(const PadWork& w, uint32_t& nA, uint32_t& nS) {
  nA = 0;
  nS = 0;
  for (uint32_t k = 0; k < w.n_items; k++) {
    if (w.items[k] == kPadItemA) nA++;
    else nS++;
  }
}

// row lengths, the longest content, and the reference's panic when a template drops ids
// (`processed_ids.len() - encoding.ids.len()` underflows, src/huggingface/mod.rs:378)
__global__ void k_pad_len(PadWork w) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t nA, nS;
  count_items(w, nA, nS);
  uint64_t L = 0;
  if (r < w.n_rows) {
    const PadRow x = pad_row(w, r, nA, nS);
    if (x.P < x.n) atomicOr(&w.counters[2], 1u);
    L = x.L;
    w.row_len[r] = L > w.target ? L : w.target;
  }
  // wave maximum, one atomic per wave
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(L, o, 64);
    L = u > L ? u : L;
  }
  if ((threadIdx.x & 63) == 0 && L) atomicMax((unsigned long long*)w.counters, (unsigned long long)L);
}

// id is in the sorted list
__device__ __forceinline__ bool in_sorted(const uint32_t* list, uint32_t n, uint32_t id) {
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

__device__ __forceinline__ bool is_special(const PadWork& w, uint32_t id) {
  return in_sorted(w.special_ids, w.n_special, id);
}

// The per-cell body shared by k_pad_rows and k_win_rows: the values of content position i of row
// x (the template walk, type id, special mask and marking), or of a padding cell, stored at cell o
__device__ __forceinline__ void row_cell(const PadWork& w, const PadRow& x, bool is_pad, uint64_t i, uint64_t o) {
  uint32_t id = w.pad_id, attn = 0, type = 0, spec = 1;
  if (!is_pad) {
    if (w.use_tpl) {
      uint64_t off = 0;
      for (uint32_t k = 0; k < w.n_items; k++) {
        const uint32_t it = w.items[k];
        const uint64_t len = it == kPadItemA ? x.n : 1;
        if (i < off + len) {
          id = it == kPadItemA ? w.ids[x.base + (i - off)] : it;
          break;
        }
        off += len;
      }
    } else {
      id = w.ids[x.base + i];
    }
    attn = 1;
    type = (i < x.n && i >= x.na) ? 1u : 0u;
    spec = (i >= x.n || (w.mark && is_special(w, id))) ? 1u : 0u;
  }
  w.out_ids[o] = id;
  if (w.out_attn) w.out_attn[o] = attn;
  if (w.out_type) w.out_type[o] = type;
  if (w.out_special) w.out_special[o] = spec;
}

__device__ __forceinline__ void pad_cell(const PadWork& w, uint32_t r, uint64_t c, uint32_t nA, uint32_t nS) {
  const PadRow x = pad_row(w, r, nA, nS);
  const uint64_t rowlen = x.L > w.target ? x.L : w.target;
  const uint64_t pad = rowlen - x.L;
  bool is_pad;
  uint64_t i = 0;
  if (c >= rowlen) {
    is_pad = true;  // past a ragged row's end: filled like padding
  } else if (w.pad_left) {
    is_pad = c < pad;
    i = c - pad;
  } else {
    is_pad = c >= x.L;
    i = c;
  }
  row_cell(w, x, is_pad, i, (uint64_t)r * w.width + c);
}

// one thread per output cell (grid-stride over rows * width, row-major: consecutive lanes write
// consecutive cells of a row)
__global__ __launch_bounds__(256) void k_pad_rows(PadWork w) {
  uint32_t nA, nS;
  count_items(w, nA, nS);
  const uint64_t total = (uint64_t)w.n_rows * w.width;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x; cell < total; cell += stride) {
    const uint32_t r = (uint32_t)(cell / w.width);
    pad_cell(w, r, cell - (uint64_t)r * w.width, nA, nS);
  }
}

// ---- overflowing stride windows (window_hd.h) ---------------------------------------------

// per row: its window count into row_win (the host scans it into first-window indices), the
// longest main window (k_pad_len's wave maximum: L = min(P, max_len)), and the two panics of the
// reference -- a template that drops ids (as k_pad_len), and an overflowing row whose template
// changed its length: every window slices `tokens`, still n long, up to P (src/encoding.rs:189)
__global__ void k_win_len(WinWork w) {
  const PadWork& p = w.p;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t nA, nS;
  count_items(p, nA, nS);
  uint64_t L = 0;
  if (r < p.n_rows) {
    const PadRow x = pad_row(p, r, nA, nS);
    if (x.P < x.n) atomicOr(&p.counters[2], 1u);
    if (x.P > p.max_len && x.P != x.n) atomicOr(&p.counters[3], 1u);
    L = x.L;
    w.row_win[r] = win::count(x.P, p.max_len, w.stride);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(L, o, 64);
    L = u > L ? u : L;
  }
  if ((threadIdx.x & 63) == 0 && L) atomicMax((unsigned long long*)p.counters, (unsigned long long)L);
}

// Encoding::from_ids rows (no special tokens: Tokenizer.encode's ids, tokens = the ids' vocab
// strings with the ids that have none left out, src/bindings/tokenizer.rs:88-97): a row holding
// such an id has fewer tokens than ids, so when it overflows, its windows slice `tokens` past
// their end as well.  Only added tokens with ids outside model.vocab are such ids (w.tokenless,
// sorted); launched only when the tokenizer has some.  One thread per id of the batch; the few
// that match look up their row.
__global__ __launch_bounds__(256) void k_win_tokens(WinWork w, uint32_t n_docs) {
  const PadWork& p = w.p;
  const uint64_t n_ids = p.tok_off[n_docs];
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n_ids; g += (uint64_t)gridDim.x * 256) {
    if (!in_sorted(w.tokenless, w.n_tokenless, p.ids[g])) continue;
    uint32_t lo = 0, hi = n_docs;  // tok_off[lo] <= g < tok_off[hi] (empty docs repeat a value)
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (p.tok_off[mid] <= g) lo = mid;
      else hi = mid;
    }
    const PadRow x = pad_row(p, p.pairs ? lo >> 1 : lo, 0, 0);
    if (x.P > p.max_len) atomicOr(&p.counters[3], 1u);
  }
}

// One wavefront per window, its lanes over consecutive columns, and a contiguous share of the
// windows per wavefront: the first window's row is found by bisecting the scanned row_win, the
// later ones' by stepping on (a search per window is a chain of dependent loads that the stores
// then wait for).  The row's numbers, the window's bounds and the padding are computed once per
// wave -- everything but the column is the same in all 64 lanes, so no cell pays a 64-bit division
// or a search.  Window k of the row holds content positions [k * (max_len - stride), min(.. +
// max_len, P)); only window 0 is padded to the target (on the left with pad_left), as the
// reference pads the main encoding and leaves its overflowing list alone.  Cells outside the
// window's Encoding are filled like padding.
constexpr int kWinWaves = 4;

__global__ __launch_bounds__(64 * kWinWaves) void k_win_rows(WinWork w) {
  const PadWork& p = w.p;
  uint32_t nA, nS;
  count_items(p, nA, nS);
  const uint32_t lane = threadIdx.x & 63;
  // (threadIdx.x >> 6 is the same in a wave's lanes, which the compiler cannot see by itself)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t* __restrict__ row_win = w.row_win;
  // the wave's windows: a contiguous share, so the row is searched once and then only advanced
  const uint64_t n_waves = (uint64_t)gridDim.x * kWinWaves;
  const uint64_t share = (w.n_windows + n_waves - 1) / n_waves;
  const uint64_t w0 = ((uint64_t)blockIdx.x * kWinWaves + wave) * share;
  const uint64_t w1 = w0 + share < w.n_windows ? w0 + share : w.n_windows;
  if (w0 >= w1) return;
  // the last row with row_win[r] <= w0: row_win[0] = 0, row_win[n_rows] = n_windows > w0, and every
  // row has a window, so the values increase strictly
  uint32_t r = 0, hi = p.n_rows;
  while (hi - r > 1) {
    const uint32_t mid = r + ((hi - r) >> 1);
    if (row_win[mid] <= w0) r = mid;
    else hi = mid;
  }
  uint64_t first = row_win[r], next = row_win[r + 1];
  PadRow x = pad_row(p, r, nA, nS);
  for (uint64_t wv = w0; wv < w1; wv++) {
    while (wv >= next) {
      r++;
      first = next;
      next = row_win[r + 1];
      x = pad_row(p, r, nA, nS);
    }
    const uint64_t k = wv - first;
    const uint64_t start = win::start(k, p.max_len, w.stride);
    const uint64_t len = k ? win::end(k, x.P, p.max_len, w.stride) - start : x.L;  // content cells
    const uint64_t enc_len = (k == 0 && p.target > len) ? p.target : len;         // with window 0's padding
    const uint64_t lead = p.pad_left ? enc_len - len : 0;                          // padding cells in front
    if (lane == 0) {
      w.win_len[wv] = enc_len;
      w.win_row[wv] = r;
      if (w.win_start) w.win_start[wv] = start;
    }
    const uint64_t o = wv * p.width;
    for (uint64_t c = lane; c < p.width; c += 64) row_cell(p, x, c < lead || c >= lead + len, start + (c - lead), o + c);
  }
}

hipError_t launch_pad_len(const PadWork& w, hipStream_t s) {
  if (w.n_rows) k_pad_len<<<(w.n_rows + 255) / 256, 256, 0, s>>>(w);
  return hipGetLastError();
}

hipError_t launch_pad_rows(const PadWork& w, hipStream_t s) {
  const uint64_t total = (uint64_t)w.n_rows * w.width;
  if (!total) return hipSuccess;
  const uint64_t blocks = (total + 255) / 256;
  k_pad_rows<<<(uint32_t)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(w);
  return hipGetLastError();
}

hipError_t launch_win_len(const WinWork& w, hipStream_t s) {
  if (!w.p.n_rows) return hipSuccess;
  k_win_len<<<(w.p.n_rows + 255) / 256, 256, 0, s>>>(w);
  if (w.n_tokenless) {
    const uint32_t n_docs = w.p.pairs ? 2 * w.p.n_rows : w.p.n_rows;
    k_win_tokens<<<(uint32_t)std::min<uint64_t>(w.ids_bound / 256 + 1, 2048), 256, 0, s>>>(w, n_docs);
  }
  return hipGetLastError();
}

// at most 1536 workgroups (6 per CU, 24 wavefronts: what stays resident at once); timed on one
// batch with 512 .. 4096, and with 16-byte stores, in profiles/stride_windows/ab_summary.txt
hipError_t launch_win_rows(const WinWork& w, hipStream_t s) {
  if (!w.n_windows) return hipSuccess;
  const uint64_t blocks = (w.n_windows + kWinWaves - 1) / kWinWaves;
  k_win_rows<<<(uint32_t)(blocks < 1536 ? blocks : 1536), 64 * kWinWaves, 0, s>>>(w);
  return hipGetLastError();
}

}  // namespace ctok_dev
