// HIP kernels (gfx950) of PipelineTokenizer's Encoding path behind include/ctok_pipeline.h: every word's
// span in its sequence's original text, every id's offsets and word index, and the masks of the
// processed rows.  The rules are pipeline_enc_hd.h's, which tools/pipeline_enc_check.cpp runs on the CPU.
//
// Reference (Complexity-ML/complexity-tokenizer v0.3.3):
//   pre_tokenize_with_offsets    src/huggingface/mod.rs:448-480   k_pe_word_find
//   encode_single_to_encoding    src/huggingface/mod.rs:395-443   k_pe_tok_len, k_pe_tok_spans
//   encode_to_encoding_impl      src/huggingface/mod.rs:358-392   k_pe_row_heads, k_pe_enc_rows
//
// k_pe_word_find: a wavefront per sequence.  The words of a sequence depend on each other (a search
// starts where the previous word ended), so the loop over them is wave-uniform; the search is wave-
// parallel: lane i tests the candidate at base + i, the first byte first, and __ballot's lowest lane of
// the first window with a match is the leftmost match.  A candidate is tested only when it ends at or
// before the sequence's end, so no byte of the next text (or of a caller's tail) is read.  The needle
// is read from global memory: all lanes of a window read the same needle byte at each step.
// The other kernels own an id, a row or a cell per thread; every loop is a binary search.
// The only hand-off between workgroups is the kernel boundary.  No MFMA: byte and integer work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pipeline_enc_internal.h"

namespace ctok_pe {

using namespace pipeline_enc;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;

static uint32_t grid_for(uint64_t n, uint32_t per_block, uint32_t max_grid) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {  // the same value in every lane
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, d);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void k_pe_word_find(Find f) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t q = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); q < f.n_seqs; q += n_waves) {
    const uint64_t o0 = f.off[q], o1 = f.off[q + 1];
    const uint8_t* text = f.text + o0;
    const uint64_t L = o1 > o0 ? o1 - o0 : 0;
    uint64_t w0 = f.text_word[q], w1 = f.text_word[q + 1];
    if (w1 > f.n_words) w1 = f.n_words;
    if (w0 > w1) w0 = w1;
    uint64_t s = 0, work = 0;
    uint64_t lane_cmp = 0;  // this lane's equal bytes after a first byte: the cost of partial matches, which `work` does not see
    bool cmp_over = false;
    for (uint64_t w = w0; w < w1 && !cmp_over; w++) {
      if (boundary_panic(text, L, s)) {
        if (lane == 0) atomicMin(&f.rep[kRepPanic], (unsigned long long)(q << 32 | s));
        break;
      }
      const uint64_t a = f.word_off[w], b = f.word_off[w + 1];
      const uint64_t wl = b > a ? b - a : 0;
      const uint64_t skip = needle_skip(f.words + a, wl);
      const uint8_t* needle = f.words + a + skip;
      const uint64_t m = wl - skip;
      uint64_t pos = L + 1;
      bool cut = false;
      if (!m) {
        pos = s;
      } else {
        for (uint64_t base = s; base <= L && m <= L - base; base += 64) {
          if (work + (base - s) > f.limit) {  // whatever the search finds, the work is above the limit
            work += base - s;
            cut = true;
            break;
          }
          const unsigned long long hits = __ballot(match_at(text, L, base + lane, needle, m, &lane_cmp));
          if (hits) {
            pos = base + (uint64_t)(__ffsll(hits) - 1);
            break;
          }
          // a window lasts as long as its longest compare: every 64 windows, the lane that compared the most
          if ((((base - s) >> 6) & 63) == 63 && wave_max(lane_cmp) > f.cmp_limit) {
            cmp_over = true;
            break;
          }
        }
      }
      if (cut || cmp_over) break;
      uint64_t ws, we, wk;
      word_span(pos, s, m, wl, L, &ws, &we, &wk);
      if (lane == 0) {
        f.wstart[w] = ws;
        f.wend[w] = we;
      }
      work += wk;
      s = we;
      if (work > f.limit) break;
      cmp_over = wave_max(lane_cmp) > f.cmp_limit;
    }
    if (lane == 0) {
      f.work[q] = work;
      atomicMax(&f.rep[kRepMaxWork], (unsigned long long)work);
      if (work > f.limit) atomicMin(&f.rep[kRepOver], (unsigned long long)q);
      else if (cmp_over) atomicMin(&f.rep[kRepCompares], (unsigned long long)q);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_pe_tok_len(Spans p) {
  for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k <= p.n_ids; k += (uint64_t)gridDim.x * kThreads)
    p.scan[k] = k < p.n_ids ? table_len(p.len_id, p.len_val, p.n_len, p.ids[k]) : 0;
}

__global__ __launch_bounds__(kThreads) void k_pe_tok_spans(Spans p) {
  for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < p.n_ids; k += (uint64_t)gridDim.x * kThreads) {
    // wpos[n_words] = n_ids > k and text_word[n_seqs] = n_words > w: the owners are below the ends
    const uint32_t w = find_owner32(p.wpos, p.n_words, (uint32_t)k);
    const uint64_t q = find_owner(p.text_word, p.n_seqs, w);
    if (w >= p.n_words || q >= p.n_seqs) continue;
    uint64_t a, e;
    tok_span(p.wstart[w], p.wend[w], p.scan[k], p.scan[k + 1], p.scan[p.wpos[w]], &a, &e);
    p.offsets[2 * k] = a;
    p.offsets[2 * k + 1] = e;
    p.word_ids[k] = (uint32_t)(w - p.text_word[q]);
  }
}

__global__ __launch_bounds__(kThreads) void k_pe_row_heads(Rows r) {
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i <= r.n_rows; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t at = r.tok_off[i * r.per_row];
    r.seq_off[i] = at;
    if (i < r.n_rows) r.n_a[i] = r.tok_off[i * r.per_row + 1] - at;
  }
}

__global__ __launch_bounds__(kThreads) void k_pe_enc_rows(Rows r) {
  __shared__ uint32_t s_special[kMaxSpecial];
  const uint32_t n_sp = r.n_special < kMaxSpecial ? r.n_special : kMaxSpecial;
  for (uint32_t i = threadIdx.x; i < n_sp; i += kThreads) s_special[i] = r.special[i];
  __syncthreads();
  const uint64_t n = r.n_cells > r.n_rows ? r.n_cells : r.n_rows;
  for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kThreads) {
    if (j < r.n_rows && r.row_off[j + 1] - r.row_off[j] < r.seq_off[j + 1] - r.seq_off[j])
      atomicMin(&r.rep[kRepShort], (unsigned long long)j);
    if (j >= r.n_cells) continue;
    const uint64_t row = find_owner(r.row_off, r.n_rows, j);  // row_off[n_rows] = n_cells > j
    if (row >= r.n_rows) continue;
    uint32_t t, sp;
    row_cell(j - r.row_off[row], r.seq_off[row + 1] - r.seq_off[row], r.n_a[row], is_special(s_special, n_sp, r.out_ids[j]), &t, &sp);
    r.type_ids[j] = t;
    r.special_mask[j] = sp;
  }
}

hipError_t launch_word_find(const Find& f, hipStream_t s) {
  if (f.n_seqs) k_pe_word_find<<<grid_for(f.n_seqs, kWaves, 1u << 20), kThreads, 0, s>>>(f);
  return hipGetLastError();
}

hipError_t launch_tok_len(const Spans& p, hipStream_t s) {
  k_pe_tok_len<<<grid_for(p.n_ids + 1, kThreads, 8192), kThreads, 0, s>>>(p);
  return hipGetLastError();
}

hipError_t launch_tok_spans(const Spans& p, hipStream_t s) {
  if (p.n_ids) k_pe_tok_spans<<<grid_for(p.n_ids, kThreads, 8192), kThreads, 0, s>>>(p);
  return hipGetLastError();
}

hipError_t launch_row_heads(const Rows& r, hipStream_t s) {
  k_pe_row_heads<<<grid_for(r.n_rows + 1, kThreads, 8192), kThreads, 0, s>>>(r);
  return hipGetLastError();
}

hipError_t launch_enc_rows(const Rows& r, hipStream_t s) {
  const uint64_t n = r.n_cells > r.n_rows ? r.n_cells : r.n_rows;
  if (n) k_pe_enc_rows<<<grid_for(n, kThreads, 8192), kThreads, 0, s>>>(r);
  return hipGetLastError();
}

}  // namespace ctok_pe
