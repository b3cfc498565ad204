// Encode path: device-wide exclusive scans -- scan_u32 / scan_u64 (k_scan_*) and the tile scan
// before emission (k_tiles_*).
#include "dev_common.h"

namespace ctok_dev {

// ------------------------------------------------------------------------------------------
// device-wide exclusive scan (4096 elements per 256-thread block, recursive over partials)

constexpr int kScanPer = 16;
constexpr int kScanBlock = 256 * kScanPer;

template <typename T>
__global__ __launch_bounds__(256) void k_scan_reduce(const T* __restrict__ in, uint64_t n_max, const uint32_t* n_dev,
                                                     T* __restrict__ part) {
  __shared__ T s_scan[17];
  const uint64_t n = n_dev ? (uint64_t)*n_dev : n_max;
  const uint64_t b0 = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanPer;
  T s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    const uint64_t i = b0 + k;
    if (i < n) s += in[i];
  }
  T total;
  block_excl_scan<T>(s, s_scan, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(256) void k_scan_apply(const T* in, T* out, uint64_t n_max, const uint32_t* n_dev,
                                                    const T* __restrict__ part_scanned, int write_total) {
  __shared__ T s_scan[17];
  const uint64_t n = n_dev ? (uint64_t)*n_dev : n_max;
  const uint64_t b0 = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanPer;
  T v[kScanPer];
  T s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    const uint64_t i = b0 + k;
    v[k] = i < n ? in[i] : T(0);
    s += v[k];
  }
  T total;
  T ex = block_excl_scan<T>(s, s_scan, &total);
  const T base = part_scanned ? part_scanned[blockIdx.x] : T(0);
  ex += base;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    const uint64_t i = b0 + k;
    if (i < n) out[i] = ex;
    ex += v[k];
  }
  if (write_total && threadIdx.x == 0) out[n] = base + total;  // index n is read by no thread
}

template <typename T>
__global__ void k_write_total(T* out, uint64_t n_max, const uint32_t* n_dev, const T* part, uint64_t nb) {
  const uint64_t n = n_dev ? (uint64_t)*n_dev : n_max;
  out[n] = part[nb];
}

// exclusive scan of in[0, n) into out[0, n) (in place allowed) and out[n] = total
template <typename T>
static hipError_t scan_impl(const T* in, T* out, uint64_t n_max, const uint32_t* n_dev, T* tmp, uint64_t tmp_cap,
                            hipStream_t s) {
  const uint64_t nb = (n_max + kScanBlock - 1) / kScanBlock;
  if (nb <= 1) {
    k_scan_apply<T><<<1, 256, 0, s>>>(in, out, n_max, n_dev, nullptr, 1);
    return hipGetLastError();
  }
  if (nb + 1 > tmp_cap) return hipErrorInvalidValue;
  T* part = tmp;
  k_scan_reduce<T><<<(unsigned)nb, 256, 0, s>>>(in, n_max, n_dev, part);
  HIPCHK(hipGetLastError());
  HIPCHK(scan_impl<T>(part, part, nb, nullptr, tmp + nb + 1, tmp_cap - nb - 1, s));  // part[nb] = total
  k_scan_apply<T><<<(unsigned)nb, 256, 0, s>>>(in, out, n_max, n_dev, part, 0);
  HIPCHK(hipGetLastError());
  k_write_total<T><<<1, 1, 0, s>>>(out, n_max, n_dev, part, nb);
  return hipGetLastError();
}

uint64_t scan_tmp_elems(uint64_t n_max) {
  uint64_t tot = 0;
  uint64_t n = n_max;
  for (;;) {
    const uint64_t nb = (n + kScanBlock - 1) / kScanBlock;
    if (nb <= 1) break;
    tot += nb + 1;
    n = nb;
  }
  return tot + 16;
}

// Both per-tile scans (tile_tok: the tiles' first ids, tile_doc: their first documents) as ONE
// scan of packed u64 values tok | doc << 32: every partial sum of either array is below 2^32 (ids
// and documents of a call are < 2^32), so the low half never carries into the high one.
// Reduce, scan of the block partials, apply: 3 launches (1 for <= 4096 tiles) instead of 8 (and
// the apply sums the pieces for the statistics, which took a launch of its own).
// The tile scan's blocks: 1024 tiles (4 per thread), so that a call of a few tens of thousands of
// tiles (a 160 MB shard: 40k) spreads its reduce and apply over tens of workgroups instead of ten
// (its 3 launches took 23 us there with 4096-tile blocks)
constexpr int kTileScanPer = 4;
constexpr int kTileScanBlock = 256 * kTileScanPer;

__device__ __forceinline__ uint64_t tile_pair(const Work& w, uint64_t i) {
  return i < w.n_tiles ? (uint64_t)w.tile_tok[i] | ((uint64_t)w.tile_doc[i] << 32) : 0ull;
}

__global__ __launch_bounds__(256) void k_tiles_reduce(Work w, uint64_t* __restrict__ part) {
  __shared__ uint64_t s_scan[17];
  const uint64_t b0 = (uint64_t)blockIdx.x * kTileScanBlock + threadIdx.x * kTileScanPer;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < kTileScanPer; k++) v += tile_pair(w, b0 + k);
  uint64_t total;
  block_excl_scan<uint64_t>(v, s_scan, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// count: also the batch's pieces (statistics only): the sum of tile_np into counters[kCtrPieces]
__global__ __launch_bounds__(256) void k_tiles_apply(Work w, const uint64_t* __restrict__ part_scanned, uint32_t count) {
  __shared__ uint64_t s_scan[17];
  const uint64_t n = w.n_tiles;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTileScanBlock + threadIdx.x * kTileScanPer;
  uint64_t v[kTileScanPer];
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kTileScanPer; k++) {
    v[k] = tile_pair(w, b0 + k);
    sum += v[k];
  }
  uint64_t total;
  uint64_t ex = block_excl_scan<uint64_t>(sum, s_scan, &total);
  const uint64_t base = part_scanned ? part_scanned[blockIdx.x] : 0ull;
  ex += base;
#pragma unroll
  for (int k = 0; k < kTileScanPer; k++) {
    const uint64_t i = b0 + k;
    if (i < n) {
      w.tile_tok[i] = (uint32_t)ex;
      w.tile_doc[i] = (uint32_t)(ex >> 32);
    }
    ex += v[k];
  }
  if (count) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kTileScanPer; k++)
      if (b0 + k < n) c += w.tile_np[b0 + k];
    c = wave_sum_full_u32(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&w.counters[kCtrPieces], c);  // (counters are zeroed per call)
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {  // the totals at index n
    w.tile_tok[n] = (uint32_t)(base + total);
    w.tile_doc[n] = (uint32_t)((base + total) >> 32);
  }
}

uint64_t tile_scan_tmp_elems(uint64_t n_tiles) {
  const uint64_t nb = (n_tiles + kTileScanBlock - 1) / kTileScanBlock;
  return nb + 1 + scan_tmp_elems(nb + 1);
}

hipError_t scan_tiles(const Work& w, hipStream_t s, bool count, Lx x) {
  const uint64_t nb = ((uint64_t)w.n_tiles + kTileScanBlock - 1) / kTileScanBlock;
  if (nb <= 1) {
    launch_lx(x, k_tiles_apply, 1, 256, 0, s, w, (const uint64_t*)nullptr, count ? 1u : 0u);
    return hipGetLastError();
  }
  uint64_t* part = reinterpret_cast<uint64_t*>(w.scan_tmp);
  const uint64_t cap = w.scan_tmp_cap / 2;
  if (nb + 1 > cap) return hipErrorInvalidValue;
  launch_lx(x, k_tiles_reduce, (unsigned)nb, 256, 0, s, w, part);
  HIPCHK(hipGetLastError());
  HIPCHK(scan_u64(part, nb, part + nb + 1, cap - nb - 1, s));
  k_tiles_apply<<<(unsigned)nb, 256, 0, s>>>(w, part, count ? 1u : 0u);
  return hipGetLastError();
}

hipError_t scan_u32(const uint32_t* in, uint32_t* out, uint64_t n_max, const uint32_t* n_dev, uint32_t* tmp,
                    uint64_t tmp_cap, hipStream_t s) {
  return scan_impl<uint32_t>(in, out, n_max, n_dev, tmp, tmp_cap, s);
}

hipError_t scan_u64(uint64_t* inout, uint64_t n, uint64_t* tmp, uint64_t tmp_cap, hipStream_t s) {
  return scan_impl<uint64_t>(inout, inout, n, nullptr, tmp, tmp_cap, s);
}

}  // namespace ctok_dev
