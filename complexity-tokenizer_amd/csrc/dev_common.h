// Device-side helpers shared by the encode path's translation units (segment.hip, kernels.hip,
// long.hip, emit.hip, scan.hip, nfc.hip): launch plumbing, the report, wave reductions and scans,
// piece-record checks, code-point classes, the merge-table lookup, LDS pointer types.  Device-only:
// every function here is __forceinline__, inline or a template (no definition with external
// linkage), so each translation unit inlines its own copy.  File map: DESIGN.md section 4.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <type_traits>

#include "ctok_internal.h"

namespace ctok_dev {

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

// A kernel launch with Lx's start / stop events (recorded by its own dispatch) through
// hipExtLaunchKernel, or a plain launch when it has none.
template <typename F, typename... A>
static inline void launch_lx(const Lx& x, F k, dim3 grid, dim3 block, uint32_t lds, hipStream_t s, A... a) {
  if (x.start || x.stop)
    hipExtLaunchKernelGGL(k, grid, block, lds, s, x.start, x.stop, 0u, a...);
  else
    hipLaunchKernelGGL(k, grid, block, lds, s, a...);
}

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kDead = 0xFFFFFFFFu;
constexpr uint32_t kSel = kNoRank - 1;  // marks a merge site during a parallel round

// ------------------------------------------------------------------------------------------
// small device helpers

// The call's report (Work::report; one wave, after k_segment has completed): the counters, with
// the class-3 shards summed into counters[kCtrC3Count], into the pinned host words, a
// system-scope release, then the call's sequence number (see k_report).
__device__ __forceinline__ void write_report(const Work& w) {
  const uint32_t lane = threadIdx.x & 63;
  // the class-3 shards (kC3Shards == 64: one per lane): their exclusive prefix into c3pre for
  // k_bpe_sparse, their sum into the report (all ones when a shard overflowed its capacity)
  uint32_t c3 = 0;
  if (w.c3_max) {
    const uint32_t c = w.counters[kNumCounters + lane];
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)inc, o, 64);
      if (lane >= (uint32_t)o) inc += v;
    }
    w.c3pre[lane] = inc - c;
    if (lane == 63) w.c3pre[64] = inc;
    c3 = __shfl((int)inc, 63, 64);
    if (__ballot(c > w.c3_max / kC3Shards)) c3 = ~0u;
  }
  if (lane < (uint32_t)kNumCounters) w.report[lane] = lane == (uint32_t)kCtrC3Count ? c3 : w.counters[lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_store(&w.report[kNumCounters], w.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (and the sequence number itself on its way)
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// Wave minimum in uniform control flow (all 64 lanes active): DPP within each row of 16 (quad
// swaps, half-row and row mirrors, fused into v_min), then the four row minima through
// readlane.  About 10 instructions and no LDS round trip, against six ds_bpermute waits for the
// shuffle form above; the long-piece rounds are latency-bound, with two reductions per round.
__device__ __forceinline__ uint32_t wave_min_full_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));   // lane ^ 1
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));   // lane ^ 2
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  const uint32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const uint32_t c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return min(min(a, b), min(c, d));
}

// Wave sum in uniform control flow, the same DPP row reduction as wave_min_full_u32.
__device__ __forceinline__ uint32_t wave_sum_full_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);   // lane ^ 1
  v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);   // lane ^ 2
  v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ uint64_t lanemask_lt() {
  const uint32_t lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// u32 inclusive wave scan in uniform control flow (all 64 lanes active): DPP row shifts within
// each row of 16, then row broadcasts 15 / 31 -- six fused v_add, against six ds_bpermute round
// trips for the shuffle form (k_segment's and k_emit's per-round scans are on their critical
// paths).  Preferred over the template for u32 arguments.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return v;
}

__device__ __forceinline__ uint32_t lane63(uint32_t v) { return __builtin_amdgcn_readlane(v, 63); }

// block-wide exclusive scan; nthreads = blockDim.x (multiple of 64, <= 1024)
template <typename T>
__device__ T block_excl_scan(T v, T* smem /*[17]*/, T* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  T inc = wave_incl_scan(v);
  if (lane == 63) smem[wid] = inc;
  __syncthreads();
  if (wid == 0) {
    T s = lane < nw ? smem[lane] : T(0);
    T si = wave_incl_scan(s);
    if (lane < nw) smem[lane] = si - s;
    if (lane == nw - 1) smem[16] = si;
  }
  __syncthreads();
  T r = inc - v + smem[wid];
  if (total) *total = smem[16];
  __syncthreads();
  return r;
}

// Wave-uniform values are moved to SGPRs with readfirstlane: the loop exits and the chain walk
// then branch on scalars, so the wave can never split around the cross-lane reductions (a split
// wave reduces over inactive lanes and never terminates).
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Range checks of decoded piece records (opt-in build: -DCTOK_CHECK, tools/build_variant.sh):
// a record out of range prints where it was found and traps, instead of steering a gather
// through garbage offsets (round 5's r05_v12 fault: unwritten merged records).  The host then
// also fills mrec with all ones before each call, so a record no pass wrote is out of range too.
#ifdef CTOK_CHECK
#define CTOK_CHECK_REC(cond, ...)                                                            \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      printf(__VA_ARGS__);                                                                 \
      __builtin_trap();                                                                    \
    }                                                                                      \
  } while (0)
#else
#define CTOK_CHECK_REC(cond, ...) do { } while (0)
#endif

// Diagnostic (CTOK_WGREC=1, Work::wgrec non-null): workgroup `blockIdx.x` of kernel slot k records
// its start and end (wall clock, 100 MHz), its CU (xcc | se | cu) and a count.  The host prints,
// per kernel, the CUs used and the spread of the workgroups' starts and ends (ctok_encode.cpp).
constexpr uint32_t kWgRecMax = 1024;  // (4 kernel slots: short, mid<2>, mid<3>, sparse)
// (stateless: the record's place is recomputed at the end from the kernel argument, so that no
// register stays live across the kernel -- the 64-slot pass is at its register limit)
struct WgRec {
  static __device__ __forceinline__ void begin(uint64_t* base, uint32_t k) {
    if (base && threadIdx.x == 0 && blockIdx.x < kWgRecMax) {
      uint64_t* p = base + ((size_t)k * kWgRecMax + blockIdx.x) * 4;
      p[0] = (uint64_t)wall_clock64();
      p[2] = __smid();
    }
  }
  static __device__ __forceinline__ void end(uint64_t* base, uint32_t k, uint32_t count) {
    if (base && threadIdx.x == 0 && blockIdx.x < kWgRecMax) {
      uint64_t* p = base + ((size_t)k * kWgRecMax + blockIdx.x) * 4;
      p[1] = (uint64_t)wall_clock64();
      p[3] = count;
    }
  }
};

// NFC speculation failed in k_segment (a code point NFC might change): the rest of this pass is
// discarded (the host checks, normalises and runs the pipeline again), so the kernels after
// k_segment return at once instead of merging text that will be re-encoded.
__device__ __forceinline__ bool spec_failed(const Work& w) { return w.nfc_watch == 1 && uni(w.counters[kCtrNfcFlag]) != 0; }

// pieces in the long list (k_segment counts them all; past long_cap they were not stored and the
// host reruns the call with the safe capacities)
__device__ __forceinline__ uint32_t long_count(const Work& w) { return min(w.counters[kCtrLong], w.long_cap); }

// wave-aggregated append to an LDS counter: returns this lane's slot (lanes with take == false
// get garbage).  One ds_add per wave instead of one per lane.
__device__ __forceinline__ uint32_t wave_append(uint32_t* counter, bool take) {
  const uint64_t m = __ballot(take);
  uint32_t base = 0;
  if (m) {
    const uint32_t leader = __ffsll((unsigned long long)m) - 1;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t b = 0;
    if (lane == leader) b = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __builtin_amdgcn_readlane(b, leader);
  }
  return base + (uint32_t)__popcll(m & lanemask_lt());
}

__device__ __forceinline__ int u8len(uint8_t b) {
  return b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : 4;
}

__device__ __forceinline__ int cls_ascii(uint32_t c) {
  // 0 White_Space, 1 letter, 2 number, 3 other
  if (c == 32 || (c >= 9 && c <= 13)) return 0;
  if ((c | 32) >= 'a' && (c | 32) <= 'z') return 1;
  if (c >= '0' && c <= '9') return 2;
  return 3;
}

__device__ __forceinline__ int cls_of(uint32_t cp, const Tables& t) {
  if (cp < 0x80) return cls_ascii(cp);
  if (cp >= 0x110000) return 3;
  const uint32_t blk = t.cls_s1[cp >> 8];
  const uint32_t w = t.cls_s2[blk * 64 + ((cp & 255) >> 2)];
  return (w >> ((cp & 3) * 2)) & 3;
}


// A long-piece round of merge value r applies every occurrence of r at once, except when the table
// is not rank-monotone and r's merge is eager (Tables::eager): then the leftmost one alone, as the
// sequential loop would before a lower-ranked merge the first one enables.  (Wave-uniform r: a
// scalar load.)
__device__ __forceinline__ bool serial_round(const Tables& t, uint32_t r) {
  return !t.proper && ((t.eager[r >> 5] >> (r & 31)) & 1u) != 0;
}
// first_cascade (the rounds of an eager merge): the sequential loop takes the sites of rank r left
// to right, and after each one the pairs it made -- (the left neighbour, or nid when the site two
// tokens before was merged just before; nid) and (nid, the next token as it is) -- compete with the
// remaining sites.  While none of them ranks below r it goes on with the next site; the first site
// that makes a lower-ranked pair is the last one it applies before that pair's merge.  So a round
// applies the sites up to and including the first such one (all of them when there is none), which
// is the sequential result for any merge table; the lookups of this check never set the panic flag
// (they go to a sink counter): a pair they see is formed, and looked up again, only if its site is
// applied.  (x, x) runs of an eager merge take the leftmost site alone.

// Merge-table value of an entry: the merge priority.  Compact tables (new ids strictly increasing
// in rank, the usual layout) store the merged token id itself, so the minimum value is both the
// winning pair and its new id; otherwise the rank is stored and the new id is looked up.
__device__ __forceinline__ bool value_panics(const Tables& t, uint32_t v) {
  return t.compact ? v == kPanicVal : v >= t.n_ranks;
}
__device__ __forceinline__ uint32_t new_id_of(const Tables& t, uint32_t v) {
  return t.compact ? v : t.rank_newid[v];
}

// value of pair (a, b) or kNoRank.  Sets the panic bit when the reference would index
// BpeTokenizer.merges out of range (src/bpe.rs:141).
__device__ __forceinline__ uint32_t rank_of(const Tables& t, uint32_t a, uint32_t b, uint32_t* err) {
  const uint64_t key = ((uint64_t)a << kIdBits) | b;
  uint32_t h = mhash(a, b) & t.merge_mask;
  for (;;) {
    const uint64_t e = t.merge_tab[h];
    if ((e & kKeyMask) == key) {
      const uint32_t r = (uint32_t)(e >> 42);
      if (value_panics(t, r)) { atomicOr(err, kErrPanic); return kNoRank; }
      return r;
    }
    if (e == kEmpty) return kNoRank;
    h = (h + 1) & t.merge_mask;
  }
}

__device__ __forceinline__ uint16_t nfc16(const Tables& t, uint32_t cp) {
  if (cp >= 0x110000) return 0;
  return t.nfc_s2[t.nfc_s1[cp >> 8] * 256 + (cp & 255)];
}

// Neighbour lanes' words (k_segment: lane l needs lanes l - 1 and l + 1), by DPP wave shifts
// (wave_shr:1 / wave_shl:1, GFX9) instead of ds_bpermute: lane 0 (shr) and lane 63 (shl) keep
// their own value, as __shfl_up / __shfl_down leave it.  Uniform control flow only.
__device__ __forceinline__ uint32_t dpp_prev(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t dpp_next(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xF, 0xF, false);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v) {
  return (uint64_t)dpp_prev((uint32_t)v) | ((uint64_t)dpp_prev((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint64_t shfl_down64(uint64_t v) {
  return (uint64_t)dpp_next((uint32_t)v) | ((uint64_t)dpp_next((uint32_t)(v >> 32)) << 32);
}

// Bytes s .. s + 4*NW - 1 of the text as NW little-endian words, read with NW + 1 aligned dword
// loads whose addresses are clamped into the buffer: every load is unconditional (a predicated
// per-byte load makes hipcc branch and wait vmcnt(0) around each one); bytes past the piece or the
// text are garbage and must be masked by the caller.
template <int NW>
__device__ __forceinline__ void load_words(const uint8_t* text, uint32_t s, uint32_t n_bytes, uint32_t (&wv)[NW]) {
  const uint32_t a0 = s & ~3u;
  const uint32_t last = (n_bytes - 1) & ~3u;
  uint32_t d[NW + 1];
#pragma unroll
  for (int j = 0; j <= NW; j++) d[j] = *reinterpret_cast<const uint32_t*>(text + min(a0 + 4 * j, last));
  const uint32_t sh = s & 3u;
#pragma unroll
  for (int j = 0; j < NW; j++) wv[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * (k & 3))) & 255u; }

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint64_t lds_u64;
typedef __attribute__((address_space(3))) uint16_t lds_u16;

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): the attribute is set
// on the current device's instance of the kernel, and ctok_exec.devices launches from one host
// thread per device at once, so the flag is a per-device bit under a lock (one per kernel).
struct LdsAttr {
  std::mutex mu;
  uint64_t done = 0;  // bit d: set on device d (ordinals >= 64 set it on every call)
};
static inline hipError_t lds_attr_once(LdsAttr& a, const void* fn, size_t bytes) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const uint64_t bit = dev < 64 ? 1ull << dev : 0ull;
  std::lock_guard<std::mutex> lk(a.mu);
  if (a.done & bit) return hipSuccess;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  a.done |= bit;
  return hipSuccess;
}

static inline uint32_t grid_for(uint64_t threads, uint64_t max_blocks = 16384) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((threads + 255) / 256, max_blocks));
}

}  // namespace ctok_dev
