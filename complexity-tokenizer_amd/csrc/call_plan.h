// The decisions of one encode call that depend on numbers alone: list capacities from the batch
// size, the passes to launch from k_segment's report, and what the final counters mean for the
// call.  Host-only and free of HIP calls, so tools/call_plan_check.cpp tests them without a GPU;
// ctok_encode.cpp acts on them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <optional>

#include "ctok_internal.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {
using namespace ctok_dev;

// Workspace sized from what the call needs (ctok_stats.workspace_bytes): the class-0 lists lean
// (kCap0Lean per tile, the rest of a tile's class-0 pieces spill to the long list), the
// dropped-byte list small (it only fills when the vocab lacks some byte chars).  A list that
// outgrows its lean capacity sets counters[kCtrOverflow]: the call runs again with the safe
// capacities (every class-0 piece listed, a dropped-byte entry per byte).
struct Capacities {
  uint32_t k0;        // class-0 entries per tile (Work::k0)
  uint32_t unit;      // tiles per work unit of the register merge passes (Work::unit)
  uint32_t long_cap;  // long_list entries
  uint32_t mid_cap;   // mid_list (dropped-byte) entries
  uint64_t c3_limit;  // the sparse path takes class 3 when it holds at most this many pieces (0: never)
  uint32_t c3_max;    // c3q entries (Work::c3_max): c3_limit in whole shards, at most what the tiles can hold
};

// unit_knob: CTOK_UNIT (8, 16, 32 or 64, anything else: the rule); c3_knob: CTOK_C3_SPARSE (unset: the rule)
inline Capacities plan_capacities(uint64_t B, uint64_t n_tiles, bool safe, uint32_t n_at, uint32_t unit_knob,
                                  std::optional<uint64_t> c3_knob) {
  Capacities c;
  c.k0 = safe ? kCap0 : kCap0Lean;
  // merge-pass work units: 64 tiles, or 16 for batches under 8192 tiles (32 MB), which 64-tile
  // units spread over too few CUs (3.8 MB: 0.41 -> 0.30 ms per call; from 16 MB up 64 is faster,
  // profiles/r03/v16_ab_unit.txt)
  c.unit = unit_knob == 8 || unit_knob == 16 || unit_knob == 32 || unit_knob == 64 ? unit_knob
           : n_tiles >= 8192                                                        ? 64u
                                                                                    : 16u;
  c.long_cap = (uint32_t)(B / kShortMax + n_tiles + 8);
  c.mid_cap = (uint32_t)(safe ? B + 8 : std::min<uint64_t>(B + 8, std::max<uint64_t>(65536, B / 256)));
  // sparse class 3 (k_bpe_sparse): at most c3_limit pieces of 33..64 B are merged a wavefront
  // each instead of by the register pass -- by default the class is sparse at <= 1 piece per 16
  // tiles (English text: C4 ~600 in 322k tiles; C5-NFC's sub-batch of CJK-heavy documents, ~17
  // per tile, is faster in the register pass), up to kC3SparseDefault; CTOK_C3_SPARSE=n sets the
  // bound (0 disables).  k_segment queues the pieces in c3q's 64 shards (shard = tile % 64):
  // capacity the bound rounded up to whole shards, at most what a shard's tiles can hold (kCap3
  // each) -- a bound that large never overflows; a smaller one overflows when the pieces crowd
  // into a few tiles, and the call then takes the register pass (locally dense: the faster one there).
  c.c3_limit = n_at != 0 ? 0ull
               : c3_knob ? *c3_knob
                         : std::min<uint64_t>(kC3SparseDefault, std::max<uint64_t>(64, n_tiles / 16));
  const uint64_t c3_most = (uint64_t)kCap3 * ((n_tiles + kC3Shards - 1) / kC3Shards) * kC3Shards;
  c.c3_max = c.c3_limit ? (uint32_t)std::min<uint64_t>((c.c3_limit + kC3Shards - 1) / kC3Shards * kC3Shards, c3_most) : 0u;
  return c;
}

// What the host launches once the report (k_segment's counters) has arrived.  The main stream has
// run k_clear, k_tilefirst, k_segment and k_bpe_short; the side stream is ordered after k_segment
// by the report itself (no fork event) and joins the main stream once, before the tail.
struct PassPlan {
  bool spec_fail;     // nfc_watch 1 and the flag is set: the passes stop, nothing long to launch
  uint32_t n_long;    // long pieces to prepare and merge on the side stream
  uint32_t mid_wide;  // Work::mid_wide: the 17..32 B pass at 768 threads (no long pieces)
  bool folded;        // k_bpe_short took the 17..32 B class as its third pass: no k_bpe_mid<2> launch
  bool mid_side;      // the 17..32 B pass on the side stream (idle without long pieces)
  uint32_t c3n;       // class-3 pieces (all ones: a shard of c3q overflowed)
  bool c3_sparse;     // the 33..64 B class by k_bpe_sparse, not the register pass
  bool c3_side;       // that pass -- register or sparse -- on the side stream (idle again when folded)
  bool c3_long_side;  // the side instance of the 33..64 B register pass, beside the long tiers
  bool join;          // something ran on the side stream
};

// rep: the report's counters; overlap: CTOK_OVERLAP (>= 1: passes go to the idle side stream)
inline PassPlan plan_passes(const Tables& tb, const uint32_t* rep, const Capacities& cap, uint32_t nfc_watch, int overlap,
                            bool mid512, uint64_t n_tiles) {
  PassPlan p;
  const uint32_t longs = rep[kCtrLong];
  p.mid_wide = (longs == 0 && !mid512) ? 1u : 0u;
  p.spec_fail = nfc_watch == 1 && rep[kCtrNfcFlag];
  p.n_long = p.spec_fail ? 0u : std::min<uint32_t>(longs, cap.long_cap);
  p.c3n = rep[kCtrC3Count];
  p.c3_sparse = p.c3n != 0 && p.c3n <= cap.c3_limit && p.c3n <= cap.c3_max;
  // (the same decision as k_bpe_short's, from the same counter: mid_folded)
  p.folded = n_tiles && mid_folded(tb, longs);
  p.mid_side = !p.folded && overlap >= 1 && longs == 0;
  p.c3_side = p.folded && overlap >= 1 && (p.c3n != 0 || rep[kCtrAnyC3] != 0);
  p.c3_long_side = rep[kCtrAnyC3] != 0 && !p.c3_sparse;
  p.join = p.n_long || p.mid_side || p.c3_side;
  return p;
}

enum class Outcome {
  Done,
  Splice,           // finished on raw text with flagged docs: encode those again normalised (nfc_splice)
  RerunNormalised,  // a code point NFC may change: check, normalise, run again
  RerunSafe,        // a lean list overflowed: run again with the safe capacities
  ErrOverflow,      // a list overflowed its safe capacity: k_emit wrote nothing (CTOK_E_DEVICE)
  ErrPanic,         // CTOK_E_PANIC
  ErrCapacity,      // CTOK_E_CAPACITY
};

// cnt: the final counters; ntok: the call's token count
inline Outcome call_outcome(const uint32_t* cnt, uint64_t ntok, uint64_t ids_cap, uint32_t nfc_watch, bool safe,
                            uint32_t long_cap) {
  const bool flag = cnt[kCtrNfcFlag] != 0, panic = cnt[kCtrErr] & kErrPanic;
  if (nfc_watch == 1 && flag) return Outcome::RerunNormalised;
  if (cnt[kCtrOverflow] || cnt[kCtrLong] > long_cap) return safe ? Outcome::ErrOverflow : Outcome::RerunSafe;
  if (nfc_watch == 2 && flag) {
    // the pass's ids did not all fit the output, or its panic flag may come from a flagged doc's
    // raw (unnormalised) pairs, which the reference never sees (it normalises first)
    return ntok > ids_cap || panic ? Outcome::RerunNormalised : Outcome::Splice;
  }
  if (panic) return Outcome::ErrPanic;
  if (ntok > ids_cap) return Outcome::ErrCapacity;
  return Outcome::Done;
}

}  // namespace ctok_rt
