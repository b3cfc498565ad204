// Host check of an encode call's numeric decisions (csrc/call_plan.h): list capacities, the pass
// plan from k_segment's report, and the call's outcome from its final counters.  The expected
// values are written out by hand from the rules, not computed through the header.  Prints "ok" and
// exits 0, else says what differed.
//   build: g++ -O2 -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ call_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <optional>

#include "../csrc/call_plan.h"

using namespace ctok_rt;

namespace {

int g_bad = 0;

void eq(const char* what, const char* field, uint64_t got, uint64_t want) {
  if (got == want) return;
  printf("%s: %s = %llu, expected %llu\n", what, field, (unsigned long long)got, (unsigned long long)want);
  g_bad++;
}

// kTile = 3968 B, kCap0 = 3968, kCap0Lean = 1040, kCap3 = 121 per tile, 64 shards
void capacities(const char* what, uint64_t B, uint64_t nt, bool safe, uint32_t n_at, uint32_t unit_knob,
                std::optional<uint64_t> c3_knob, Capacities want) {
  const Capacities c = plan_capacities(B, nt, safe, n_at, unit_knob, c3_knob);
  eq(what, "k0", c.k0, want.k0);
  eq(what, "unit", c.unit, want.unit);
  eq(what, "long_cap", c.long_cap, want.long_cap);
  eq(what, "mid_cap", c.mid_cap, want.mid_cap);
  eq(what, "c3_limit", c.c3_limit, want.c3_limit);
  eq(what, "c3_max", c.c3_max, want.c3_max);
}

void check_capacities() {
  const std::optional<uint64_t> none;
  // no tiles: nothing fits the class-3 queue (capped by what the tiles can hold)
  capacities("B 0", 0, 0, false, 0, 0, none, {1040, 16, 8, 8, 64, 0});
  // one tile: long_cap = 100 / 32 + 1 + 8, mid_cap = B + 8, one shard row = 121 * 64 = 7744 >= 64
  capacities("1 tile", 100, 1, false, 0, 0, none, {1040, 16, 12, 108, 64, 64});
  capacities("1 tile safe", 100, 1, true, 0, 0, none, {3968, 16, 12, 108, 64, 64});
  // unit: 16 below 8192 tiles, 64 from there; B = tiles * 3968
  capacities("8191 tiles", 32501888ull, 8191, false, 0, 0, none, {1040, 16, 1023883, 126960, 511, 512});
  capacities("8192 tiles", 32505856ull, 8192, false, 0, 0, none, {1040, 64, 1024008, 126976, 512, 512});
  capacities("unit knob 8", 32505856ull, 8192, false, 0, 8, none, {1040, 8, 1024008, 126976, 512, 512});
  capacities("unit knob 7 (ignored)", 100, 1, false, 0, 7, none, {1040, 16, 12, 108, 64, 64});
  // mid_cap lean = min(B + 8, max(65536, B / 256)) on either side of B / 256 = 65536; safe = B + 8
  capacities("B/256 65535 lean", 16777215ull, 4229, false, 0, 0, none, {1040, 16, 528524, 65536, 264, 320});
  capacities("B/256 65535 safe", 16777215ull, 4229, true, 0, 0, none, {3968, 16, 528524, 16777223, 264, 320});
  capacities("B/256 65537 lean", 16777472ull, 4229, false, 0, 0, none, {1040, 16, 528533, 65537, 264, 320});
  capacities("B/256 65537 safe", 16777472ull, 4229, true, 0, 0, none, {3968, 16, 528533, 16777480, 264, 320});
  // c3_limit default = min(65536, max(64, tiles / 16))
  capacities("1023 tiles", 1023 * 3968ull, 1023, false, 0, 0, none, {1040, 16, 127883, 65536, 64, 64});
  capacities("1024 tiles", 1024 * 3968ull, 1024, false, 0, 0, none, {1040, 16, 128008, 65536, 64, 64});
  capacities("1040 tiles", 1040 * 3968ull, 1040, false, 0, 0, none, {1040, 16, 130008, 65536, 65, 128});
  {
    const Capacities c = plan_capacities(16 * 65536 * 3968ull, 16 * 65536, false, 0, 0, none);
    eq("16 * 65536 tiles", "c3_limit", c.c3_limit, 65536);
    eq("16 * 65536 tiles", "c3_max", c.c3_max, 65536);
    eq("16 * 65536 tiles", "unit", c.unit, 64);
    const Capacities d = plan_capacities((16 * 65536 + 16) * 3968ull, 16 * 65536 + 16, false, 0, 0, none);
    eq("16 * 65536 + 16 tiles", "c3_limit", d.c3_limit, 65536);
  }
  // the knob: 0 disables, 1 rounds up to a slot per shard, 10^8 is capped by kCap3 per tile of whole shard rows
  capacities("knob 0", 100, 1, false, 0, 0, 0, {1040, 16, 12, 108, 0, 0});
  capacities("knob 1", 100, 1, false, 0, 0, 1, {1040, 16, 12, 108, 1, 64});
  capacities("knob 1e8, 1 tile", 100, 1, false, 0, 0, 100000000ull, {1040, 16, 12, 108, 100000000ull, 7744});
  capacities("knob 1e8, 100 tiles", 396800, 100, false, 0, 0, 100000000ull, {1040, 16, 12508, 65536, 100000000ull, 15488});
  // added tokens in pieces: no sparse class 3, whatever the knob
  capacities("n_at 1", 100, 1, false, 1, 0, none, {1040, 16, 12, 108, 0, 0});
  capacities("n_at 1, knob 5", 100, 1, false, 1, 0, 5, {1040, 16, 12, 108, 0, 0});
}

struct Rep {
  uint32_t longs = 0, c3_count = 0, any_c3 = 0, nfc_flag = 0;
};

void passes(const char* what, const Tables& tb, Rep r, uint32_t nfc_watch, int overlap, bool mid512, uint64_t nt,
            PassPlan want) {
  // 10 tiles of text: long_cap = 39680 / 32 + 10 + 8 = 1258, c3_limit = c3_max = 64
  const Capacities cap{1040, 16, 1258, 39688, 64, 64};
  uint32_t rep[kNumCounters] = {};
  rep[0] = r.longs, rep[22] = r.c3_count, rep[20] = r.any_c3, rep[12] = r.nfc_flag;
  const PassPlan p = plan_passes(tb, rep, cap, nfc_watch, overlap, mid512, nt);
  eq(what, "spec_fail", p.spec_fail, want.spec_fail);
  eq(what, "n_long", p.n_long, want.n_long);
  eq(what, "mid_wide", p.mid_wide, want.mid_wide);
  eq(what, "folded", p.folded, want.folded);
  eq(what, "mid_side", p.mid_side, want.mid_side);
  eq(what, "c3n", p.c3n, want.c3n);
  eq(what, "c3_sparse", p.c3_sparse, want.c3_sparse);
  eq(what, "c3_side", p.c3_side, want.c3_side);
  eq(what, "c3_long_side", p.c3_long_side, want.c3_long_side);
  eq(what, "join", p.join, want.join);
}

void check_passes() {
  Tables packed{}, wide{};
  packed.narrow = packed.compact = packed.short_packed = 1;
  packed.mid_packed = 2;
  const uint32_t all = 0xFFFFFFFFu;
  // PassPlan: spec_fail, n_long, mid_wide, folded, mid_side, c3n, c3_sparse, c3_side, c3_long_side, join
  // packed table, no long piece: k_bpe_short took the 17..32 B class; the side stream only for class 3
  passes("packed", packed, {}, 0, 1, false, 10, {false, 0, 1, true, false, 0, false, false, false, false});
  passes("packed AnyC3", packed, {0, 0, 1, 0}, 0, 1, false, 10, {false, 0, 1, true, false, 0, false, true, true, true});
  passes("packed C3Count 5", packed, {0, 5, 1, 0}, 0, 1, false, 10, {false, 0, 1, true, false, 5, true, true, false, true});
  passes("packed C3Count 5, AnyC3 unset", packed, {0, 5, 0, 0}, 0, 1, false, 10,
         {false, 0, 1, true, false, 5, true, true, false, true});
  passes("packed OVERLAP=0", packed, {0, 5, 1, 0}, 0, 0, false, 10, {false, 0, 1, true, false, 5, true, false, false, false});
  passes("packed MID512", packed, {}, 0, 1, true, 10, {false, 0, 0, true, false, 0, false, false, false, false});
  // one long piece: not folded, the 17..32 B pass on the main stream at 512 threads, the side stream joins
  passes("packed 1 long", packed, {1, 0, 0, 0}, 0, 1, false, 10, {false, 1, 0, false, false, 0, false, false, false, true});
  passes("packed 1 long, AnyC3", packed, {1, 0, 1, 0}, 0, 1, false, 10,
         {false, 1, 0, false, false, 0, false, false, true, true});
  // the table has the property but added tokens can match in pieces: never folded
  {
    Tables at = packed;
    at.n_at = 1;
    passes("packed n_at", at, {}, 0, 1, false, 10, {false, 0, 1, false, true, 0, false, false, false, true});
  }
  passes("packed no tiles", packed, {}, 0, 1, false, 0, {false, 0, 1, false, true, 0, false, false, false, true});
  // wide table, no long piece: the 17..32 B pass on the idle side stream
  passes("wide", wide, {}, 0, 1, false, 10, {false, 0, 1, false, true, 0, false, false, false, true});
  passes("wide OVERLAP=0", wide, {}, 0, 0, false, 10, {false, 0, 1, false, false, 0, false, false, false, false});
  passes("wide 3 long", wide, {3, 0, 0, 0}, 0, 1, false, 10, {false, 3, 0, false, false, 0, false, false, false, true});
  passes("long past long_cap", wide, {5000, 0, 0, 0}, 0, 1, false, 10,
         {false, 1258, 0, false, false, 0, false, false, false, true});
  // class 3: sparse within the bound (the side instance of the register pass then off), register
  // pass past it or when a shard of the queue overflowed (count all ones)
  passes("C3Count 64", wide, {2, 64, 1, 0}, 0, 1, false, 10, {false, 2, 0, false, false, 64, true, false, false, true});
  passes("C3Count 65", wide, {2, 65, 1, 0}, 0, 1, false, 10, {false, 2, 0, false, false, 65, false, false, true, true});
  passes("C3Count all ones", wide, {2, all, 1, 0}, 0, 1, false, 10, {false, 2, 0, false, false, all, false, false, true, true});
  passes("packed C3Count all ones", packed, {0, all, 1, 0}, 0, 1, false, 10,
         {false, 0, 1, true, false, all, false, true, true, true});
  // NFC: watch 1 with the flag set stops the passes (nothing long to launch); watch 2 finishes them
  passes("watch 1, flag", wide, {7, 0, 0, 1}, 1, 1, false, 10, {true, 0, 0, false, false, 0, false, false, false, false});
  passes("watch 1, no flag", wide, {7, 0, 0, 0}, 1, 1, false, 10, {false, 7, 0, false, false, 0, false, false, false, true});
  passes("watch 2, flag", wide, {7, 0, 0, 1}, 2, 1, false, 10, {false, 7, 0, false, false, 0, false, false, false, true});
}

struct Fin {
  uint32_t nfc_flag = 0, overflow = 0, longs = 0, err = 0;
};

void outcome(const char* what, Fin f, uint64_t ntok, uint32_t nfc_watch, bool safe, Outcome want) {
  uint32_t cnt[kNumCounters] = {};
  cnt[12] = f.nfc_flag, cnt[25] = f.overflow, cnt[0] = f.longs, cnt[2] = f.err;
  eq(what, "outcome", (uint64_t)call_outcome(cnt, ntok, /*ids_cap=*/1000, nfc_watch, safe, /*long_cap=*/100), (uint64_t)want);
}

void check_outcome() {
  outcome("clean", {}, 1000, 0, false, Outcome::Done);
  outcome("clean, longs at the cap", {0, 0, 100, 0}, 10, 2, true, Outcome::Done);
  // 1. watch 1 and the flag: normalise and run again, whatever else happened
  outcome("watch 1, flag", {1, 0, 0, 0}, 10, 1, false, Outcome::RerunNormalised);
  outcome("watch 1, flag, overflow", {1, 1, 0, 0}, 10, 1, false, Outcome::RerunNormalised);
  outcome("watch 1, flag, overflow, safe", {1, 1, 0, 0}, 10, 1, true, Outcome::RerunNormalised);
  outcome("watch 1, flag, panic, too many ids", {1, 0, 0, 1}, 1001, 1, false, Outcome::RerunNormalised);
  // 2. a lean list overflowed: safe capacities; already safe: an error (the ids were not written)
  outcome("overflow", {0, 1, 0, 0}, 10, 0, false, Outcome::RerunSafe);
  outcome("longs past the cap", {0, 0, 101, 0}, 10, 0, false, Outcome::RerunSafe);
  outcome("overflow, panic", {0, 1, 0, 1}, 10, 0, false, Outcome::RerunSafe);
  outcome("overflow, safe", {0, 1, 0, 0}, 10, 0, true, Outcome::ErrOverflow);
  outcome("longs past the cap, safe", {0, 0, 101, 0}, 10, 0, true, Outcome::ErrOverflow);
  outcome("watch 2, flag, overflow", {1, 1, 0, 0}, 10, 2, false, Outcome::RerunSafe);
  outcome("watch 2, flag, overflow, safe", {1, 1, 0, 0}, 10, 2, true, Outcome::ErrOverflow);
  // 3. watch 2 and the flag: splice, unless the pass's ids did not fit or it panicked
  outcome("watch 2, flag", {1, 0, 0, 0}, 1000, 2, false, Outcome::Splice);
  outcome("watch 2, flag, too many ids", {1, 0, 0, 0}, 1001, 2, false, Outcome::RerunNormalised);
  outcome("watch 2, flag, panic", {1, 0, 0, 1}, 10, 2, false, Outcome::RerunNormalised);
  // 4. panic before 5. capacity
  outcome("panic", {0, 0, 0, 1}, 10, 0, false, Outcome::ErrPanic);
  outcome("panic, too many ids", {0, 0, 0, 1}, 1001, 0, false, Outcome::ErrPanic);
  outcome("watch 2, no flag, panic", {0, 0, 0, 1}, 10, 2, false, Outcome::ErrPanic);
  outcome("other error bits only", {0, 0, 0, 2}, 10, 0, false, Outcome::Done);
  outcome("too many ids", {}, 1001, 0, false, Outcome::ErrCapacity);
  outcome("watch 2, no flag, too many ids", {}, 1001, 2, true, Outcome::ErrCapacity);
}

}  // namespace

int main() {
  check_capacities();
  check_passes();
  check_outcome();
  if (g_bad) {
    printf("%d mismatches\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
