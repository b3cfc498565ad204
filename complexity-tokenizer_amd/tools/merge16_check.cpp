// Host check of the packed 16-slot merge tier (csrc/merge16_hd.h) against a scalar model of the
// register tier it replaces (kernels.hip merge_slots<16>: 16 + 16 u32 slots, the lowest
// (value, position) pair merges, the slots right of it shift left, the two new pairs are looked
// up).  Pair values come from a stub lookup.  Prints "ok" and exits 0, else says what differed.
//   directed: every m in 9..16 x every merge position x values {0, 5, 0xFFFD, 0xFFFE} x neighbours
//             with and without a value; ties of the lowest value at every pair of positions; tokens
//             0, 0xFFFD and 0xFFFE (the two largest ids of a narrow table, next to the 0xFFFF of
//             "none" and of dead slots)
//   random:   full merge sequences from 9..16 tokens down to <= 8 (or until nothing merges), the
//             state compared after every step, then the hand-off encoding of the 8-slot tier
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../csrc/merge16_hd.h"

namespace {

constexpr uint32_t kNoRank = 0x3FFFFFu;  // the u32 tiers' "no merge"
constexpr uint32_t kDead = 0xFFFFFFFFu;

// The stub table: value of pair (a, b) (< 0xFFFF) or kNoRank; new id of a value.
struct Stub {
  uint32_t seed = 0;
  int mode = 0;  // 0: hashed values; 1: every pair none; 2: every pair value 0; 3: every pair 0xFFFE; 4: 0xFFFD
  bool compact = true;
  uint32_t value(uint32_t a, uint32_t b) const {
    if (mode == 1) return kNoRank;
    if (mode == 2) return 0;
    if (mode == 3) return 0xFFFEu;
    if (mode == 4) return 0xFFFDu;
    uint32_t h = (a * 0x9E3779B1u) ^ (b * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
    h ^= h >> 15;
    h *= 0x27D4EB2Fu;
    h ^= h >> 13;
    if (h % 5 == 0) return kNoRank;
    if (h % 61 == 1) return 0;
    if (h % 61 == 2) return 0xFFFEu;
    if (h % 61 == 3) return 0xFFFDu;
    return (h >> 8) % (seed % 3 == 0 ? 7u : 0xFFFFu);  // (few distinct values: many ties)
  }
  uint32_t new_id(uint32_t v) const { return compact ? v : (v * 31u + 7u) % 0xFFFFu; }
};

// merge_slots<16> on plain arrays (kernels.hip), one step; false when nothing merges
struct Model {
  uint32_t tk[16], rk[16], m;
  bool step(const Stub& st) {
    uint32_t key = ~0u;
    for (int k = 0; k < 15; k++) {
      const uint32_t c = (rk[k] << 6) | (uint32_t)k;
      key = c < key ? c : key;
    }
    const uint32_t best = key >> 6, bi = key & 63u;
    if (best == kNoRank) return false;
    const uint32_t nid = st.new_id(best);
    uint32_t L = 0, R = 0;
    for (int k = 0; k < 16; k++) {
      L = ((uint32_t)k + 1 == bi) ? tk[k] : L;
      R = ((uint32_t)k == bi + 2) ? tk[k] : R;
    }
    const bool has_l = bi > 0, has_r = bi + 2 < m;
    for (int k = 0; k < 16; k++) {
      const uint32_t nxt_t = k + 1 < 16 ? tk[k + 1] : kDead;
      const uint32_t nxt_r = k + 1 < 16 ? rk[k + 1] : kNoRank;
      const bool gt = (uint32_t)k > bi;
      tk[k] = gt ? nxt_t : ((uint32_t)k == bi ? nid : tk[k]);
      rk[k] = gt ? nxt_r : rk[k];
    }
    m--;
    const uint32_t rl = has_l ? st.value(L, nid) : kNoRank;
    const uint32_t rr = has_r ? st.value(nid, R) : kNoRank;
    for (int k = 0; k < 15; k++) rk[k] = ((uint32_t)k + 1 == bi) ? rl : (((uint32_t)k == bi) ? rr : rk[k]);
    return true;
  }
};

// the lookup object of m16::step over the stub
struct StubLk {
  const Stub& st;
  uint32_t l = 0, n = 0, r = 0;
  bool hl = false, hr = false;
  uint32_t new_id(uint32_t v) const { return st.new_id(v); }
  void start(uint32_t L, uint32_t nid, uint32_t R, bool has_l, bool has_r) {
    l = L; n = nid; r = R; hl = has_l; hr = has_r;
  }
  void finish(uint32_t& rl, uint32_t& rr) const {
    rl = (hl ? st.value(l, n) : kNoRank) & 0xFFFFu;
    rr = (hr ? st.value(n, r) : kNoRank) & 0xFFFFu;
  }
};

struct Packed {
  uint32_t T[8], R[8], m;
};

void load(const Model& md, Packed& pk) {
  for (int d = 0; d < 8; d++) {
    pk.T[d] = m16::pack2(md.tk[2 * d], md.tk[2 * d + 1]);
    pk.R[d] = m16::pack2(md.rk[2 * d], md.rk[2 * d + 1]);  // (kNoRank's low half is kNone)
  }
  pk.m = md.m;
}

int fails = 0;
void fail(const char* what, const Model& md, const Packed& pk, int k) {
  if (fails++ < 20) {
    std::fprintf(stderr, "merge16_check: %s at slot %d (model m=%u packed m=%u)\n", what, k, md.m, pk.m);
    for (int i = 0; i < 16; i++)
      std::fprintf(stderr, "  %2d  tok %08x / %04x   value %06x / %04x\n", i, md.tk[i],
                   (pk.T[i >> 1] >> (16 * (i & 1))) & 0xFFFFu, md.rk[i], (pk.R[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
  }
}

uint32_t slot_of(const uint32_t (&A)[8], int k) { return (A[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }

void compare(const Model& md, const Packed& pk) {
  if (md.m != pk.m) return fail("token count", md, pk, -1);
  for (int k = 0; k < 16; k++) {
    if ((uint32_t)k < md.m && slot_of(pk.T, k) != md.tk[k]) return fail("token", md, pk, k);
    const uint32_t want = (uint32_t)k + 1 < md.m ? (md.rk[k] & 0xFFFFu) : m16::kNone;  // dead values stay kNone
    if (slot_of(pk.R, k) != want) return fail("value", md, pk, k);
    if ((uint32_t)k + 1 < md.m && md.rk[k] != kNoRank && md.rk[k] >= 0xFFFFu) return fail("model value range", md, pk, k);
  }
}

template <int K>
void handoff_slot(const Model& md, const Packed& pk) {
  // merge_lds8's key of slot K from u32 state: value << 3 | K, dead / last slots all ones; a
  // key >= kNoRank << 3 means "no merge" to it, whatever its low bits
  const uint32_t want = (uint32_t)K + 1 < md.m ? (md.rk[K] << 3) | (uint32_t)K : ~0u;
  const uint32_t got = m16::lds8_key<K>(pk.R);
  const bool none = want >= (kNoRank << 3);
  if (none ? got != ~0u : got != want) fail("hand-off key", md, pk, K);
  if ((uint32_t)K < md.m && m16::half<K>(pk.T) != md.tk[K]) fail("hand-off token", md, pk, K);
}
void handoff(const Model& md, const Packed& pk) {
  handoff_slot<0>(md, pk); handoff_slot<1>(md, pk); handoff_slot<2>(md, pk); handoff_slot<3>(md, pk);
  handoff_slot<4>(md, pk); handoff_slot<5>(md, pk); handoff_slot<6>(md, pk); handoff_slot<7>(md, pk);
}

// one step of both from the model's state; the results must agree
void one_step(Model md, const Stub& st) {
  Packed pk;
  load(md, pk);
  compare(md, pk);
  StubLk lk{st};
  const bool a = md.step(st);
  const bool b = m16::step(pk.T, pk.R, pk.m, lk);
  if (a != b) return fail("merged / stopped", md, pk, -1);
  compare(md, pk);
  if (md.m <= 8) handoff(md, pk);
}

uint32_t rng_state = 12345;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

void fill_tokens(Model& md, uint32_t m, int variant) {
  static const uint32_t special[4] = {0u, 0xFFFEu, 0xFFFDu, 0x8000u};
  md.m = m;
  for (uint32_t k = 0; k < 16; k++) {
    uint32_t v = variant == 0 ? 100u + k : variant == 1 ? special[(k + m) & 3] : rnd() % 0xFFFFu;
    md.tk[k] = k < m ? v : kDead;
    md.rk[k] = kNoRank;
  }
}

void directed() {
  static const uint32_t lows[4] = {0u, 5u, 0xFFFDu, 0xFFFEu};
  for (uint32_t m = 9; m <= 16; m++)
    for (int variant = 0; variant < 3; variant++)
      for (int mode = 0; mode < 5; mode++)
        for (uint32_t low : lows)
          for (int others = 0; others < 2; others++) {  // 0: the other pairs have no value; 1: higher values
            if (others == 1 && low == 0xFFFEu) continue;
            Stub st;
            st.mode = mode;
            st.seed = m * 7 + (uint32_t)variant;
            st.compact = (m + (uint32_t)mode) & 1;
            // the lowest value at p alone, and at p and q (leftmost must win)
            for (uint32_t p = 0; p + 1 < m; p++)
              for (uint32_t q = p; q + 1 < m; q++) {
                Model md;
                fill_tokens(md, m, variant);
                for (uint32_t k = 0; k + 1 < m; k++)
                  md.rk[k] = others ? low + 1 + (k * 37u) % (0xFFFEu - low) : kNoRank;
                md.rk[p] = low;
                md.rk[q] = low;
                one_step(md, st);
              }
            // nothing merges
            Model md;
            fill_tokens(md, m, variant);
            one_step(md, st);
          }
}

void random_runs(int runs) {
  for (int it = 0; it < runs; it++) {
    Stub st;
    st.seed = rnd();
    st.compact = rnd() & 1;
    Model md;
    const uint32_t m = 9 + rnd() % 8;
    const uint32_t alpha = 1 + rnd() % 6;  // small alphabets: periodic strings, repeated equal pairs
    md.m = m;
    for (uint32_t k = 0; k < 16; k++) {
      const uint32_t v = (it & 1) ? rnd() % alpha : (k % alpha);
      md.tk[k] = k < m ? (v == 0 ? 0u : v == 1 ? 0xFFFEu : v == 2 ? 0xFFFDu : v * 1000u) : kDead;
    }
    for (uint32_t k = 0; k < 16; k++) md.rk[k] = k + 1 < m ? st.value(md.tk[k], md.tk[k + 1]) : kNoRank;
    Packed pk;
    load(md, pk);
    StubLk lk{st};
    for (;;) {
      compare(md, pk);
      if (fails) return;
      if (md.m <= 8) break;
      const bool a = md.step(st);
      const bool b = m16::step(pk.T, pk.R, pk.m, lk);
      if (a != b) return fail("merged / stopped", md, pk, -1);
      if (!a) break;
    }
    if (md.m <= 8) handoff(md, pk);
  }
}

void tier_runs(int runs) {  // m16::tier against the stepped model
  for (int it = 0; it < runs; it++) {
    Stub st;
    st.seed = rnd();
    Model md;
    md.m = 9 + rnd() % 8;
    const uint32_t hi = (it & 1) ? 0xFFFBu : 3u;  // tokens 3..6, or the four largest ids 0xFFFB..0xFFFE
    for (uint32_t k = 0; k < 16; k++) md.tk[k] = k < md.m ? hi + rnd() % 4 : kDead;
    for (uint32_t k = 0; k < 16; k++) md.rk[k] = k + 1 < md.m ? st.value(md.tk[k], md.tk[k + 1]) : kNoRank;
    Packed pk;
    load(md, pk);
    StubLk lk{st};
    const bool more = m16::tier(pk.T, pk.R, pk.m, 8, lk);
    bool more_md = true;
    while (md.m > 8 && (more_md = md.step(st))) {}
    if (more != more_md) return fail("tier result", md, pk, -1);
    compare(md, pk);
    if (fails) return;
  }
}

}  // namespace

int main() {
  directed();
  random_runs(20000);
  tier_runs(5000);
  if (fails) {
    std::fprintf(stderr, "merge16_check: %d mismatches\n", fails);
    return 1;
  }
  std::puts("ok");
  return 0;
}
