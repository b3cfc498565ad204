// Host check of the packed merge tiers (csrc/merge_packed_hd.h), for N = 16 and N = 32 slots, against
// a scalar model of the register tier each replaces (kernels.hip merge_slots<N>: N + N u32 slots,
// the lowest (value, position) pair merges, the slots right of it shift left, the two new pairs
// are looked up).  Pair values come from a stub lookup.  Prints "ok" and exits 0, else says what
// differed.  Per N:
//   directed: every m in N/2 + 1 .. N x every merge position x values {0, 5, 0xFFFD, 0xFFFE} x
//             neighbours with and without a value; ties of the lowest value at every pair of
//             positions; tokens 0, 0xFFFD and 0xFFFE (the two largest ids of a narrow table, next to
//             the 0xFFFF of "none" and of dead slots)
//   random:   full merge sequences from N/2 + 1 .. N tokens down the tiers (32 slots to <= 16 tokens,
//             low_half, 16 slots to <= 8 tokens) or until nothing merges, the state compared after
//             every step, then the hand-off encoding of the 8-slot tier
//   tiers:    mpk::tier down the same hand-offs against the stepped model
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../csrc/merge_packed_hd.h"

namespace {

constexpr uint32_t kNoRank = 0x3FFFFFu;  // the u32 tiers' "no merge"
constexpr uint32_t kDead = 0xFFFFFFFFu;

// The stub table: value of pair (a, b) (< 0xFFFF) or kNoRank; new id of a value.
struct Stub {
  // one hashed pair in none_of has no value: 5 at 16 slots, 7 at 32 (this sets how deep the random
  // pieces merge, so each size keeps its own)
  explicit Stub(int slots) : none_of(slots == 16 ? 5u : 7u) {}
  uint32_t none_of;
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
    if (h % none_of == 0) return kNoRank;
    if (h % 61 == 1) return 0;
    if (h % 61 == 2) return 0xFFFEu;
    if (h % 61 == 3) return 0xFFFDu;
    return (h >> 8) % (seed % 3 == 0 ? 7u : 0xFFFFu);  // (few distinct values: many ties)
  }
  uint32_t new_id(uint32_t v) const { return compact ? v : (v * 31u + 7u) % 0xFFFFu; }
};

// merge_slots<N> on plain arrays (kernels.hip), one step; false when nothing merges.  (The same
// loop on N slots is merge_slots<N / 2> on a piece that has shrunk: the slots >= m hold kDead /
// kNoRank, so the model runs on through the hand-offs.)
template <int N>
struct Model {
  uint32_t tk[N], rk[N], m;
  bool step(const Stub& st) {
    uint32_t key = ~0u;
    for (int k = 0; k < N - 1; k++) {
      const uint32_t c = (rk[k] << 6) | (uint32_t)k;
      key = c < key ? c : key;
    }
    const uint32_t best = key >> 6, bi = key & 63u;
    if (best == kNoRank) return false;
    const uint32_t nid = st.new_id(best);
    uint32_t L = 0, R = 0;
    for (int k = 0; k < N; k++) {
      L = ((uint32_t)k + 1 == bi) ? tk[k] : L;
      R = ((uint32_t)k == bi + 2) ? tk[k] : R;
    }
    const bool has_l = bi > 0, has_r = bi + 2 < m;
    for (int k = 0; k < N; k++) {
      const uint32_t nxt_t = k + 1 < N ? tk[k + 1] : kDead;
      const uint32_t nxt_r = k + 1 < N ? rk[k + 1] : kNoRank;
      const bool gt = (uint32_t)k > bi;
      tk[k] = gt ? nxt_t : ((uint32_t)k == bi ? nid : tk[k]);
      rk[k] = gt ? nxt_r : rk[k];
    }
    m--;
    const uint32_t rl = has_l ? st.value(L, nid) : kNoRank;
    const uint32_t rr = has_r ? st.value(nid, R) : kNoRank;
    for (int k = 0; k < N - 1; k++) rk[k] = ((uint32_t)k + 1 == bi) ? rl : (((uint32_t)k == bi) ? rr : rk[k]);
    return true;
  }
};

// the lookup object of mpk::step over the stub
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

template <int N>
struct Packed {
  uint32_t T[N / 2], R[N / 2], m;
};

template <int N>
void load(const Model<N>& md, Packed<N>& pk) {
  for (int d = 0; d < N / 2; d++) {
    pk.T[d] = mpk::pack2(md.tk[2 * d], md.tk[2 * d + 1]);
    pk.R[d] = mpk::pack2(md.rk[2 * d], md.rk[2 * d + 1]);  // (kNoRank's low half is kNone)
  }
  pk.m = md.m;
}

template <int ND>
uint32_t slot_of(const uint32_t (&A)[ND], int k) { return (A[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }

int fails = 0;
template <int N, int ND>
void fail(const char* what, const Model<N>& md, const uint32_t (&T)[ND], const uint32_t (&R)[ND], uint32_t m, int k) {
  if (fails++ < 20) {
    std::fprintf(stderr, "merge_packed_check<%d>: %s at slot %d (model m=%u packed m=%u, %d packed slots)\n", N, what, k,
                 md.m, m, 2 * ND);
    for (int i = 0; i < 2 * ND; i++)
      std::fprintf(stderr, "  %2d  tok %08x / %04x   value %06x / %04x\n", i, md.tk[i], slot_of(T, i), md.rk[i], slot_of(R, i));
  }
}

// the packed state (2 * ND slots) against the model's first 2 * ND slots
template <int N, int ND>
void compare(const Model<N>& md, const uint32_t (&T)[ND], const uint32_t (&R)[ND], uint32_t m) {
  static_assert(2 * ND <= N, "the model has every packed slot");
  if (md.m != m) return fail("token count", md, T, R, m, -1);
  if (md.m > 2u * ND) return fail("more tokens than slots", md, T, R, m, -1);
  for (int k = 0; k < 2 * ND; k++) {
    if ((uint32_t)k < md.m && slot_of(T, k) != md.tk[k]) return fail("token", md, T, R, m, k);
    const uint32_t want = (uint32_t)k + 1 < md.m ? (md.rk[k] & 0xFFFFu) : mpk::kNone;  // dead values stay kNone
    if (slot_of(R, k) != want) return fail("value", md, T, R, m, k);
    if ((uint32_t)k + 1 < md.m && md.rk[k] != kNoRank && md.rk[k] >= 0xFFFFu) return fail("model value range", md, T, R, m, k);
  }
}
template <int N>
void compare(const Model<N>& md, const Packed<N>& pk) { compare(md, pk.T, pk.R, pk.m); }

template <int K, int N>
void handoff8_slot(const Model<N>& md, const uint32_t (&T)[8], const uint32_t (&R)[8], uint32_t m) {
  // merge_lds8's key of slot K from u32 state: value << 3 | K, dead / last slots all ones; a
  // key >= kNoRank << 3 means "no merge" to it, whatever its low bits
  const uint32_t want = (uint32_t)K + 1 < md.m ? (md.rk[K] << 3) | (uint32_t)K : ~0u;
  const uint32_t got = mpk::lds8_key<K>(R);
  const bool none = want >= (kNoRank << 3);
  if (none ? got != ~0u : got != want) fail("hand-off key", md, T, R, m, K);
  if ((uint32_t)K < md.m && mpk::half<K>(T) != md.tk[K]) fail("hand-off token", md, T, R, m, K);
}
template <int N>
void handoff8(const Model<N>& md, const uint32_t (&T)[8], const uint32_t (&R)[8], uint32_t m) {
  handoff8_slot<0>(md, T, R, m); handoff8_slot<1>(md, T, R, m); handoff8_slot<2>(md, T, R, m); handoff8_slot<3>(md, T, R, m);
  handoff8_slot<4>(md, T, R, m); handoff8_slot<5>(md, T, R, m); handoff8_slot<6>(md, T, R, m); handoff8_slot<7>(md, T, R, m);
}

// one step of both from the model's state; the results must agree, and so must the next tier's
// view of the state once the piece fits it
template <int N>
void one_step(Model<N> md, const Stub& st) {
  Packed<N> pk;
  load(md, pk);
  compare(md, pk);
  StubLk lk{st};
  const bool a = md.step(st);
  const bool b = mpk::step(pk.T, pk.R, pk.m, lk);
  if (a != b) return fail("merged / stopped", md, pk.T, pk.R, pk.m, -1);
  compare(md, pk);
  if constexpr (N == 32) {
    if (md.m <= 16) {  // the hand-off state is the 16-slot tier's
      uint32_t T8[8], R8[8];
      mpk::low_half(pk.T, T8);
      mpk::low_half(pk.R, R8);
      compare(md, T8, R8, pk.m);
    }
  } else {
    if (md.m <= 8) handoff8(md, pk.T, pk.R, pk.m);
  }
}

uint32_t rng_state;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

template <int N>
void fill_tokens(Model<N>& md, uint32_t m, int variant) {
  static const uint32_t special[4] = {0u, 0xFFFEu, 0xFFFDu, 0x8000u};
  md.m = m;
  for (uint32_t k = 0; k < N; k++) {
    uint32_t v = variant == 0 ? 100u + k : variant == 1 ? special[(k + m) & 3] : rnd() % 0xFFFFu;
    md.tk[k] = k < m ? v : kDead;
    md.rk[k] = kNoRank;
  }
}

template <int N>
void directed() {
  static const uint32_t lows[4] = {0u, 5u, 0xFFFDu, 0xFFFEu};
  for (uint32_t m = N / 2 + 1; m <= N; m++)
    for (int variant = 0; variant < 3; variant++)
      for (int mode = 0; mode < 5; mode++)
        for (uint32_t low : lows)
          for (int others = 0; others < 2; others++) {  // 0: the other pairs have no value; 1: higher values
            if (others == 1 && low == 0xFFFEu) continue;
            Stub st(N);
            st.mode = mode;
            st.seed = m * 7 + (uint32_t)variant;
            st.compact = (m + (uint32_t)mode) & 1;
            // the lowest value at p alone, and at p and q (leftmost must win)
            for (uint32_t p = 0; p + 1 < m; p++)
              for (uint32_t q = p; q + 1 < m; q++) {
                Model<N> md;
                fill_tokens(md, m, variant);
                for (uint32_t k = 0; k + 1 < m; k++)
                  md.rk[k] = others ? low + 1 + (k * 37u) % (0xFFFEu - low) : kNoRank;
                md.rk[p] = low;
                md.rk[q] = low;
                one_step(md, st);
              }
            // nothing merges
            Model<N> md;
            fill_tokens(md, m, variant);
            one_step(md, st);
          }
}

// Steps on 2 ND slots down to <= ND tokens, compared after each, then the next tier: the low halves
// on 16 slots, or the 8-slot tier's keys.  Ends where nothing merges, or at the first mismatch.
template <int N, int ND>
void step_down(Model<N>& md, uint32_t (&T)[ND], uint32_t (&R)[ND], uint32_t m, const Stub& st, StubLk& lk) {
  for (;;) {
    compare(md, T, R, m);
    if (fails) return;
    if (md.m <= (uint32_t)ND) break;
    const bool a = md.step(st);
    const bool b = mpk::step(T, R, m, lk);
    if (a != b) return fail("merged / stopped", md, T, R, m, -1);
    if (!a) return;
  }
  if constexpr (ND == 16) {
    uint32_t T8[8], R8[8];
    mpk::low_half(T, T8);
    mpk::low_half(R, R8);
    step_down(md, T8, R8, m, st, lk);
  } else {
    handoff8(md, T, R, m);
  }
}

template <int N>
void random_runs(int runs) {
  for (int it = 0; it < runs; it++) {
    Stub st(N);
    st.seed = rnd();
    st.compact = rnd() & 1;
    Model<N> md;
    const uint32_t m = N / 2 + 1 + rnd() % (N / 2);
    const uint32_t alpha = 1 + rnd() % 6;  // small alphabets: periodic strings, repeated equal pairs
    md.m = m;
    for (uint32_t k = 0; k < N; k++) {
      const uint32_t v = (it & 1) ? rnd() % alpha : (k % alpha);
      md.tk[k] = k < m ? (v == 0 ? 0u : v == 1 ? 0xFFFEu : v == 2 ? 0xFFFDu : v * 1000u) : kDead;
    }
    for (uint32_t k = 0; k < N; k++) md.rk[k] = k + 1 < m ? st.value(md.tk[k], md.tk[k + 1]) : kNoRank;
    Packed<N> pk;
    load(md, pk);
    StubLk lk{st};
    step_down(md, pk.T, pk.R, pk.m, st, lk);
    if (fails) return;
  }
}

// mpk::tier on 2 ND slots against the stepped model, then the next tier as in step_down
template <int N, int ND>
void tier_down(Model<N>& md, uint32_t (&T)[ND], uint32_t (&R)[ND], uint32_t m, const Stub& st, StubLk& lk) {
  const bool more = mpk::tier(T, R, m, (uint32_t)ND, lk);
  bool more_md = true;
  while (md.m > (uint32_t)ND && (more_md = md.step(st))) {}
  if (more != more_md) return fail("tier result", md, T, R, m, -1);
  compare(md, T, R, m);
  if (fails || !more) return;
  if constexpr (ND == 16) {
    uint32_t T8[8], R8[8];
    mpk::low_half(T, T8);
    mpk::low_half(R, R8);
    tier_down(md, T8, R8, m, st, lk);
  } else {
    handoff8(md, T, R, m);
  }
}

template <int N>
void tier_runs(int runs) {
  for (int it = 0; it < runs; it++) {
    Stub st(N);
    st.seed = rnd();
    Model<N> md;
    md.m = N / 2 + 1 + rnd() % (N / 2);
    const uint32_t hi = (it & 1) ? 0xFFFBu : 3u;  // tokens 3..6, or the four largest ids 0xFFFB..0xFFFE
    for (uint32_t k = 0; k < N; k++) md.tk[k] = k < md.m ? hi + rnd() % 4 : kDead;
    for (uint32_t k = 0; k < N; k++) md.rk[k] = k + 1 < md.m ? st.value(md.tk[k], md.tk[k + 1]) : kNoRank;
    Packed<N> pk;
    load(md, pk);
    StubLk lk{st};
    tier_down(md, pk.T, pk.R, pk.m, st, lk);
    if (fails) return;
  }
}

template <int N>
void check() {
  rng_state = 12345;  // each size draws the same sequence whatever ran before it
  directed<N>();
  random_runs<N>(20000);
  tier_runs<N>(5000);
}

}  // namespace

int main() {
  check<16>();
  check<32>();
  if (fails) {
    std::fprintf(stderr, "merge_packed_check: %d mismatches\n", fails);
    return 1;
  }
  std::puts("ok");
  return 0;
}
