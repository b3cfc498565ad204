// The packed merge tiers of the 9..16 B and 17..32 B passes (kernels.hip, class_pass<16> and
// class_pass<32>), shared with the host-side check in tests (tools/merge_packed_check.cpp):
// integer code only, one builtin with a plain-C++ fallback on the host.
//
// State of one piece (narrow vocabularies whose table values all fit, Tables::short_packed), on
// ND = 8 dwords (16 slots) or ND = 16 dwords (32 slots):
//     T[ND]  tokens, 2 ND x u16: slot k in half k & 1 of dword k >> 1
//     R[ND]  values ("ranks"), 2 ND x u16: slot k holds the merge-table value of the pair
//            (token k, token k + 1), kNone (0xFFFF) when the pair has no merge or k + 1 >= m
// A step does what merge_slots<2 ND> does on 2 ND + 2 ND u32 registers: the leftmost pair of the
// lowest value merges (src/bpe.rs:118-149), the slots right of it move left by one, the two new
// pairs are looked up.  The move is one v_alignbyte per dword and a select (dword d takes its
// shifted version when its high slot lies right of the merge); L, R and the rewritten dwords come
// from ND-way dword selects on shared predicates (see step).  The 32-slot tier runs until the
// piece is at <= 16 tokens and hands its low 8 + 8 dwords to the 16-slot tier (low_half), which
// hands to the 8-slot LDS tier (lds8_key).  The arrays are only indexed with compile-time
// constants (they stay in registers) and only handled as u32 values: nothing here views storage
// through two types.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MPK_HD __host__ __device__ __forceinline__
#define MPK_UNROLL _Pragma("unroll")
#else
#define MPK_HD inline
#define MPK_UNROLL
#endif

namespace mpk {

constexpr uint32_t kNone = 0xFFFFu;  // value: no merge; token: dead slot

// (hi:lo) >> 16: the dword one slot further right
MPK_HD uint32_t shr16(uint32_t hi, uint32_t lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, 2u);
#else
  return (lo >> 16) | (hi << 16);
#endif
}
MPK_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
MPK_HD uint32_t pack2(uint32_t lo, uint32_t hi) { return (lo & 0xFFFFu) | (hi << 16); }
// a's bits where mask is set, else b's (v_bfi_b32)
MPK_HD uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }

// slot K of A (compile-time K)
template <int K, int ND>
MPK_HD uint32_t half(const uint32_t (&A)[ND]) {
  static_assert(K >= 0 && K < 2 * ND, "slot within the array");
  return (K & 1) ? A[K >> 1] >> 16 : A[K >> 1] & 0xFFFFu;
}
// min over the slots of value << 16 | slot: the lowest value, leftmost on ties (one instruction
// per slot for the key -- shift-or for the low half, and-or for the high one -- and the minimum)
template <int ND>
MPK_HD uint32_t min_key(const uint32_t (&R)[ND]) {
  uint32_t key = ~0u;
MPK_UNROLL
  for (int d = 0; d < ND; d++) {
    key = umin(key, (R[d] << 16) | (uint32_t)(2 * d));
    key = umin(key, (R[d] & 0xFFFF0000u) | (uint32_t)(2 * d + 1));
  }
  return key;
}

// One merge step on m tokens.  lk supplies the table: new_id(value) -> the merged token's id;
// start(L, nid, R, has_l, has_r) begins the lookups of (L, nid) and (nid, R); finish(rl, rr)
// returns their 16-bit values, kNone where the pair has no merge or no neighbour (the moves run
// between the two, so the device's table loads overlap them).  Returns false, state unchanged,
// when no pair can merge.
//
// With the merge at slot bi = 2D + odd (the key's low 4 or 5 bits), everything dynamic hangs on
// the ND predicates D == d and the ND bi < 2d + 1, shared by the token and the value arrays:
//   S[d]      = slots (2d + 1, 2d + 2): dword d one slot further right (v_alignbyte)
//   A[d]      = odd ? T[d] : S[d - 1], d = 0..ND: L = slot bi - 1 is the low half of A[D], R = slot
//               bi + 2 the high half of A[D + 1] -- two ND-way selects on D == d
//   tokens    dword D becomes (L, nid) when odd, (nid, R) when even; dwords right of it take S
//             (bi < 2d + 1), dwords left of it stay
//   values    dwords take their shifted version likewise; slots bi - 1 and bi then get rl and rr
//             through one bit-field insert per dword: of (rl, rr) with a full mask at dword D when
//             odd; of (rr, rl) with the low-half mask at dword D and the high-half mask at dword
//             D - 1 when even (no dword D - 1 at bi = 0, where there is no left pair either)
template <int ND, class LK>
MPK_HD bool step(uint32_t (&T)[ND], uint32_t (&R)[ND], uint32_t& m, LK& lk) {
  static_assert(ND == 8 || ND == 16, "16 or 32 slots: the slot is the key's low 4 or 5 bits");
  const uint32_t key = min_key(R);
  const uint32_t best = key >> 16, bi = key & (uint32_t)(2 * ND - 1);
  if (best == kNone) return false;
  const uint32_t nid = lk.new_id(best) & 0xFFFFu;
  const uint32_t D = bi >> 1;
  const bool odd = (bi & 1u) != 0;
  uint32_t S[ND];
MPK_UNROLL
  for (int d = 0; d < ND; d++) S[d] = shr16(d + 1 < ND ? T[d + 1] : ~0u, T[d]);
  // (the selects start from 0, not from an array element: a select between two elements is turned
  // by the compiler into a load through a selected address, which puts the array in scratch)
  uint32_t A[ND + 1];
  A[0] = odd ? T[0] : 0u;
MPK_UNROLL
  for (int d = 1; d < ND; d++) A[d] = odd ? T[d] : S[d - 1];
  A[ND] = odd ? ~0u : S[ND - 1];
  uint32_t L0 = 0, R0 = 0;
MPK_UNROLL
  for (int d = 0; d < ND; d++) {
    L0 = D == (uint32_t)d ? A[d] : L0;
    R0 = D == (uint32_t)d ? A[d + 1] : R0;
  }
  const uint32_t L = L0 & 0xFFFFu, Rt = R0 >> 16;
  const bool has_l = bi > 0, has_r = bi + 2 < m;
  lk.start(L, nid, Rt, has_l, has_r);
  const uint32_t Y = odd ? (L | (nid << 16)) : (nid | (R0 & 0xFFFF0000u));
  const uint32_t mA = odd ? 0xFFFFFFFFu : 0x0000FFFFu, mB = odd ? 0u : 0xFFFF0000u;
  uint32_t mask[ND];
MPK_UNROLL
  for (int d = 0; d < ND; d++) {  // ascending: dword d + 1 is read before it is overwritten
    const bool right = bi < (uint32_t)(2 * d + 1);
    T[d] = D == (uint32_t)d ? Y : (right ? S[d] : T[d]);
    const uint32_t sr = shr16(d + 1 < ND ? R[d + 1] : ~0u, R[d]);
    R[d] = right ? sr : R[d];
    mask[d] = D == (uint32_t)d ? mA : (D == (uint32_t)(d + 1) ? mB : 0u);
  }
  m--;
  uint32_t rl, rr;
  lk.finish(rl, rr);
  const uint32_t vv = odd ? pack2(rl, rr) : pack2(rr, rl);
MPK_UNROLL
  for (int d = 0; d < ND; d++) R[d] = bfi(mask[d], vv, R[d]);
  return true;
}

// The tier: steps until the piece is at <= stop tokens (true: the next tier continues -- the
// 16-slot one on low_half at stop = 16, the 8-slot one at stop = 8) or nothing merges (false).
template <int ND, class LK>
MPK_HD bool tier(uint32_t (&T)[ND], uint32_t (&R)[ND], uint32_t& m, uint32_t stop, LK& lk) {
  for (;;) {
    if (m <= stop) return true;
    if (!step(T, R, m, lk)) return false;
  }
}

// Hand-off from 32 to 16 slots at m <= 16: the low eight dwords of each array.  Value slot 15 is
// kNone there (slot k + 1 >= m) and the token slots >= m are never read, as the 16-slot tier expects.
MPK_HD void low_half(const uint32_t (&A)[16], uint32_t (&lo)[8]) {
MPK_UNROLL
  for (int d = 0; d < 8; d++) lo[d] = A[d];
}

// Hand-off to the 8-slot LDS tier (merge_lds8): slot K's key value << 3 | K, all ones when the
// slot starts no mergeable pair; its token is half<K>(T).
template <int K, int ND>
MPK_HD uint32_t lds8_key(const uint32_t (&R)[ND]) {
  static_assert(K < 8, "a slot of the 8-slot tier");
  const uint32_t r = half<K>(R);
  return r == kNone ? ~0u : (r << 3) | (uint32_t)K;
}

}  // namespace mpk
