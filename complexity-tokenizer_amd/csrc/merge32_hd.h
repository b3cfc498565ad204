// The packed 32-slot merge tier of the 17..32 B pass (kernels.hip, class_pass<32>), shared with the
// host-side check in tests (tools/merge32_check.cpp).  It is merge16_hd.h's step on twice the
// dwords and hands over to it at <= 16 tokens:
//     T[16]  tokens, 32 x u16: slot k in half k & 1 of dword k >> 1
//     R[16]  values, 32 x u16: slot k holds the merge-table value of the pair (token k, token k + 1),
//            kNone (0xFFFF) when the pair has no merge or k + 1 >= m
// A step does what merge_slots<32> does on 32 + 32 u32 registers.  The key is value << 16 | slot
// with a 5-bit slot; the sixteen predicates D == d and the sixteen bi < 2d + 1 are shared by the
// token and the value arrays, the move is one v_alignbyte per dword, the two new values go in with
// one v_bfi per value dword, and the lookups start before the moves (see m16::step, whose comments
// apply word for word).  The arrays are only indexed with compile-time constants and only handled
// as u32 values; the selects start from 0, not from an array element.
#pragma once
#include "merge16_hd.h"

namespace m32 {

using m16::bfi;
using m16::kNone;
using m16::pack2;
using m16::shr16;
using m16::umin;

M16_HD uint32_t min_key(const uint32_t (&R)[16]) {
  uint32_t key = ~0u;
M16_UNROLL
  for (int d = 0; d < 16; d++) {
    key = umin(key, (R[d] << 16) | (uint32_t)(2 * d));
    key = umin(key, (R[d] & 0xFFFF0000u) | (uint32_t)(2 * d + 1));
  }
  return key;
}

// One merge step on m tokens; lk as in m16::step.  Returns false, state unchanged, when no pair
// can merge.
template <class LK>
M16_HD bool step(uint32_t (&T)[16], uint32_t (&R)[16], uint32_t& m, LK& lk) {
  const uint32_t key = min_key(R);
  const uint32_t best = key >> 16, bi = key & 31u;
  if (best == kNone) return false;
  const uint32_t nid = lk.new_id(best) & 0xFFFFu;
  const uint32_t D = bi >> 1;
  const bool odd = (bi & 1u) != 0;
  uint32_t S[16];
M16_UNROLL
  for (int d = 0; d < 16; d++) S[d] = shr16(d + 1 < 16 ? T[d + 1] : ~0u, T[d]);
  uint32_t A[17];
  A[0] = odd ? T[0] : 0u;
M16_UNROLL
  for (int d = 1; d < 16; d++) A[d] = odd ? T[d] : S[d - 1];
  A[16] = odd ? ~0u : S[15];
  uint32_t L0 = 0, R0 = 0;
M16_UNROLL
  for (int d = 0; d < 16; d++) {
    L0 = D == (uint32_t)d ? A[d] : L0;
    R0 = D == (uint32_t)d ? A[d + 1] : R0;
  }
  const uint32_t L = L0 & 0xFFFFu, Rt = R0 >> 16;
  const bool has_l = bi > 0, has_r = bi + 2 < m;
  lk.start(L, nid, Rt, has_l, has_r);
  const uint32_t Y = odd ? (L | (nid << 16)) : (nid | (R0 & 0xFFFF0000u));
  const uint32_t mA = odd ? 0xFFFFFFFFu : 0x0000FFFFu, mB = odd ? 0u : 0xFFFF0000u;
  uint32_t mask[16];
M16_UNROLL
  for (int d = 0; d < 16; d++) {  // ascending: dword d + 1 is read before it is overwritten
    const bool right = bi < (uint32_t)(2 * d + 1);
    T[d] = D == (uint32_t)d ? Y : (right ? S[d] : T[d]);
    const uint32_t sr = shr16(d + 1 < 16 ? R[d + 1] : ~0u, R[d]);
    R[d] = right ? sr : R[d];
    mask[d] = D == (uint32_t)d ? mA : (D == (uint32_t)(d + 1) ? mB : 0u);
  }
  m--;
  uint32_t rl, rr;
  lk.finish(rl, rr);
  const uint32_t vv = odd ? pack2(rl, rr) : pack2(rr, rl);
M16_UNROLL
  for (int d = 0; d < 16; d++) R[d] = bfi(mask[d], vv, R[d]);
  return true;
}

// The tier: steps until the piece is at <= stop tokens (true: with stop = 16 the low 8 + 8 dwords
// are m16's state, see low_half) or nothing merges (false).
template <class LK>
M16_HD bool tier(uint32_t (&T)[16], uint32_t (&R)[16], uint32_t& m, uint32_t stop, LK& lk) {
  for (;;) {
    if (m <= stop) return true;
    if (!step(T, R, m, lk)) return false;
  }
}

// Hand-off to the 16-slot tier at m <= 16: the low eight dwords of each array.  Value slot 15 is
// kNone there (slot k + 1 >= m) and the token slots >= m are never read, as m16 expects.
M16_HD void low_half(const uint32_t (&A)[16], uint32_t (&lo)[8]) {
M16_UNROLL
  for (int d = 0; d < 8; d++) lo[d] = A[d];
}

// slot K of A (compile-time K)
template <int K>
M16_HD uint32_t half(const uint32_t (&A)[16]) {
  return (K & 1) ? A[K >> 1] >> 16 : A[K >> 1] & 0xFFFFu;
}

}  // namespace m32
