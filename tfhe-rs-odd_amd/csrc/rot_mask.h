// rot_mask.h -- sign and wrap masks of the classic PBS rotation on a negated accumulator.
//
// No HIP includes: pbs_classic.hip and the CPU checker (scripts/check_rot_mask.cpp) compile the
// same text.
//
// A wave holds polynomial positions j = lane + 64 h (h < 2V = N / 32) and keeps n = -acc
// (mod 2^64).  For a mask element a~ = full N + rem the CMUX input is
//   ct1[j] = (X^a~ acc - acc)[j] = s x - c,   x = acc[jj mod N],  jj = j - rem,  c = acc[j],
//   s = -1 iff wrap != full_odd,  wrap = jj < 0  (polynomial_wrapping_monic_monomial_mul_and_subtract).
// The gather returns y = -x and the register holds n_h = -c, so
//   s = -1:  ct1 =  y + n_h
//   s = +1:  ct1 = -y + n_h = ~(y + ~n_h)           (-v = ~v + 1, ~(a + b) = ~a + ~b + 1)
// and with m = 0xffffffff for s = +1, 0 otherwise, M = (m, m):
//   hi32(ct1) = hi32(y + (n_h ^ M)) ^ m
// -- two 32-bit xors and one 64-bit add, no conditional negate and no carry flag; the final xor
// folds into the digit's first add (v_xad_u32).
//
// jj wraps exactly for h < hcut, so the per-lane masks are one 2V-bit word per CMUX.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROT_HD __host__ __device__ __forceinline__
#else
#define ROT_HD static inline
#endif

namespace tfhe_mi355 {

// number of wrapping positions of this lane: jj = lane - rem + 64 h < 0 iff h < hcut.
// lane in [0, 64), rem in [0, N): hcut in [0, N / 32]
ROT_HD int rot_hcut(int lane, int rem) { return (63 - (lane - rem)) >> 6; }

// bit h set iff h < hcut.  hcut reaches 32 at N = 2048 (rem - lane >= 1985): the shift is 64-bit
ROT_HD uint32_t rot_wbits(int hcut) { return ~(uint32_t)(~(uint64_t)0 << hcut); }

// bit h set iff s = +1, i.e. wrap == full_odd
ROT_HD uint32_t rot_mbits(uint32_t wbits, bool full_odd) { return wbits ^ (full_odd ? 0u : ~0u); }

// bit h of mbits, sign-extended (v_bfe_i32 with immediates for a constant h)
ROT_HD uint32_t rot_mask(uint32_t mbits, int h) { return (uint32_t)((int32_t)(mbits << (31 - h)) >> 31); }

// the gather reads the buffer at jj + N (true) or jj (false)
ROT_HD bool rot_wrap(int hcut, int h) { return h < hcut; }

// hi32(s x - c) ^ m from y = -x, nh = -c: the caller applies the last xor (it folds into an add)
ROT_HD uint32_t rot_sum_hi(uint64_t y, uint64_t nh, uint32_t m) {
    const uint64_t M = ((uint64_t)m << 32) | m;
    return (uint32_t)((y + (nh ^ M)) >> 32);
}
// hi32(s x - c)
ROT_HD uint32_t rot_ct1_hi(uint64_t y, uint64_t nh, uint32_t m) { return rot_sum_hi(y, nh, m) ^ m; }

}  // namespace tfhe_mi355
