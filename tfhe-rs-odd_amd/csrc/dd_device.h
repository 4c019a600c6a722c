// dd_device.h -- double-double arithmetic and the 128-bit torus conversions of the f128 PBS
// (DESIGN.md 3b).  Every function is one fixed sequence of IEEE-754 binary64 operations: the
// file is compiled with -ffp-contract=off, every fused operation is an explicit fma(), nothing is
// reassociated.  tests/pbs_ref128.c restates the same sequences in plain C; the two agree bit for bit.
//
// The reference's f128 type and butterflies live in concrete-fft (fft128/math/fft/mod.rs:5), which is
// not part of the reference tree; its conversions are (mod.rs:138-239):
//   u128_to_signed_to_f128   hi = RN(signed x), lo = RN(x - hi)                mod.rs:201-223
//   u128_from_torus_f128     x - floor(x), * 2^128, floor(x + 1/2), wrapping   mod.rs:226-239
//   f64_to_u128 / f64_to_i128  integer bit manipulation of the f64 pattern     mod.rs:162-198
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfhe_mi355 {

typedef unsigned __int128 u128;
typedef __int128 i128;

struct dd {
    double hi, lo;
};
struct cdd {
    dd re, im;
};

#define DD_FN __host__ __device__ __forceinline__ static

DD_FN double dd_bits_to_f64(uint64_t b) {
    union {
        uint64_t u;
        double d;
    } v;
    v.u = b;
    return v.d;
}
DD_FN uint64_t dd_f64_to_bits(double d) {
    union {
        uint64_t u;
        double d;
    } v;
    v.d = d;
    return v.u;
}
// 2^e for -1022 <= e <= 1023
DD_FN double dd_pow2(int e) { return dd_bits_to_f64((uint64_t)(1023 + e) << 52); }

// ---- error-free transforms -----------------------------------------------------------------------
DD_FN dd two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    const double e = (a - (s - bb)) + (b - bb);
    return {s, e};
}
// requires |a| >= |b| (or a == 0)
DD_FN dd quick_two_sum(double a, double b) {
    const double s = a + b;
    const double e = b - (s - a);
    return {s, e};
}
DD_FN dd two_prod(double a, double b) {
    const double p = a * b;
    const double e = fma(a, b, -p);
    return {p, e};
}

// ---- double-double -------------------------------------------------------------------------------
DD_FN dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
DD_FN dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return quick_two_sum(s.hi, s.lo);
}
DD_FN dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
DD_FN dd dd_add_f64(dd a, double b) {
    dd s = two_sum(a.hi, b);
    s.lo = s.lo + a.lo;
    return quick_two_sum(s.hi, s.lo);
}
DD_FN dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    const double t1 = a.hi * b.lo;
    const double t2 = a.lo * b.hi;
    const double t = t1 + t2;
    p.lo = p.lo + t;
    return quick_two_sum(p.hi, p.lo);
}
DD_FN dd dd_mul_f64(dd a, double b) {
    dd p = two_prod(a.hi, b);
    const double t = a.lo * b;
    p.lo = p.lo + t;
    return quick_two_sum(p.hi, p.lo);
}
// exact for a power of two c (no underflow at the magnitudes of the PBS)
DD_FN dd dd_scale(dd a, double c) { return {a.hi * c, a.lo * c}; }

// complex: re = ar br - ai bi, im = ai br + ar bi (ggsw.rs:591-648)
DD_FN cdd cdd_add(cdd a, cdd b) { return {dd_add(a.re, b.re), dd_add(a.im, b.im)}; }
DD_FN cdd cdd_sub(cdd a, cdd b) { return {dd_sub(a.re, b.re), dd_sub(a.im, b.im)}; }
DD_FN cdd cdd_mul(cdd a, cdd b) {
    return {dd_sub(dd_mul(a.re, b.re), dd_mul(a.im, b.im)), dd_add(dd_mul(a.im, b.re), dd_mul(a.re, b.im))};
}
DD_FN cdd cdd_conj(cdd a) { return {a.re, dd_neg(a.im)}; }

// ---- integer <-> double-double -------------------------------------------------------------------
// RN (ties to even) of a 128-bit magnitude, by integer bit manipulation
DD_FN double u128_mag_to_f64(u128 m, u128 *rounded) {
    if (m == 0) {
        *rounded = 0;
        return 0.0;
    }
    const uint64_t h = (uint64_t)(m >> 64), l = (uint64_t)m;
    const int top = h ? 127 - __builtin_clzll(h) : 63 - __builtin_clzll(l);  // index of the leading one
    if (top <= 52) {
        *rounded = m;
        return (double)(int64_t)l;  // exact
    }
    const int sh = top - 52;
    uint64_t mant = (uint64_t)(m >> sh);  // 53 bits
    const u128 rest = m & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
    if (rest > half || (rest == half && (mant & 1))) mant += 1;  // may reach 2^53: still exact below
    *rounded = (u128)mant << sh;                                // <= 2^127 for m <= 2^127
    return (double)(int64_t)mant * dd_pow2(sh);
}
// u128 -> signed -> (hi, lo), hi = RN(x), lo = RN(x - hi)
DD_FN dd u128_to_signed_dd(u128 x) {
    const bool neg = (x >> 127) != 0;
    const u128 mag = neg ? (u128)0 - x : x;  // 2^127 for x = 2^127
    u128 r, r2;
    const double hi = u128_mag_to_f64(mag, &r);
    const bool below = r > mag;  // hi rounded up: the correction is negative
    const double lo = u128_mag_to_f64(below ? r - mag : mag - r, &r2);
    const double shi = neg ? -hi : hi;
    const double slo = (neg != below) ? -lo : lo;
    return {shi, slo};
}
// wrapping truncations of |f| >= 0 (mod.rs:162-198); values >= 2^128 give 0, as the reference's shift does
DD_FN u128 f64_to_u128_wrapping(double f) {
    const uint64_t b = dd_f64_to_bits(f);
    if (b < ((uint64_t)1023 << 52)) return 0;  // [0, 1)
    if (b >> 63) return 0;                      // negative: not produced after the floor subtraction
    const u128 m = ((u128)1 << 127) | ((u128)b << 75);
    const int s = 1150 - (int)(b >> 52);
    if (s < 0 || s >= 128) return 0;
    return m >> s;
}
DD_FN u128 f64_to_i128_wrapping(double f) {
    const uint64_t b = dd_f64_to_bits(f);
    const uint64_t a = b & ~((uint64_t)1 << 63);
    if (a < ((uint64_t)1023 << 52)) return 0;
    const u128 m = ((u128)1 << 127) | ((u128)a << 75);
    const int s = 1150 - (int)(a >> 52);
    if (s < 0 || s >= 128) return 0;
    const u128 u = m >> s;
    return (b >> 63) ? (u128)0 - u : u;
}
DD_FN dd dd_floor(dd x) {
    const double f0 = floor(x.hi);
    if (f0 == x.hi) return two_sum(f0, floor(x.lo));
    return {f0, 0.0};
}
// torus fraction (any real, taken mod 1) -> u128: (x - floor x) 2^128, floor(. + 1/2), wrapping
DD_FN u128 torus128_from_dd(dd x) {
    x = dd_sub(x, dd_floor(x));
    x = dd_scale(x, dd_pow2(128));
    x = dd_floor(dd_add_f64(x, 0.5));
    return f64_to_u128_wrapping(x.hi) + f64_to_i128_wrapping(x.lo);
}

// ---- decomposer on 128-bit words (decomposer.rs:99-119, fft64/math/decomposition.rs:33-86) -------
// state of closest_representable(x) >> (128 - base_log * level)
DD_FN u128 decomp128_state(u128 x, int bl) {
    u128 st = ((x >> (127 - bl)) + 1) >> 1;
    return st & (((u128)1 << bl) - 1);
}
// one level: returns the signed digit in [-B/2, B/2], updates the state (base_log <= 31)
DD_FN int64_t decomp128_next(u128 &st, int base_log) {
    const u128 mask = ((u128)1 << base_log) - 1;
    const u128 res = st & mask;
    st >>= base_log;
    u128 carry = ((res - 1) | st) & res;
    carry >>= base_log - 1;
    st += carry;
    return (int64_t)res - (int64_t)(carry << base_log);
}
// closest_representable with base_log m, level 1: the non-native modulus 2^m (bootstrap.rs:321-334)
DD_FN u128 round_to_modulus128(u128 x, int m) {
    const int sh = 127 - m;
    return ((((x >> sh) + 1) >> 1) << 1) << sh;
}
DD_FN uint32_t pbs_modulus_switch128(u128 x, int log2n) {
    u128 o = x >> (128 - log2n - 2);
    o += 1;
    o >>= 1;
    return (uint32_t)o;  // in [0, 2N]
}

}  // namespace tfhe_mi355
