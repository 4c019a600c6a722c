// fft128_tables.cpp -- canonical twist and twiddle tables of the f128 FFT.
//
// Every entry is the double-double hi = RN(x), lo = RN(x - hi) of the exact real x = cos or sin of a
// multiple of pi / N.  They are computed in fixed point with 256 fractional bits (five 64-bit limbs, Taylor
// series at an argument <= pi/4), far above the ~160 bits at which lo could misround, so an independent
// computation at any sufficient precision (tests/pbs128_reference.py, big integers at 320 bits) gives
// the same bits.  __float128 (113 bits) would not.
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "engine.h"

namespace tfhe_mi355 {
namespace {

typedef unsigned __int128 u128;
constexpr int LIMBS = 5;  // value = sum limb[i] 2^(64 i) / 2^256: limb[4] is the integer part

struct Fx {
    uint64_t l[LIMBS];
};

Fx fx_zero() {
    Fx r;
    memset(r.l, 0, sizeof r.l);
    return r;
}
bool fx_is_zero(const Fx &a) {
    for (int i = 0; i < LIMBS; i++)
        if (a.l[i]) return false;
    return true;
}
int fx_cmp(const Fx &a, const Fx &b) {
    for (int i = LIMBS - 1; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i] ? -1 : 1;
    return 0;
}
Fx fx_add(const Fx &a, const Fx &b) {
    Fx r;
    u128 c = 0;
    for (int i = 0; i < LIMBS; i++) {
        c += (u128)a.l[i] + b.l[i];
        r.l[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
Fx fx_sub(const Fx &a, const Fx &b) {  // a >= b
    Fx r;
    uint64_t borrow = 0;
    for (int i = 0; i < LIMBS; i++) {
        const u128 d = (u128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return r;
}
Fx fx_mul(const Fx &a, const Fx &b) {  // truncated product (values below 4)
    uint64_t w[2 * LIMBS] = {0};
    for (int i = 0; i < LIMBS; i++) {
        u128 c = 0;
        for (int j = 0; j < LIMBS; j++) {
            c += (u128)a.l[i] * b.l[j] + w[i + j];
            w[i + j] = (uint64_t)c;
            c >>= 64;
        }
        w[i + LIMBS] = (uint64_t)c;
    }
    Fx r;
    for (int i = 0; i < LIMBS; i++) r.l[i] = w[i + 4];
    return r;
}
Fx fx_div_small(const Fx &a, uint64_t d) {
    Fx r;
    u128 rem = 0;
    for (int i = LIMBS - 1; i >= 0; i--) {
        const u128 cur = (rem << 64) | a.l[i];
        r.l[i] = (uint64_t)(cur / d);
        rem = cur % d;
    }
    return r;
}
Fx fx_mul_small(const Fx &a, uint64_t m) {
    Fx r;
    u128 c = 0;
    for (int i = 0; i < LIMBS; i++) {
        c += (u128)a.l[i] * m;
        r.l[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
Fx fx_shr(const Fx &a, int s) {  // 0 < s < 64
    Fx r;
    for (int i = 0; i < LIMBS; i++) r.l[i] = (a.l[i] >> s) | (i + 1 < LIMBS ? a.l[i + 1] << (64 - s) : 0);
    return r;
}

// pi = 3.243F6A88 85A308D3 13198A2E 03707344 A4093822 299F31D0 082EFA98 EC4E6C89 (hex, truncated)
const Fx FX_PI = {{0x082EFA98EC4E6C89ull, 0xA4093822299F31D0ull, 0x13198A2E03707344ull, 0x243F6A8885A308D3ull, 3ull}};

// cos and sin of x in [0, pi/4] by Taylor series, positive and negative terms summed apart
void fx_cos_sin(const Fx &x, Fx *c, Fx *s) {
    const Fx x2 = fx_mul(x, x);
    Fx one = fx_zero();
    one.l[4] = 1;
    Fx pos = one, neg = fx_zero(), term = one;
    for (uint64_t k = 1; !fx_is_zero(term); k++) {
        term = fx_div_small(fx_mul(term, x2), (2 * k - 1) * (2 * k));
        if (k & 1) neg = fx_add(neg, term);
        else pos = fx_add(pos, term);
    }
    *c = fx_sub(pos, neg);
    pos = x, neg = fx_zero(), term = x;
    for (uint64_t k = 1; !fx_is_zero(term); k++) {
        term = fx_div_small(fx_mul(term, x2), (2 * k) * (2 * k + 1));
        if (k & 1) neg = fx_add(neg, term);
        else pos = fx_add(pos, term);
    }
    *s = fx_sub(pos, neg);
}

// RN (ties to even) of a non-negative fixed-point value; *rounded receives the value of the result
double fx_round(const Fx &a, Fx *rounded) {
    *rounded = fx_zero();
    int top = -1;
    for (int i = LIMBS - 1; i >= 0 && top < 0; i--)
        if (a.l[i]) top = 64 * i + 63 - __builtin_clzll(a.l[i]);
    if (top < 0) return 0.0;
    auto bit = [&](int p) -> uint64_t { return p < 0 ? 0 : (a.l[p / 64] >> (p % 64)) & 1; };
    uint64_t mant = 0;
    for (int p = top; p > top - 53; p--) mant = (mant << 1) | bit(p);
    const int low = top - 52;  // weight of the mantissa's last bit
    bool sticky = false;
    for (int p = low - 2; p >= 0 && !sticky; p--) sticky = bit(p);
    if (bit(low - 1) && (sticky || (mant & 1))) mant += 1;
    // low > 0 for every table entry but 0 and 1 (the smallest is sin(pi/2048) > 2^-10)
    if (low >= 0) {
        const int li = low / 64, sh = low % 64;
        rounded->l[li] = mant << sh;
        if (sh && li + 1 < LIMBS) rounded->l[li + 1] = mant >> (64 - sh);
    }
    return std::ldexp((double)mant, low - 256);
}

void fx_to_dd(const Fx &a, bool negative, double *hi, double *lo) {
    Fx r, r2;
    const double h = fx_round(a, &r);
    const bool below = fx_cmp(r, a) > 0;
    const double l = fx_round(below ? fx_sub(r, a) : fx_sub(a, r), &r2);
    *hi = negative ? -h : h;
    *lo = (negative != below) ? -l : l;
}

// cos and sin of pi u / N for 0 <= u <= N as double-doubles
void unit_root(int u, int N, double *c_hi, double *c_lo, double *s_hi, double *s_lo) {
    bool cneg = false, swap = false;
    if (u > N / 2) {  // cos(pi - x) = -cos x, sin(pi - x) = sin x
        u = N - u;
        cneg = true;
    }
    if (u > N / 4) {  // cos(pi/2 - x) = sin x
        u = N / 2 - u;
        swap = true;
    }
    int log2n = 0;
    while ((1 << log2n) < N) log2n++;
    const Fx x = fx_shr(fx_mul_small(FX_PI, (uint64_t)u), log2n);
    Fx c, s;
    fx_cos_sin(x, &c, &s);
    if (swap) {
        const Fx t = c;
        c = s;
        s = t;
    }
    fx_to_dd(c, cneg, c_hi, c_lo);
    fx_to_dd(s, false, s_hi, s_lo);
}

}  // namespace

void fft128_host_tables(int N, double *twist, double *twiddles) {
    const int M = N / 2, Q = M / 2;
    for (int j = 0; j < M; j++)  // exp(i pi j / N)
        unit_root(j, N, &twist[j], &twist[M + j], &twist[2 * M + j], &twist[3 * M + j]);
    for (int t = 0; t < Q; t++) {  // exp(-2 pi i t / M) = exp(-i pi 4t / N)
        double sh, sl;
        unit_root(4 * t, N, &twiddles[t], &twiddles[Q + t], &sh, &sl);
        twiddles[2 * Q + t] = -sh;
        twiddles[3 * Q + t] = -sl;
    }
}

}  // namespace tfhe_mi355
