/* pbs_ref128.c -- CPU restatement of the 128-bit-torus PBS, test infrastructure.
 *
 * Plain C, built by tests/pbs128_reference.py with -O2 -std=gnu11 -ffp-contract=off -mfma -fopenmp.  It
 * shares no code with the engine: it restates the double-double primitives, conversions, the radix-2
 * transform, the MAC order, the decomposer, the modulus switch and the sample extraction of DESIGN.md 3b
 * operation for operation, and takes the twist and twiddle tables as data from Python.  It also holds the
 * exact arithmetic the tests compare against (negacyclic product and CMUX over Z/2^128) and a small
 * client (binary keys, GGSW rows, Gaussian noise scaled to 2^128, a seeded PRNG of its own).
 *
 * A u128 word is unsigned __int128 (two little-endian uint64_t: low, high). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned __int128 u128;
typedef struct { double hi, lo; } dd;
typedef struct { dd re, im; } cdd;

static double bits_f64(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t f64_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static double pow2(int e) { return bits_f64((uint64_t)(1023 + e) << 52); }

/* ---- double-double (every fused operation is an explicit fma) ---- */
static dd two_sum(double a, double b) {
    double s = a + b;
    double bb = s - a;
    double e = (a - (s - bb)) + (b - bb);
    return (dd){s, e};
}
static dd quick_two_sum(double a, double b) {
    double s = a + b;
    double e = b - (s - a);
    return (dd){s, e};
}
static dd two_prod(double a, double b) {
    double p = a * b;
    double e = fma(a, b, -p);
    return (dd){p, e};
}
static dd dd_neg(dd a) { return (dd){-a.hi, -a.lo}; }
static dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    dd t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return quick_two_sum(s.hi, s.lo);
}
static dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
static dd dd_add_f64(dd a, double b) {
    dd s = two_sum(a.hi, b);
    s.lo = s.lo + a.lo;
    return quick_two_sum(s.hi, s.lo);
}
static dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    double t1 = a.hi * b.lo;
    double t2 = a.lo * b.hi;
    double t = t1 + t2;
    p.lo = p.lo + t;
    return quick_two_sum(p.hi, p.lo);
}
static dd dd_mul_f64(dd a, double b) {
    dd p = two_prod(a.hi, b);
    double t = a.lo * b;
    p.lo = p.lo + t;
    return quick_two_sum(p.hi, p.lo);
}
static dd dd_scale(dd a, double c) { return (dd){a.hi * c, a.lo * c}; }
static cdd cdd_add(cdd a, cdd b) { return (cdd){dd_add(a.re, b.re), dd_add(a.im, b.im)}; }
static cdd cdd_sub(cdd a, cdd b) { return (cdd){dd_sub(a.re, b.re), dd_sub(a.im, b.im)}; }
static cdd cdd_mul(cdd a, cdd b) {
    return (cdd){dd_sub(dd_mul(a.re, b.re), dd_mul(a.im, b.im)), dd_add(dd_mul(a.im, b.re), dd_mul(a.re, b.im))};
}
static cdd cdd_conj(cdd a) { return (cdd){a.re, dd_neg(a.im)}; }

/* ---- conversions ---- */
static double mag_to_f64(u128 m, u128 *rounded) {
    if (m == 0) { *rounded = 0; return 0.0; }
    uint64_t h = (uint64_t)(m >> 64), l = (uint64_t)m;
    int top = h ? 127 - __builtin_clzll(h) : 63 - __builtin_clzll(l);
    if (top <= 52) { *rounded = m; return (double)(int64_t)l; }
    int sh = top - 52;
    uint64_t mant = (uint64_t)(m >> sh);
    u128 rest = m & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
    if (rest > half || (rest == half && (mant & 1))) mant += 1;
    *rounded = (u128)mant << sh;
    return (double)(int64_t)mant * pow2(sh);
}
static dd to_signed_dd(u128 x) {
    int neg = (int)(x >> 127);
    u128 mag = neg ? (u128)0 - x : x, r, r2;
    double hi = mag_to_f64(mag, &r);
    int below = r > mag;
    double lo = mag_to_f64(below ? r - mag : mag - r, &r2);
    return (dd){neg ? -hi : hi, (neg != below) ? -lo : lo};
}
static u128 f64_to_u128w(double f) {
    uint64_t b = f64_bits(f);
    if (b < ((uint64_t)1023 << 52)) return 0;
    if (b >> 63) return 0;
    u128 m = ((u128)1 << 127) | ((u128)b << 75);
    int s = 1150 - (int)(b >> 52);
    if (s < 0 || s >= 128) return 0;
    return m >> s;
}
static u128 f64_to_i128w(double f) {
    uint64_t b = f64_bits(f), a = b & ~((uint64_t)1 << 63);
    if (a < ((uint64_t)1023 << 52)) return 0;
    u128 m = ((u128)1 << 127) | ((u128)a << 75);
    int s = 1150 - (int)(a >> 52);
    if (s < 0 || s >= 128) return 0;
    u128 u = m >> s;
    return (b >> 63) ? (u128)0 - u : u;
}
static dd dd_floor(dd x) {
    double f0 = floor(x.hi);
    if (f0 == x.hi) return two_sum(f0, floor(x.lo));
    return (dd){f0, 0.0};
}
static u128 torus_from_dd(dd x) {
    x = dd_sub(x, dd_floor(x));
    x = dd_scale(x, pow2(128));
    x = dd_floor(dd_add_f64(x, 0.5));
    return f64_to_u128w(x.hi) + f64_to_i128w(x.lo);
}

/* ---- decomposer, modulus switch ---- */
static u128 decomp_state(u128 x, int bl) {
    u128 st = ((x >> (127 - bl)) + 1) >> 1;
    return st & (((u128)1 << bl) - 1);
}
static int64_t decomp_next(u128 *st, int base_log) {
    u128 mask = ((u128)1 << base_log) - 1;
    u128 res = *st & mask;
    *st >>= base_log;
    u128 carry = ((res - 1) | *st) & res;
    carry >>= base_log - 1;
    *st += carry;
    return (int64_t)res - (int64_t)(carry << base_log);
}
static u128 closest_representable(u128 x, int base_log, int level) {
    int sh = 127 - base_log * level;
    return ((((x >> sh) + 1) >> 1) << 1) << sh;
}
static uint32_t modulus_switch(u128 x, int log2n) {
    u128 o = x >> (128 - log2n - 2);
    o += 1;
    o >>= 1;
    return (uint32_t)o;
}

/* ---- transform on an array of M complex double-doubles; tables as 4 planes ---- */
static cdd plane_get(const double *p, int M, int i) { return (cdd){{p[i], p[M + i]}, {p[2 * M + i], p[3 * M + i]}}; }

static void fft_forward(cdd *s, int M, const double *tw) {
    for (int h = M / 2; h >= 1; h >>= 1) {
        int step = M / (2 * h);
        for (int b = 0; b < M / 2; b++) {
            int j = b & (h - 1);
            int i0 = ((b - j) << 1) + j, i1 = i0 + h;
            cdd x = s[i0], y = s[i1];
            s[i0] = cdd_add(x, y);
            s[i1] = cdd_mul(cdd_sub(x, y), plane_get(tw, M / 2, j * step));
        }
    }
}
static void fft_inverse(cdd *s, int M, const double *tw) {
    for (int h = 1; h <= M / 2; h <<= 1) {
        int step = M / (2 * h);
        for (int b = 0; b < M / 2; b++) {
            int j = b & (h - 1);
            int i0 = ((b - j) << 1) + j, i1 = i0 + h;
            cdd x = s[i0];
            cdd t = cdd_mul(s[i1], cdd_conj(plane_get(tw, M / 2, j * step)));
            s[i0] = cdd_add(x, t);
            s[i1] = cdd_sub(x, t);
        }
    }
}
static void forward_torus(const u128 *poly, int N, const double *twist, const double *tw, cdd *out) {
    int M = N / 2;
    double norm = pow2(-128);
    for (int j = 0; j < M; j++) {
        cdd z = {dd_scale(to_signed_dd(poly[j]), norm), dd_scale(to_signed_dd(poly[j + M]), norm)};
        out[j] = cdd_mul(z, plane_get(twist, M, j));
    }
    fft_forward(out, M, tw);
}
static void forward_integer(const double *re, const double *im, int N, const double *twist, const double *tw,
                            cdd *out) {
    int M = N / 2;
    for (int j = 0; j < M; j++) {
        cdd w = plane_get(twist, M, j);
        out[j] = (cdd){dd_sub(dd_mul_f64(w.re, re[j]), dd_mul_f64(w.im, im[j])),
                       dd_add(dd_mul_f64(w.re, im[j]), dd_mul_f64(w.im, re[j]))};
    }
    fft_forward(out, M, tw);
}
/* poly += backward(spectrum); the spectrum is destroyed */
static void add_backward(cdd *s, int N, const double *twist, const double *tw, u128 *poly) {
    int M = N / 2;
    double inv_m = 1.0 / (double)M;
    fft_inverse(s, M, tw);
    for (int j = 0; j < M; j++) {
        cdd z = cdd_mul(s[j], cdd_conj(plane_get(twist, M, j)));
        poly[j] += torus_from_dd(dd_scale(z.re, inv_m));
        poly[j + M] += torus_from_dd(dd_scale(z.im, inv_m));
    }
}

/* ---- exported: conversions and transform pieces for the CPU tests ---- */
void ref128_to_signed_dd(const u128 *x, double *hi, double *lo, long n) {
    for (long i = 0; i < n; i++) { dd v = to_signed_dd(x[i]); hi[i] = v.hi; lo[i] = v.lo; }
}
void ref128_torus_from_f128(const double *hi, const double *lo, const u128 *acc, u128 *out, long n) {
    for (long i = 0; i < n; i++) out[i] = (acc ? acc[i] : (u128)0) + torus_from_dd((dd){hi[i], lo[i]});
}
void ref128_decompose(const u128 *x, long n, int base_log, int level, int64_t *digits /* [level][n], L first */,
                      u128 *closest) {
    for (long i = 0; i < n; i++) {
        closest[i] = closest_representable(x[i], base_log, level);
        u128 st = decomp_state(x[i], base_log * level);
        for (int l = 0; l < level; l++) digits[(long)l * n + i] = decomp_next(&st, base_log);
    }
}
/* forward torus transform and back: out = round trip of poly */
void ref128_roundtrip(const u128 *poly, int N, const double *twist, const double *tw, u128 *out) {
    cdd *s = malloc(sizeof(cdd) * (N / 2));
    forward_torus(poly, N, twist, tw, s);
    memset(out, 0, sizeof(u128) * N);
    add_backward(s, N, twist, tw, out);
    free(s);
}
/* out = torus poly * small signed integer poly through the transform */
void ref128_fft_product(const u128 *torus, const int64_t *integer, int N, const double *twist, const double *tw,
                        u128 *out) {
    int M = N / 2;
    cdd *a = malloc(sizeof(cdd) * M), *b = malloc(sizeof(cdd) * M);
    double *re = malloc(sizeof(double) * M), *im = malloc(sizeof(double) * M);
    for (int j = 0; j < M; j++) { re[j] = (double)integer[j]; im[j] = (double)integer[j + M]; }
    forward_torus(torus, N, twist, tw, a);
    forward_integer(re, im, N, twist, tw, b);
    for (int j = 0; j < M; j++) a[j] = cdd_mul(a[j], b[j]);
    memset(out, 0, sizeof(u128) * N);
    add_backward(a, N, twist, tw, out);
    free(a); free(b); free(re); free(im);
}
/* exact negacyclic product over Z/2^128, O(N^2) */
void ref128_exact_product(const u128 *torus, const int64_t *integer, int N, u128 *out) {
#pragma omp parallel for
    for (int j = 0; j < N; j++) {
        u128 acc = 0;
        for (int i = 0; i < N; i++) {
            int d = j - i;
            u128 t = torus[i] * (u128)(__int128)integer[d < 0 ? d + N : d];
            acc += d < 0 ? (u128)0 - t : t;
        }
        out[j] = acc;
    }
}

/* ---- Fourier key, blind rotation, PBS ---- */
/* fbsk: [npoly][4][M] planes, the engine's layout */
void ref128_bsk_to_fourier(const u128 *bsk, long npoly, int N, const double *twist, const double *tw, double *fbsk) {
    int M = N / 2;
#pragma omp parallel for
    for (long p = 0; p < npoly; p++) {
        cdd *s = malloc(sizeof(cdd) * M);
        forward_torus(bsk + p * N, N, twist, tw, s);
        double *o = fbsk + p * 4 * M;
        for (int j = 0; j < M; j++) { o[j] = s[j].re.hi; o[M + j] = s[j].re.lo; o[2 * M + j] = s[j].im.hi; o[3 * M + j] = s[j].im.lo; }
        free(s);
    }
}

static void rotate_sub(const u128 *p, int N, uint32_t at, u128 *ct1) { /* X^at p - p */
    int full_odd = (at / N) & 1, rem = at % N;
    for (int j = 0; j < N; j++) {
        int src = j - rem, wrap = src < 0;
        u128 v = p[wrap ? src + N : src];
        ct1[j] = ((wrap != full_odd) ? (u128)0 - v : v) - p[j];
    }
}

/* acc += ggsw (Fourier) external product with ct1 = X^at acc - acc: one CMUX, the kernel's order */
static void cmux(u128 *acc, const double *ggsw, uint32_t at, int N, int k, int base_log, int level,
                 const double *twist, const double *tw) {
    int M = N / 2, K1 = k + 1;
    u128 *ct1 = malloc(sizeof(u128) * K1 * N);
    cdd *out = malloc(sizeof(cdd) * K1 * M), *f = malloc(sizeof(cdd) * M);
    double *re = malloc(sizeof(double) * M), *im = malloc(sizeof(double) * M);
    for (int r = 0; r < K1; r++) rotate_sub(acc + r * N, N, at, ct1 + r * N);
    for (int lvl = level; lvl >= 1; lvl--) {
        for (int r = 0; r < K1; r++) {
            for (int j = 0; j < N; j++) {
                u128 st = decomp_state(ct1[r * N + j], base_log * level);
                int64_t d = 0;
                for (int l = level; l >= lvl; l--) d = decomp_next(&st, base_log);
                if (j < M) re[j] = (double)d; else im[j - M] = (double)d;
            }
            forward_integer(re, im, N, twist, tw, f);
            const double *row = ggsw + (size_t)((lvl - 1) * K1 + r) * K1 * 4 * M;
            int first = lvl == level && r == 0;
            for (int c = 0; c < K1; c++)
                for (int j = 0; j < M; j++) {
                    cdd prod = cdd_mul(plane_get(row + (size_t)c * 4 * M, M, j), f[j]);
                    out[c * M + j] = first ? prod : cdd_add(out[c * M + j], prod);
                }
        }
    }
    for (int c = 0; c < K1; c++) add_backward(out + c * M, N, twist, tw, acc + c * N);
    free(ct1); free(out); free(f); free(re); free(im);
}

/* lwe_in [count][n+1]; luts [lut_count][(k+1)N]; out [count][kN+1] or [count][(k+1)N] when glwe_out */
void ref128_pbs_batch(const double *fbsk, const double *twist, const double *tw, int n, int N, int k, int base_log,
                      int level, int modulus_log, const u128 *lwe_in, const u128 *luts, long lut_count,
                      const uint32_t *lut_indexes, u128 *out, long count, int glwe_out, int threads) {
    int K1 = k + 1, M = N / 2, log2n = 0;
    while ((1 << log2n) < N) log2n++;
    size_t ggsw_stride = (size_t)level * K1 * K1 * 4 * M;
#pragma omp parallel for num_threads(threads > 0 ? threads : 1) schedule(dynamic)
    for (long ct = 0; ct < count; ct++) {
        const u128 *in = lwe_in + ct * (n + 1);
        long li = lut_indexes ? lut_indexes[ct] : 0;
        if (li >= lut_count) li = lut_count - 1;
        const u128 *lut = luts + li * K1 * N;
        u128 *acc = malloc(sizeof(u128) * K1 * N);
        uint32_t bt = modulus_switch(in[n], log2n);
        int full = bt / N, rem = bt % N;
        for (int p = 0; p < K1; p++)
            for (int j = 0; j < N; j++) {
                int src = j + rem, wrap = src >= N;
                u128 v = lut[p * N + (wrap ? src - N : src)];
                acc[p * N + j] = (wrap != (full & 1)) ? (u128)0 - v : v;
            }
        for (int i = 0; i < n; i++)
            cmux(acc, fbsk + (size_t)i * ggsw_stride, modulus_switch(in[i], log2n), N, k, base_log, level, twist, tw);
        if (modulus_log < 128)
            for (int e = 0; e < K1 * N; e++) acc[e] = closest_representable(acc[e], modulus_log, 1);
        if (glwe_out) {
            memcpy(out + ct * K1 * N, acc, sizeof(u128) * K1 * N);
        } else {
            u128 *o = out + ct * ((long)k * N + 1);
            for (int p = 0; p < k; p++)
                for (int j = 0; j < N; j++) o[p * N + j] = j == 0 ? acc[p * N] : (u128)0 - acc[p * N + N - j];
            o[k * N] = acc[k * N];
        }
        free(acc);
    }
}

/* ---- exact CMUX from the standard-domain GGSW [level][k+1][k+1][N]: acc += sum digits * rows ---- */
void ref128_exact_cmux(u128 *acc, const u128 *ggsw, uint32_t at, int N, int k, int base_log, int level) {
    int K1 = k + 1;
    u128 *ct1 = malloc(sizeof(u128) * K1 * N), *prod = malloc(sizeof(u128) * N);
    int64_t *dg = malloc(sizeof(int64_t) * N);
    for (int r = 0; r < K1; r++) rotate_sub(acc + r * N, N, at, ct1 + r * N);
    for (int lvl = level; lvl >= 1; lvl--)
        for (int r = 0; r < K1; r++) {
            for (int j = 0; j < N; j++) {
                u128 st = decomp_state(ct1[r * N + j], base_log * level);
                int64_t d = 0;
                for (int l = level; l >= lvl; l--) d = decomp_next(&st, base_log);
                dg[j] = d;
            }
            for (int c = 0; c < K1; c++) {
                ref128_exact_product(ggsw + ((size_t)((lvl - 1) * K1 + r) * K1 + c) * N, dg, N, prod);
                for (int j = 0; j < N; j++) acc[c * N + j] += prod[j];
            }
        }
    free(ct1); free(prod); free(dg);
}

/* ---- client: a seeded PRNG of this file's own (splitmix64 stream per (seed, index)) ---- */
typedef struct { uint64_t s; } rng;
static uint64_t rng_next(rng *r) {
    uint64_t z = (r->s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static rng rng_at(uint64_t seed, uint64_t index) {
    rng r = {seed * 0xD1342543DE82EF95ull + index * 0xDA942042E4DD58B5ull + 1};
    rng_next(&r);
    return r;
}
static u128 rng_u128(rng *r) { u128 h = rng_next(r); return (h << 64) | rng_next(r); }
static double rng_unit(rng *r) { return ((double)(rng_next(r) >> 11) + 0.5) * 0x1p-53; }
/* Gaussian noise of standard deviation std (as a torus fraction) scaled to 2^128 */
static u128 rng_noise(rng *r, double std) {
    double g = sqrt(-2.0 * log(rng_unit(r))) * cos(6.283185307179586 * rng_unit(r)) * std;
    long double v = (long double)g * 0x1p128L;
    __int128 q = (__int128)roundl(v);
    return (u128)q;
}
void ref128_uniform(uint64_t seed, u128 *out, long n) {
    rng r = rng_at(seed, 0);
    for (long i = 0; i < n; i++) out[i] = rng_u128(&r);
}
void ref128_binary_key(uint64_t seed, uint64_t *key, long n) {
    rng r = rng_at(seed, 1);
    for (long i = 0; i < n; i++) key[i] = rng_next(&r) >> 63;
}
/* one GLWE encryption of the plaintext polynomial pt under glwe_sk [k][N]: out [(k+1)N] */
static void glwe_encrypt(rng *r, const uint64_t *glwe_sk, int k, int N, const u128 *pt, double std, u128 *out) {
    u128 *body = out + (size_t)k * N;
    for (int j = 0; j < N; j++) body[j] = pt[j] + rng_noise(r, std);
    for (int p = 0; p < k; p++) {
        u128 *mask = out + (size_t)p * N;
        for (int j = 0; j < N; j++) mask[j] = rng_u128(r);
        for (int i = 0; i < N; i++) {
            if (!glwe_sk[p * N + i]) continue;
            for (int j = 0; j < N; j++) { /* body += mask * X^i */
                int d = j - i;
                body[j] += d < 0 ? (u128)0 - mask[d + N] : mask[d];
            }
        }
    }
}
/* GGSW of the bit m [level][k+1][k+1 polys][N] (ggsw_encryption.rs): row (lvl, r) encrypts
 * -m S_r 2^(128 - base_log lvl) for r < k and m 2^(128 - base_log lvl) for r = k */
static void ggsw_encrypt(rng *r, uint64_t m, const uint64_t *glwe_sk, int k, int N, int base_log, int level,
                         double std, u128 *out) {
    int K1 = k + 1;
    u128 *pt = malloc(sizeof(u128) * N);
    for (int lvl = 1; lvl <= level; lvl++) {
        u128 factor = (u128)1 << (128 - base_log * lvl);
        for (int row = 0; row < K1; row++) {
            for (int j = 0; j < N; j++) {
                if (row < k) pt[j] = (m && glwe_sk[row * N + j]) ? (u128)0 - factor : 0;
                else pt[j] = (j == 0 && m) ? factor : 0;
            }
            glwe_encrypt(r, glwe_sk, k, N, pt, std, out + ((size_t)(lvl - 1) * K1 + row) * K1 * N);
        }
    }
    free(pt);
}
void ref128_gen_ggsw(uint64_t seed, uint64_t m, const uint64_t *glwe_sk, int k, int N, int base_log, int level,
                     double std, u128 *out) {
    rng r = rng_at(seed, 3);
    ggsw_encrypt(&r, m, glwe_sk, k, N, base_log, level, std, out);
}
void ref128_gen_bsk(uint64_t seed, const uint64_t *lwe_sk, int n, const uint64_t *glwe_sk, int k, int N,
                    int base_log, int level, double std, u128 *bsk, int threads) {
    size_t stride = (size_t)level * (k + 1) * (k + 1) * N;
#pragma omp parallel for num_threads(threads > 0 ? threads : 1) schedule(dynamic)
    for (int i = 0; i < n; i++) {
        rng r = rng_at(seed, 16 + (uint64_t)i);
        ggsw_encrypt(&r, lwe_sk[i], glwe_sk, k, N, base_log, level, std, bsk + (size_t)i * stride);
    }
}
void ref128_lwe_encrypt(uint64_t seed, const uint64_t *sk, int n, const u128 *pts, long count, double std, u128 *cts) {
    for (long c = 0; c < count; c++) {
        rng r = rng_at(seed, (uint64_t)1 << 32 | (uint64_t)c);
        u128 *ct = cts + c * (n + 1);
        u128 body = pts[c] + rng_noise(&r, std);
        for (int i = 0; i < n; i++) {
            ct[i] = rng_u128(&r);
            if (sk[i]) body += ct[i];
        }
        ct[n] = body;
    }
}
void ref128_lwe_decrypt(const uint64_t *sk, int n, const u128 *cts, long count, u128 *pts) {
    for (long c = 0; c < count; c++) {
        const u128 *ct = cts + c * (n + 1);
        u128 body = ct[n];
        for (int i = 0; i < n; i++)
            if (sk[i]) body -= ct[i];
        pts[c] = body;
    }
}
