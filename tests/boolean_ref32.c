/* boolean_ref32.c -- CPU restatement of the 32-bit-torus PBS (test infrastructure of
 * tests/boolean_reference.py; shares no code with libtfhe_mi355).
 *
 * What the reference's fft64 code does for Scalar = u32 (boolean/engine/bootstrapping.rs:257-297):
 * blind_rotate_assign (fft64/crypto/bootstrap.rs:243-344) with fast_pbs_modulus_switch at 32 bits
 * (fft_impl/common.rs:26-43), the u32 SignedDecomposer (decomposer.rs:99-153, iter.rs:134-141),
 * convert_forward_integer_u32, update_with_fmadd (ggsw.rs:616-697) and convert_add_backward_torus_u32
 * (x86.rs:877-947: fract = t - rint(t), then a WRAPPING conversion of rint(fract 2^32) to i32).
 *
 * The FFT itself is not restated: the forward integer transform and the raw inverse transform are the
 * oracle's own (function pointers handed in from Python: orc_fft_forward_integer, orc_fft_complex),
 * so the FFT DAG and twist are the oracle's bit for bit.  This file adds the fma MAC in the oracle's
 * order (levels L..1, rows 0..k) and the backward twist, fma and rounding, which need a real fma(). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef int (*fft_complex_fn)(int M, const double *in_reim, double *out_reim, int inverse);
typedef int (*forward_integer_fn)(int N, const uint64_t *x, double *out_reim);

typedef struct {
    fft_complex_fn fft;
    forward_integer_fn fwd;
    const double *twist; /* [M] (re, im): exp(i pi j / N), the oracle's table */
    int n, k, N, base_log, level;
} ref32_ctx;

/* X = rint_half_even(fr 2^32) mod 2^32 for fr in [-1/2, 1/2]; fr = +-1/2 -> 0x80000000 */
uint32_t ref32_from_fraction(double fr) { return (uint32_t)(int64_t)rint(fr * 4294967296.0); }

static uint32_t ref32_modulus_switch(uint32_t x, int log2N) {
    uint32_t o = x >> (32 - log2N - 2);
    return (o + 1) >> 1;
}

/* closest_representable (decomposer.rs:99-119) on 32 bits */
static uint32_t closest32(uint32_t x, int beta, int L) {
    int shift = 32 - beta * L - 1;
    uint32_t r = x >> shift;
    r += 1;
    r &= ~(uint32_t)1;
    return r << shift;
}

/* all L digits of x, digit[0] = level L (the first the iterator yields) */
static void ref32_decompose(uint32_t x, int beta, int L, int32_t *digits) {
    uint32_t state = closest32(x, beta, L) >> (32 - beta * L);
    uint32_t mask = ((uint32_t)1 << beta) - 1;
    for (int l = 0; l < L; l++) {
        uint32_t res = state & mask;
        state >>= beta;
        uint32_t carry = ((res - 1) | state) & res;
        carry >>= beta - 1;
        state += carry;
        digits[l] = (int32_t)(res - (carry << beta));
    }
}

/* out = X^e p in Z[X]/(X^N + 1), 0 <= e < 2N */
static void mono_mul(uint32_t *out, const uint32_t *p, int N, int e) {
    for (int j = 0; j < N; j++) {
        int t = j + e;
        uint32_t v = p[j];
        out[t % N] = ((t / N) & 1) ? 0u - v : v;
    }
}

/* acc += ggsw (x) glwe: add_external_product_assign (ggsw.rs:477-598) on u32 words.
 * ggsw: [L][k+1][k+1][M] complex, level matrix lvl at index lvl - 1. */
static void external_product_add32(const ref32_ctx *c, const double *ggsw, uint32_t *acc, const uint32_t *glwe) {
    const int k = c->k, N = c->N, M = N / 2, L = c->level, beta = c->base_log;
    const size_t gl = (size_t)(k + 1) * N;
    int32_t *dig = malloc(sizeof(int32_t) * gl * L);
    uint64_t *row = malloc(sizeof(uint64_t) * N);
    double *fd = malloc(sizeof(double) * 2 * M);
    double *facc = calloc((size_t)(k + 1) * 2 * M, sizeof(double));
    double *z = malloc(sizeof(double) * 2 * M);
    for (size_t j = 0; j < gl; j++) ref32_decompose(glwe[j], beta, L, dig + j * L);
    int first = 1;
    for (int lvl = L; lvl >= 1; lvl--) {
        const double *lm = ggsw + (size_t)(lvl - 1) * (k + 1) * (k + 1) * 2 * M;
        for (int r = 0; r <= k; r++) {
            for (int j = 0; j < N; j++) row[j] = (uint64_t)(int64_t)dig[((size_t)r * N + j) * L + (L - lvl)];
            c->fwd(N, row, fd);
            for (int col = 0; col <= k; col++) {
                const double *g = lm + ((size_t)r * (k + 1) + col) * 2 * M;
                double *a = facc + (size_t)col * 2 * M;
                for (int f = 0; f < M; f++) {
                    double gr = g[2 * f], gi = g[2 * f + 1], dr = fd[2 * f], di = fd[2 * f + 1];
                    if (first) {
                        a[2 * f] = fma(gr, dr, -(gi * di));
                        a[2 * f + 1] = fma(gr, di, gi * dr);
                    } else {
                        a[2 * f] = fma(gr, dr, fma(-gi, di, a[2 * f]));
                        a[2 * f + 1] = fma(gr, di, fma(gi, dr, a[2 * f + 1]));
                    }
                }
            }
            first = 0;
        }
    }
    const double norm = 1.0 / (double)M;
    for (int col = 0; col <= k; col++) {
        c->fft(M, facc + (size_t)col * 2 * M, z, 1);
        uint32_t *o = acc + (size_t)col * N;
        for (int j = 0; j < M; j++) {
            double wr = norm * c->twist[2 * j], wi = norm * c->twist[2 * j + 1];
            double mr = fma(z[2 * j], wr, z[2 * j + 1] * wi);
            double mi = fma(-z[2 * j], wi, z[2 * j + 1] * wr);
            o[j] += ref32_from_fraction(mr - rint(mr));
            o[j + M] += ref32_from_fraction(mi - rint(mi));
        }
    }
    free(dig);
    free(row);
    free(fd);
    free(facc);
    free(z);
}

void ref32_external_product(fft_complex_fn fft, forward_integer_fn fwd, const double *twist, int k, int N,
                            int base_log, int level, const double *ggsw, uint32_t *acc, const uint32_t *glwe) {
    ref32_ctx c = {fft, fwd, twist, 0, k, N, base_log, level};
    external_product_add32(&c, ggsw, acc, glwe);
}

static void pbs_one32(const ref32_ctx *c, const double *fbsk, const uint32_t *in, uint32_t *out, const uint32_t *lut,
                      int glwe_out) {
    const int n = c->n, k = c->k, N = c->N, M = N / 2;
    int log2N = 0;
    while ((1 << log2N) < N) log2N++;
    const size_t gl = (size_t)(k + 1) * N;
    const size_t ggsw_len = (size_t)c->level * (k + 1) * (k + 1) * 2 * M;
    uint32_t *acc = malloc(sizeof(uint32_t) * gl), *ct1 = malloc(sizeof(uint32_t) * gl);
    const int bt = (int)ref32_modulus_switch(in[n], log2N);
    /* ct0 = LUT / X^{b~} = LUT X^{2N - b~} */
    for (int p = 0; p <= k; p++) mono_mul(acc + (size_t)p * N, lut + (size_t)p * N, N, (4 * N - bt) % (2 * N));
    for (int i = 0; i < n; i++) {
        if (in[i] == 0) continue; /* bootstrap.rs:285 */
        const int at = (int)ref32_modulus_switch(in[i], log2N);
        for (int p = 0; p <= k; p++) mono_mul(ct1 + (size_t)p * N, acc + (size_t)p * N, N, at % (2 * N));
        for (size_t j = 0; j < gl; j++) ct1[j] -= acc[j];
        external_product_add32(c, fbsk + (size_t)i * ggsw_len, acc, ct1);
    }
    if (glwe_out) {
        memcpy(out, acc, sizeof(uint32_t) * gl);
    } else { /* extract_lwe_sample_from_glwe_ciphertext at degree 0 */
        for (int p = 0; p < k; p++) {
            const uint32_t *a = acc + (size_t)p * N;
            out[(size_t)p * N] = a[0];
            for (int j = 1; j < N; j++) out[(size_t)p * N + j] = 0u - a[N - j];
        }
        out[(size_t)k * N] = acc[(size_t)k * N];
    }
    free(acc);
    free(ct1);
}

void ref32_pbs_batch(fft_complex_fn fft, forward_integer_fn fwd, const double *twist, const double *fbsk, int n, int k,
                     int N, int base_log, int level, const uint32_t *in, uint32_t *out, const uint32_t *luts,
                     const uint32_t *lut_idx, long count, int glwe_out) {
    const ref32_ctx c = {fft, fwd, twist, n, k, N, base_log, level};
    const size_t out_len = glwe_out ? (size_t)(k + 1) * N : (size_t)k * N + 1;
#pragma omp parallel for schedule(dynamic, 1)
    for (long i = 0; i < count; i++) {
        const size_t li = lut_idx ? lut_idx[i] : 0;
        pbs_one32(&c, fbsk, in + (size_t)i * (n + 1), out + (size_t)i * out_len, luts + li * (size_t)(k + 1) * N,
                  glwe_out);
    }
}
