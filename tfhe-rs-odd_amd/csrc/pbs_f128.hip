// pbs_f128.hip -- programmable bootstrap on the 128-bit torus through a double-double FFT (gfx950).
//
// Native counterpart of the reference's fft128 path:
//   convert_standard_lwe_bootstrap_key_to_fourier_128     algorithms/lwe_bootstrap_key_conversion.rs:164
//   programmable_bootstrap_f128_lwe_ciphertext            algorithms/lwe_programmable_bootstrapping.rs:1378-1459
//   Fourier128LweBootstrapKey::blind_rotate_assign        fft_impl/fft128/crypto/bootstrap.rs:245-337
//   add_external_product_assign, update_with_fmadd        fft_impl/fft128/crypto/ggsw.rs:424-486, 591-648
//   convert_forward_torus / _integer / backward           fft_impl/fft128/math/fft/mod.rs:201-328
//   fast_pbs_modulus_switch, Scalar::BITS = 128           fft_impl/common.rs:26-43
// The butterflies of the reference are concrete-fft's and not part of its tree: the transform's DAG is
// this engine's own, restated op for op by tests/pbs_ref128.c.
//
// Transform: z_j = (x_j + i x_{j+M}) w_j, w_j = exp(i pi j / N), M = N/2; a radix-2
// decimation-in-frequency DFT of M points (natural order in, bit-reversed out), the pointwise products in
// bit-reversed order, a radix-2 decimation-in-time inverse (bit-reversed in, natural out, unnormalised),
// conj(w_j), 1/M, backward conversion.  Every N uses the same plan: log2(M) radix-2 stages.
//
// Layout: one workgroup of T = min(512, M) threads per ciphertext.  LDS holds the u128 accumulator
// ((k+1) N words) and one polynomial's spectrum as four f64 planes (re.hi, re.lo, im.hi, im.lo) of M
// entries; the FFT runs in those planes with one workgroup barrier per stage.  The (k+1) output spectra of
// a CMUX are accumulated in registers ((k+1) M / T complex double-double values per lane, at most 4).
// The decomposer state is recomputed per level from the accumulator (at most 4 levels), so no state is
// stored.  Twist and twiddles are read from global memory (48 KB at N = 2048, shared by every workgroup).
// The monomial degrees (fast_pbs_modulus_switch of every input word) are computed by a one-thread-per-word
// kernel into the caller's scratch (4 (n+1) bytes per ciphertext), so the CMUX loop reads one 32-bit word.
//
// Control flow is uniform: a zero mask element runs as a rotation by 0 (ct1 = 0, digits 0, spectra 0,
// increments 0), value-identical to the reference's skip (bootstrap.rs:291).
#include "dd_device.h"
#include "engine.h"

namespace tfhe_mi355 {

namespace {

constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x / 2); }

struct Planes {
    double *p;  // 4 planes of M doubles
    int M;
    __device__ __forceinline__ cdd get(int i) const { return {{p[i], p[M + i]}, {p[2 * M + i], p[3 * M + i]}}; }
    __device__ __forceinline__ void set(int i, cdd v) const {
        p[i] = v.re.hi;
        p[M + i] = v.re.lo;
        p[2 * M + i] = v.im.hi;
        p[3 * M + i] = v.im.lo;
    }
};
struct ConstPlanes {
    const double *p;
    int M;
    __device__ __forceinline__ cdd get(int i) const { return {{p[i], p[M + i]}, {p[2 * M + i], p[3 * M + i]}}; }
};

// forward: for h = M/2 .. 1: (a, b) -> (a + b, (a - b) W[j M/(2h)]), W[t] = exp(-2 pi i t / M)
template <int M, int T>
__device__ __forceinline__ void fft128_forward(Planes s, ConstPlanes W, int tid) {
    for (int h = M / 2; h >= 1; h >>= 1) {
        const int step = M / (2 * h);
        for (int b = tid; b < M / 2; b += T) {
            const int j = b & (h - 1);
            const int i0 = ((b - j) << 1) + j, i1 = i0 + h;
            const cdd x = s.get(i0), y = s.get(i1);
            s.set(i0, cdd_add(x, y));
            s.set(i1, cdd_mul(cdd_sub(x, y), W.get(j * step)));
        }
        __syncthreads();
    }
}
// inverse (unnormalised): for h = 1 .. M/2: t = b conj(W[j M/(2h)]); (a, b) -> (a + t, a - t)
template <int M, int T>
__device__ __forceinline__ void fft128_inverse(Planes s, ConstPlanes W, int tid) {
    for (int h = 1; h <= M / 2; h <<= 1) {
        const int step = M / (2 * h);
        for (int b = tid; b < M / 2; b += T) {
            const int j = b & (h - 1);
            const int i0 = ((b - j) << 1) + j, i1 = i0 + h;
            const cdd x = s.get(i0);
            const cdd t = cdd_mul(s.get(i1), cdd_conj(W.get(j * step)));
            s.set(i0, cdd_add(x, t));
            s.set(i1, cdd_sub(x, t));
        }
        __syncthreads();
    }
}

// (re + i im) w for two exact doubles (integer digits) and a double-double twist
__device__ __forceinline__ cdd twist_integer(double re, double im, cdd w) {
    return {dd_sub(dd_mul_f64(w.re, re), dd_mul_f64(w.im, im)), dd_add(dd_mul_f64(w.re, im), dd_mul_f64(w.im, re))};
}

template <int N>
struct F128Shape {
    static constexpr int M = N / 2;
    // two waves per SIMD at M >= 512: 41.4 ms per 256 ciphertexts at (2048, 1), 54.4 ms with 256 threads
    static constexpr int T = M < 512 ? M : 512;
    static constexpr int S = M / T;
    static constexpr size_t spectrum_bytes = 4 * sizeof(double) * M;
};

// ---- key conversion: one workgroup per polynomial of the standard key ------------------------------
template <int N>
__global__ void __launch_bounds__(F128Shape<N>::T) bsk128_to_fourier_kernel(const u128 *__restrict__ bsk,
                                                                            double *__restrict__ fbsk,
                                                                            const double *__restrict__ twist,
                                                                            const double *__restrict__ tw) {
    constexpr int M = F128Shape<N>::M, T = F128Shape<N>::T;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Planes sp{reinterpret_cast<double *>(smem), M};
    const ConstPlanes Wt{twist, M}, W{tw, M / 2};
    const int tid = threadIdx.x;
    const u128 *poly = bsk + (size_t)blockIdx.x * N;
    const double norm = dd_pow2(-128);
    for (int j = tid; j < M; j += T) {  // convert_forward_torus (mod.rs:263-287), then the twist
        const cdd z = {dd_scale(u128_to_signed_dd(poly[j]), norm), dd_scale(u128_to_signed_dd(poly[j + M]), norm)};
        sp.set(j, cdd_mul(z, Wt.get(j)));
    }
    __syncthreads();
    fft128_forward<M, T>(sp, W, tid);
    double *out = fbsk + (size_t)blockIdx.x * 4 * M;
    for (int e = tid; e < 4 * M; e += T) out[e] = sp.p[e];
}

// ---- blind rotation ------------------------------------------------------------------------------
template <int N, int K>
__global__ void __launch_bounds__(F128Shape<N>::T) pbs_f128_kernel(PbsF128Launch a) {
    constexpr int M = F128Shape<N>::M, T = F128Shape<N>::T, S = F128Shape<N>::S;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u128 *acc = reinterpret_cast<u128 *>(smem);  // [(K+1)][N]
    const Planes sp{reinterpret_cast<double *>(smem + sizeof(u128) * (K + 1) * N), M};
    const ConstPlanes Wt{a.twist, M}, W{a.tw, M / 2};
    const int tid = threadIdx.x;
    const int n = a.n, beta = a.base_log, L = a.level;
    const int ct = blockIdx.x;
    const uint32_t *deg = a.degrees + (size_t)ct * (n + 1);
    const uint32_t li = a.lut_indexes ? min(a.lut_indexes[ct], a.lut_count - 1u) : 0u;
    const u128 *lut = a.luts + (size_t)li * (K + 1) * N;

    // ct0 = LUT / X^{b~} (bootstrap.rs:269-283, polynomial_wrapping_monic_monomial_div)
    {
        const uint32_t bt = deg[n];
        const int full = bt / N, rem = bt % N;
        for (int e = tid; e < (K + 1) * N; e += T) {
            const int p = e / N, j = e % N;
            const int src = j + rem;
            const bool wrap = src >= N;
            const u128 v = lut[p * N + (wrap ? src - N : src)];
            acc[e] = (wrap != (bool)(full & 1)) ? (u128)0 - v : v;
        }
    }
    __syncthreads();

    const size_t poly_doubles = (size_t)4 * M;
    const size_t ggsw_stride = (size_t)L * (K + 1) * (K + 1) * poly_doubles;
    const double inv_m = 1.0 / (double)M;

    for (int i = 0; i < n; i++) {
        const uint32_t at = deg[i];
        const bool full_odd = (at / N) & 1;
        const int rem = at % N;
        const double *ggsw = a.fbsk + (size_t)i * ggsw_stride;

        cdd out[K + 1][S];
#pragma unroll 1
        for (int lvl = L; lvl >= 1; lvl--) {
#pragma unroll 1
            for (int r = 0; r <= K; r++) {
                // digits of ct1 = X^{a~} ct0 - ct0 (polynomial_algorithms.rs:425-490) at this level:
                // (X^d p)[j] = -p[N - d + j] for j < d, p[j - d] otherwise, negated again past a full N
                const u128 *pr = acc + r * N;
                for (int j = tid; j < M; j += T) {
                    double dg[2];
#pragma unroll
                    for (int hf = 0; hf < 2; hf++) {
                        const int jj = j + hf * M;
                        const int src = jj - rem;
                        const bool wrap = src < 0;
                        const u128 v = pr[wrap ? src + N : src];
                        const u128 ct1 = ((wrap != full_odd) ? (u128)0 - v : v) - pr[jj];
                        u128 st = decomp128_state(ct1, beta * L);
                        int64_t d = 0;
                        for (int l = L; l >= lvl; l--) d = decomp128_next(st, beta);
                        dg[hf] = (double)d;  // |d| <= 2^30: exact (convert_forward_integer, mod.rs:289-308)
                    }
                    sp.set(j, twist_integer(dg[0], dg[1], Wt.get(j)));
                }
                __syncthreads();
                fft128_forward<M, T>(sp, W, tid);
                // out_c (+)= G[lvl][r][c] * F (ggsw.rs:591-648): first product assigns, later ones add
                const double *row = ggsw + (size_t)((lvl - 1) * (K + 1) + r) * (K + 1) * poly_doubles;
                const bool first = lvl == L && r == 0;
#pragma unroll
                for (int s = 0; s < S; s++) {
                    const int idx = tid + T * s;
                    const cdd f = sp.get(idx);
#pragma unroll
                    for (int c = 0; c <= K; c++) {
                        const ConstPlanes g{row + (size_t)c * poly_doubles, M};
                        const cdd prod = cdd_mul(g.get(idx), f);
                        out[c][s] = first ? prod : cdd_add(out[c][s], prod);
                    }
                }
                __syncthreads();  // the spectrum is overwritten by the next row
            }
        }
#pragma unroll
        for (int c = 0; c <= K; c++) {
#pragma unroll
            for (int s = 0; s < S; s++) sp.set(tid + T * s, out[c][s]);
            __syncthreads();
            fft128_inverse<M, T>(sp, W, tid);
            u128 *pc = acc + c * N;
            for (int j = tid; j < M; j += T) {  // convert_add_backward_torus (mod.rs:310-328)
                const cdd z = cdd_mul(sp.get(j), cdd_conj(Wt.get(j)));
                pc[j] += torus128_from_dd(dd_scale(z.re, inv_m));
                pc[j + M] += torus128_from_dd(dd_scale(z.im, inv_m));
            }
            __syncthreads();
        }
    }

    const int m = a.modulus_log;
    if (a.glwe_out) {
        u128 *g = a.lwe_out + (size_t)ct * (K + 1) * N;
        for (int e = tid; e < (K + 1) * N; e += T) g[e] = m < 128 ? round_to_modulus128(acc[e], m) : acc[e];
        return;
    }
    // sample extract at degree 0 (glwe_sample_extraction.rs:91-147): out[0] = acc[0], out[j] = -acc[N - j]
    u128 *o = a.lwe_out + (size_t)ct * (K * N + 1);
    for (int e = tid; e < K * N + 1; e += T) {
        u128 v;
        if (e == K * N) {
            v = acc[K * N];
            if (m < 128) v = round_to_modulus128(v, m);
        } else {
            const int p = e / N, j = e % N;
            v = acc[p * N + (j == 0 ? 0 : N - j)];
            if (m < 128) v = round_to_modulus128(v, m);  // the rounding comes before the extraction's negation
            if (j != 0) v = (u128)0 - v;
        }
        o[e] = v;
    }
}

// fast_pbs_modulus_switch (common.rs:26-43) of every word of the batch: degrees in [0, 2N]
__global__ void __launch_bounds__(256) modulus_switch128_kernel(const u128 *__restrict__ in,
                                                                uint32_t *__restrict__ deg, size_t n, int log2n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) deg[e] = pbs_modulus_switch128(in[e], log2n);
}

__global__ void __launch_bounds__(256) torus128_from_f128_kernel(const double *__restrict__ hi,
                                                                 const double *__restrict__ lo,
                                                                 const u128 *__restrict__ acc, u128 *__restrict__ out,
                                                                 size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (acc ? acc[e] : (u128)0) + torus128_from_dd({hi[e], lo[e]});
}

template <int N, int K>
size_t pbs_f128_lds() {
    return sizeof(u128) * (K + 1) * N + F128Shape<N>::spectrum_bytes;
}

template <int N, int K>
hipError_t launch_pbs_f128_t(const PbsF128Launch &a, hipStream_t s) {
    const size_t lds = pbs_f128_lds<N, K>();
    // above the default 64 KB dynamic LDS limit at the larger shapes (an attribute of the current device)
    const hipError_t attr = hipFuncSetAttribute((const void *)pbs_f128_kernel<N, K>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return attr;
    const size_t words = (size_t)a.count * (a.n + 1);
    hipLaunchKernelGGL(modulus_switch128_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a.lwe_in,
                       a.degrees, words, ilog2c(N));
    hipLaunchKernelGGL((pbs_f128_kernel<N, K>), dim3(a.count), dim3(F128Shape<N>::T), lds, s, a);
    return hipGetLastError();
}

template <int N>
hipError_t launch_bsk128_t(const u128 *bsk, double *fbsk, size_t npoly, const double *twist, const double *tw,
                           hipStream_t s) {
    hipLaunchKernelGGL((bsk128_to_fourier_kernel<N>), dim3((unsigned)npoly), dim3(F128Shape<N>::T),
                       F128Shape<N>::spectrum_bytes, s, bsk, fbsk, twist, tw);
    return hipGetLastError();
}

}  // namespace

// N in {256, 512, 1024, 2048}, k in {1, 2, 3}, (k+1) N <= 4096
#define PBS_F128_SHAPES(X) \
    X(256, 1) X(256, 2) X(256, 3) X(512, 1) X(512, 2) X(512, 3) X(1024, 1) X(1024, 2) X(1024, 3) X(2048, 1)

bool pbs_f128_supported(int N, int k) {
#define F128_SUPPORTED(n_, k_) if (N == n_ && k == k_) return true;
    PBS_F128_SHAPES(F128_SUPPORTED)
#undef F128_SUPPORTED
    return false;
}

int pbs_f128_resident_blocks(int N, int k) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 0;
#define F128_RESIDENT(n_, k_)                                                                                   \
    if (N == n_ && k == k_) {                                                                                   \
        (void)hipFuncSetAttribute((const void *)pbs_f128_kernel<n_, k_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  (int)pbs_f128_lds<n_, k_>());                                                 \
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void *)pbs_f128_kernel<n_, k_>,           \
                                                         F128Shape<n_>::T, pbs_f128_lds<n_, k_>()) != hipSuccess) \
            return 0;                                                                                           \
        return cus * per;                                                                                       \
    }
    PBS_F128_SHAPES(F128_RESIDENT)
#undef F128_RESIDENT
    return 0;
}

hipError_t launch_pbs_f128(int N, int k, const PbsF128Launch &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
#define F128_LAUNCH(n_, k_) if (N == n_ && k == k_) return launch_pbs_f128_t<n_, k_>(a, s);
    PBS_F128_SHAPES(F128_LAUNCH)
#undef F128_LAUNCH
    return hipErrorInvalidValue;
}

hipError_t launch_bsk128_to_fourier(int N, const void *d_bsk, double *d_fbsk, size_t npoly, const double *twist,
                                    const double *tw, hipStream_t s) {
    if (npoly == 0) return hipSuccess;
    const u128 *b = reinterpret_cast<const u128 *>(d_bsk);
    switch (N) {
        case 256: return launch_bsk128_t<256>(b, d_fbsk, npoly, twist, tw, s);
        case 512: return launch_bsk128_t<512>(b, d_fbsk, npoly, twist, tw, s);
        case 1024: return launch_bsk128_t<1024>(b, d_fbsk, npoly, twist, tw, s);
        case 2048: return launch_bsk128_t<2048>(b, d_fbsk, npoly, twist, tw, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_torus128_from_f128(const double *hi, const double *lo, const void *acc, void *out, size_t n,
                                     hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(torus128_from_f128_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hi, lo,
                       reinterpret_cast<const u128 *>(acc), reinterpret_cast<u128 *>(out), n);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
