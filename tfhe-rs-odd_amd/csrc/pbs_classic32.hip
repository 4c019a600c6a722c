// pbs_classic32.hip -- batched classic programmable bootstrap on the 32-bit torus (gfx950).
//
// The boolean module of the reference computes on LweCiphertextOwned<u32> with a Fourier key made
// from a LweBootstrapKeyOwned<u32> (tfhe/src/boolean/engine/bootstrapping.rs:17-97, 257-401).  The
// fft64 code is generic over the scalar; what it does for u32 words:
//   fast_pbs_modulus_switch, Scalar::BITS = 32           fft_impl/common.rs:26-43
//   SignedDecomposer<u32>                                 commons/math/decomposition/decomposer.rs:99-153
//   convert_forward_integer_u32                           fft64/math/fft/x86.rs:228-412
//   convert_add_backward_torus_u32 (wrapping cvtpd_epi32) fft64/math/fft/x86.rs:652-947
//   blind_rotate_assign / add_external_product_assign     fft64/crypto/bootstrap.rs:243-344, ggsw.rs:477-697
// The accumulator is rounded to 32 bits after every CMUX, so this is not the u64 kernel on words
// shifted left by 32.
//
// Layout: as pbs_classic.hip -- one wavefront per GLWE polynomial, (k+1) waves per ciphertext, the
// row spectra exchanged through LDS under GroupSync, WaveFft<N/2> with twiddles and twist in LDS,
// the oracle's MAC order (levels L..1, rows 0..k).  One ciphertext per workgroup, one workgroup per
// ciphertext (no persistent grid); several workgroups share a CU.  The accumulator polynomial is
// 2V uint32_t registers per lane (position lane + 64 h), rotated through a 4N-byte LDS buffer.
//
// Control flow is uniform: a zero mask element runs as a rotation by 0 (ct1 = 0, every digit 0,
// spectra +-0, increments 0), as in the u64 kernel.
#include "engine.h"
#include "pbs_common.h"

namespace tfhe_mi355 {

template <int LOG2N>
__device__ __forceinline__ uint32_t pbs_modulus_switch32(uint32_t x) {
    uint32_t o = x >> (32 - LOG2N - 2);
    o += 1;
    o >>= 1;
    return o;  // in [0, 2N]
}

template <int N, int K, int L>
struct Pbs32Config {
    static constexpr int M = N / 2;
    // after the exchange buffers: one GroupSync flag word per wave
    static constexpr size_t flags_off() { return PbsLds<M>::bytes(K + 1); }
    static constexpr size_t lds_bytes() { return flags_off() + 16 * ((K + 1 + 3) / 4); }
    static_assert(lds_bytes() <= 64 * 1024, "at least two workgroups per CU");
};

template <int N, int K, int L>
__global__ void __launch_bounds__(64 * (K + 1)) pbs_classic32_kernel(ClassicPbs32Launch a) {
    constexpr int M = N / 2;
    constexpr int V = M / 64;
    constexpr int LOG2N = ilog2(N);
    using Cfg = Pbs32Config<N, K, L>;
    using Fft = WaveFft<M>;
    using Lay = PbsLds<M>;
    constexpr int XL = Lay::XL;
    static_assert(sizeof(cx) * XL >= sizeof(uint32_t) * N, "exchange buffer holds one polynomial");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *lds = reinterpret_cast<double2 *>(smem);
    const double2 *s_twist = lds + Lay::twist_off;

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // polynomial this wave owns
    const int lane = threadIdx.x & 63;
    const int n = a.n;
    const int beta = a.base_log;
    const uint32_t dmask = (1u << beta) - 1;
    BlockSync sync;       // whole workgroup: table fill
    WaveLocalSync wsync;  // wave-private buffer reuse

    for (int e = threadIdx.x; e < M; e += blockDim.x) lds[Lay::twist_off + e] = a.twist[e];
    uint32_t *gflags = reinterpret_cast<uint32_t *>(smem + Cfg::flags_off());
    if (threadIdx.x <= K) gflags[threadIdx.x] = 0;
    Fft::Lds::template fill<M>(lds + Lay::s1_off, lds + Lay::s2_off, a.W, threadIdx.x, blockDim.x);
    const typename Fft::Lds tw{lds + Lay::s1_off, lds + Lay::s2_off};
    sync();

    cx *xct = reinterpret_cast<cx *>(lds + Lay::xbuf_off);
    GroupSync<K + 1> xsync{lds_addr(gflags), lds_addr(gflags + wave)};
    cx *xb = xct + wave * XL;
    uint32_t *xb32 = reinterpret_cast<uint32_t *>(xb);

    const int ct = blockIdx.x;  // grid = count
    const uint32_t *in = a.lwe_in + (size_t)ct * (n + 1);
    const uint32_t li = a.lut_indexes ? min(a.lut_indexes[ct], a.lut_count - 1u) : 0u;
    const uint32_t *lut = a.luts + (size_t)li * (K + 1) * N + (size_t)wave * N;

    // accumulator polynomial: c[h] = position lane + 64 h.  ct0 = LUT / X^{b~}
    // (bootstrap.rs:255-275, polynomial_wrapping_monic_monomial_div)
    uint32_t c[2 * V];
    {
        const uint32_t bt = pbs_modulus_switch32<LOG2N>(in[n]);
        const int full = bt / N, rem = bt % N;
#pragma unroll
        for (int h = 0; h < 2 * V; h++) {
            const int src = lane + 64 * h + rem;
            const bool wrap = src >= N;
            const uint32_t v = lut[wrap ? src - N : src];
            c[h] = (wrap != (bool)(full & 1)) ? 0u - v : v;
        }
    }

    constexpr size_t ggsw_stride = (size_t)L * (K + 1) * (K + 1) * M;
    const double2 *gcol = a.fbsk + (size_t)wave * M + lane;  // column c = wave, this lane

    for (int i = 0; i < n; i++) {
        const uint32_t at = pbs_modulus_switch32<LOG2N>(in[i]);
        const bool full_odd = (at / N) & 1;
        const int rem = at % N;
        const double2 *ggsw = gcol + (size_t)i * ggsw_stride;

        // ct1 = X^{a~} ct0 - ct0 (polynomial_algorithms.rs:425-490) through the wave's LDS buffer:
        // (X^d p)[j] = -p[N - d + j] for j < d, p[j - d] otherwise, negated again past a full N
        wsync();
#pragma unroll
        for (int h = 0; h < 2 * V; h++) xb32[lane + 64 * h] = c[h];
        wsync();
        uint32_t st[2 * V];  // decomposer state (closest_representable >> (32 - beta L))
#pragma unroll
        for (int h = 0; h < 2 * V; h++) {
            const int src = lane + 64 * h - rem;
            const bool wrap = src < 0;
            const uint32_t v = xb32[wrap ? src + N : src];
            const uint32_t ct1 = ((wrap != full_odd) ? 0u - v : v) - c[h];
            st[h] = ((ct1 >> (31 - beta * L)) + 1) >> 1;
        }

        cx acc[V];
#pragma unroll 1
        for (int lvl = L; lvl >= 1; lvl--) {
            cx v[V];
#pragma unroll
            for (int b = 0; b < V; b++) {
                const cx z = {(double)decomp_digit32(st[b], beta, dmask), (double)decomp_digit32(st[V + b], beta, dmask)};
                const double2 w = s_twist[lane + 64 * b];
                v[b] = cmulw(z, w.x, w.y);  // convert_forward_integer_u32
            }
            Fft::forward(v, xb, tw, lane, wsync);
            wsync();
#pragma unroll
            for (int s = 0; s < V; s++)
                reinterpret_cast<double2 *>(xb)[s * 64 + lane] = make_double2(v[s].re, v[s].im);
            xsync();
            // output column c = wave: sum_r F_r * G[lvl][r][c]   (ggsw.rs:524-567, update_with_fmadd)
            const double2 *lm = ggsw + (size_t)(lvl - 1) * (K + 1) * (K + 1) * M;
#pragma unroll
            for (int s = 0; s < V; s++) {
                cx o = lvl != L ? acc[s] : cx{0.0, 0.0};
#pragma unroll
                for (int r = 0; r <= K; r++) {
                    const double2 gg = lm[(size_t)r * (K + 1) * M + s * 64];
                    const double2 ff = reinterpret_cast<const double2 *>(xct + r * XL)[s * 64 + lane];
                    if (lvl == L && r == 0) {
                        o.re = fma(gg.x, ff.x, -(gg.y * ff.y));
                        o.im = fma(gg.x, ff.y, gg.y * ff.x);
                    } else {
                        o.re = fma(gg.x, ff.x, fma(-gg.y, ff.y, o.re));
                        o.im = fma(gg.x, ff.y, fma(gg.y, ff.x, o.im));
                    }
                }
                acc[s] = o;
            }
            xsync();  // every wave is done reading the published spectra
        }
        Fft::inverse(acc, xb, tw, lane, wsync);
#pragma unroll
        for (int b = 0; b < V; b++) {
            const double2 w = s_twist[lane + 64 * b];  // the resident key carries the 1/M
            backward_add32(acc[b], cx{w.x, w.y}, c[b], c[V + b]);
        }
    }

    if (a.glwe_out) {
        uint32_t *g = a.lwe_out + ((size_t)ct * (K + 1) + wave) * N;
#pragma unroll
        for (int h = 0; h < 2 * V; h++) g[lane + 64 * h] = c[h];
        return;
    }
    // sample extract at degree 0 (glwe_sample_extraction.rs:91-147): out[0] = acc[0], out[j] = -acc[N - j]
    wsync();
#pragma unroll
    for (int h = 0; h < 2 * V; h++) xb32[lane + 64 * h] = c[h];
    wsync();
    uint32_t *out = a.lwe_out + (size_t)ct * (K * N + 1);
    if (wave < K) {
        for (int j = lane; j < N; j += 64) out[wave * N + j] = j == 0 ? xb32[0] : 0u - xb32[N - j];
    } else if (lane == 0) {
        out[K * N] = c[0];
    }
}

template <int N, int K, int L>
static hipError_t launch_pbs32_t(const ClassicPbs32Launch &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const size_t lds = Pbs32Config<N, K, L>::lds_bytes();
    hipLaunchKernelGGL((pbs_classic32_kernel<N, K, L>), dim3(a.count), dim3(64 * (K + 1)), lds, s, a);
    return hipGetLastError();
}

// the four shapes of the boolean parameter sets (boolean/parameters/mod.rs:123-192)
#define PBS_CLASSIC32_SHAPES(X) X(512, 2, 3) X(1024, 2, 2) X(1024, 1, 4) X(1024, 1, 3)

bool classic_pbs32_supported(int N, int k, int L) {
#define PBS32_SUPPORTED(n_, k_, l_) if (N == n_ && k == k_ && L == l_) return true;
    PBS_CLASSIC32_SHAPES(PBS32_SUPPORTED)
#undef PBS32_SUPPORTED
    return false;
}

int classic_pbs32_resident_blocks(int N, int k, int L) {
#define PBS32_RESIDENT(n_, k_, l_) \
    if (N == n_ && k == k_ && L == l_) \
        return resident_blocks((const void *)pbs_classic32_kernel<n_, k_, l_>, 64 * (k_ + 1), \
                               Pbs32Config<n_, k_, l_>::lds_bytes());
    PBS_CLASSIC32_SHAPES(PBS32_RESIDENT)
#undef PBS32_RESIDENT
    return 0;
}

hipError_t launch_classic_pbs32(int N, int k, int L, const ClassicPbs32Launch &a, hipStream_t s) {
#define PBS32_LAUNCH(n_, k_, l_) if (N == n_ && k == k_ && L == l_) return launch_pbs32_t<n_, k_, l_>(a, s);
    PBS_CLASSIC32_SHAPES(PBS32_LAUNCH)
#undef PBS32_LAUNCH
    return hipErrorInvalidValue;
}

// u32 standard key -> the u64 words the Fourier conversion reads: (double)(int32_t)x 2^-32 equals
// (double)(int64_t)((uint64_t)x << 32) 2^-64 exactly, so bsk_to_fourier_kernel serves both widths
__global__ void __launch_bounds__(256) widen32_kernel(const uint32_t *__restrict__ in, uint64_t *__restrict__ out,
                                                      size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (uint64_t)in[e] << 32;
}

hipError_t launch_widen32(const uint32_t *in, uint64_t *out, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(widen32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
