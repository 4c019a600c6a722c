// glwe_mult.hip -- GLWE x GLWE product with relinearisation on gfx950 (u64 wrapping arithmetic): the
// fork's "even transistor" multiplication.
//
// Replaces glwe_mult (tfhe/src/core_crypto/algorithms/custom_glwe_glwe_product.rs:13-321) bit for bit:
//   modulus switch   every word of both GLWEs x >> (32 - log_p/2), a plain shift            (:75-132)
//   tensor product   T_i = A_i A'_i, R_ij = A_i A'_j + A_j A'_i (j < i),
//                    out.mask_i = A_i B' + A'_i B, out.body = B B'                            (:192-259)
//   relinearisation  out_q += sum_n sum_l digit_l(T/R block n) * rlk[n][l][q], n = i(i+1)/2 + j,
//                    SignedDecomposer digits, level L first as the key's GLWEs               (:261-321)
// The reference multiplies by Karatsuba (polynomial_algorithms.rs:683-742); over Z/2^64 every exact
// algorithm gives the same bits, and both kernels here sum the N terms of each coefficient directly.
//
// One workgroup of 512 threads per pair, two launches.  A negacyclic product c = a * b is computed
// with a as the broadcast operand and b in LDS as its signed extension ext[N + t] = b[t],
// ext[t] = -b[t] (0 <= t < N): c[m] = sum_j a[j] ext[N + m - j], so the wrap's sign costs nothing per
// term.  A thread owns 4 consecutive coefficients of one output polynomial; per 4 terms it reads
// a[j..j+3] (broadcast) and the 7-entry window ext[N + 4m - j - 3 .. N + 4m - j + 3] with aligned
// 16-byte LDS reads (the extension is stored 3 entries in, which makes every window start a multiple
// of 4 entries) and makes 16 multiply-adds from registers.  N/4 threads cover a polynomial, so at
// N < 2048 the 2048/N thread groups of a workgroup work on different polynomials at once.
//
// Multiplies.  A product mod 2^64 of a = a0 + 2^32 a1 and b = b0 + 2^32 b1 is
// a0 b0 + 2^32 (a0 b1 + a1 b0): one 32 x 32 -> 64 multiply-add into a 64-bit accumulator and two
// low-half 32-bit multiplies into a 32-bit one (after the modulus switch a1, b1 < 2^(log_p/2), which
// the sum does not need to know: the identity holds for every operand, also log_p = 64).  In the
// relinearisation the lane operand is an int32 digit d and the key word K = K0 + 2^32 K1 is uniform:
// with K0s = K0 as a signed 32-bit value and t = K0's top bit, d K = d K0s + 2^32 d (K1 + t), one
// signed 32 x 32 -> 64 multiply-add and one low-half multiply per term.
#include "decompose64.h"
#include "engine.h"

namespace tfhe_mi355 {

namespace {
constexpr int GM_THREADS = 512;
constexpr int GM_PAD = 4;  // an extension holds 2N + 4 entries: 3 in front, 1 behind (read, never used)

typedef unsigned long long gm_u64x2 __attribute__((ext_vector_type(2)));
typedef int gm_i32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int gm_blocks(int k) { return k * (k + 1) / 2; }

// acc + 2^32 hi += a * b for the thread's coefficients 4 m0 .. 4 m0 + 3; a: N words, e: b's extension
template <int N>
__device__ __forceinline__ void gm_mac_u64(const uint64_t *a, const uint64_t *e, int m0, uint64_t (&acc)[4],
                                           uint32_t (&hi)[4]) {
    const uint64_t *wb = e + N + 4 * m0;
#pragma unroll 2
    for (int j0 = 0; j0 < N; j0 += 4) {
        uint64_t av[4], w[8];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const gm_u64x2 t = *reinterpret_cast<const gm_u64x2 *>(a + j0 + 2 * q);
            av[2 * q] = t.x;
            av[2 * q + 1] = t.y;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const gm_u64x2 t = *reinterpret_cast<const gm_u64x2 *>(wb - j0 + 2 * q);
            w[2 * q] = t.x;
            w[2 * q + 1] = t.y;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t a0 = (uint32_t)av[u], a1 = (uint32_t)(av[u] >> 32);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint64_t b = w[r - u + 3];
                const uint32_t b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
                acc[r] += (uint64_t)a0 * (uint64_t)b0;
                hi[r] += a0 * b1 + a1 * b0;
            }
        }
    }
}

// the same with key words kp (uniform) and the int32 digit extension d
template <int N>
__device__ __forceinline__ void gm_mac_digit(const uint64_t *kp, const int32_t *d, int m0, int64_t (&acc)[4],
                                             uint32_t (&hi)[4]) {
    const int32_t *wb = d + N + 4 * m0;
#pragma unroll 2
    for (int j0 = 0; j0 < N; j0 += 4) {
        uint64_t kv[4];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const gm_u64x2 t = *reinterpret_cast<const gm_u64x2 *>(kp + j0 + 2 * q);
            kv[2 * q] = t.x;
            kv[2 * q + 1] = t.y;
        }
        const gm_i32x4 w0 = *reinterpret_cast<const gm_i32x4 *>(wb - j0);
        const gm_i32x4 w1 = *reinterpret_cast<const gm_i32x4 *>(wb - j0 + 4);
        const int32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int32_t k0s = (int32_t)(uint32_t)kv[u];
            const uint32_t kh = (uint32_t)(kv[u] >> 32) + ((uint32_t)kv[u] >> 31);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[r] += (int64_t)w[r - u + 3] * (int64_t)k0s;
                hi[r] += (uint32_t)w[r - u + 3] * kh;
            }
        }
    }
}

// coefficients 4 m0 .. 4 m0 + 3 of polynomial p of a pair's result into its output row: the GLWE
// itself, or its degree-0 sample (mask_p[0] = a_p[0], mask_p[i] = -a_p[N - i]: glwe_ops.hip,
// glwe_sample_extraction.rs); add: accumulate into what the tensor kernel wrote
template <int N>
__device__ __forceinline__ void gm_store(uint64_t *row, int p, int m0, const uint64_t (&v)[4], bool extract, bool add) {
    uint64_t *o = row + (size_t)p * N;
    if (!extract) {  // 8-byte accesses: the caller's rows need no more than a u64's alignment
#pragma unroll
        for (int r = 0; r < 4; r++) o[4 * m0 + r] = add ? o[4 * m0 + r] + v[r] : v[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int c = 4 * m0 + r;
        uint64_t *dst = o + (c == 0 ? 0 : N - c);
        const uint64_t val = c == 0 ? v[r] : 0 - v[r];
        *dst = add ? *dst + val : val;
    }
}

// sum of one value per thread over the workgroup (any order: the sum wraps); result valid in thread 0
__device__ __forceinline__ uint64_t gm_block_sum(uint64_t v, uint64_t *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = GM_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}
}  // namespace

// LDS: lhs [(k+1)][N] | rhs extensions [(k+1)][2N + 4] | reduction [512]
template <int N>
__global__ void __launch_bounds__(GM_THREADS) glwe_tensor_kernel(GlweMultLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EXT = 2 * N + GM_PAD, TP = N / 4, G = GM_THREADS / TP;
    constexpr int LOG2N = N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : 11;
    const int tid = threadIdx.x, k = a.k;
    const size_t c = blockIdx.x;
    const int glwe = (k + 1) * N, nblk = gm_blocks(k);
    uint64_t *A = reinterpret_cast<uint64_t *>(smem);
    uint64_t *E = A + glwe;
    uint64_t *red = E + (size_t)(k + 1) * EXT;
    const uint64_t *lhs = a.lhs + c * glwe, *rhs = a.rhs + c * glwe;
    const int shift = 32 - a.log_p / 2;  // 0..32

    for (int e = tid; e < glwe; e += GM_THREADS) {
        const int p = e >> LOG2N, i = e & (N - 1);
        A[e] = lhs[e] >> shift;
        const uint64_t b = rhs[e] >> shift;
        uint64_t *ep = E + (size_t)p * EXT;
        ep[3 + N + i] = b;
        ep[3 + i] = 0 - b;
        if (i < 3) ep[i] = 0;
        if (i == 3) ep[EXT - 1] = 0;
    }
    __syncthreads();

    // output polynomials, the two-product ones first: R_ij (j < i), mask_i, then T_i and the body
    const int g = tid / TP, m0 = tid % TP;
    const int noff = k * (k - 1) / 2, ntask = noff + 2 * k + (a.extract ? 0 : 1);
    uint64_t *out_row = a.out + c * (size_t)(a.extract ? k * N + 1 : glwe);
    uint64_t *tr_row = a.tr + c * (size_t)nblk * N;
    for (int t = g; t < ntask; t += G) {
        int x0, y0, x1 = -1, y1 = -1, dst_tr = -1, dst_out = -1;
        if (t < noff) {
            int i = 1;
            while (i * (i + 1) / 2 <= t) i++;
            const int j = t - i * (i - 1) / 2;
            x0 = i, y0 = j, x1 = j, y1 = i;
            dst_tr = i * (i + 1) / 2 + j;
        } else if (t < noff + k) {
            const int i = t - noff;
            x0 = i, y0 = k, x1 = k, y1 = i;
            dst_out = i;
        } else if (t < noff + 2 * k) {
            const int i = t - noff - k;
            x0 = i, y0 = i;
            dst_tr = i * (i + 1) / 2 + i;
        } else {
            x0 = k, y0 = k;
            dst_out = k;
        }
        uint64_t acc[4] = {0, 0, 0, 0};
        uint32_t hi[4] = {0, 0, 0, 0};
        gm_mac_u64<N>(A + x0 * N, E + (size_t)y0 * EXT, m0, acc, hi);
        if (x1 >= 0) gm_mac_u64<N>(A + x1 * N, E + (size_t)y1 * EXT, m0, acc, hi);
        uint64_t v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = acc[r] + ((uint64_t)hi[r] << 32);
        if (dst_tr >= 0) gm_store<N>(tr_row, dst_tr, m0, v, false, false);
        else gm_store<N>(out_row, dst_out, m0, v, a.extract && dst_out < k, false);
    }
    if (a.extract) {  // (B B')[0] = sum_j B[j] ext_B'[N - j]
        const uint64_t *b = A + k * N, *e = E + (size_t)k * EXT + 3 + N;
        uint64_t s = 0;
        for (int j = tid; j < N; j += GM_THREADS) s += b[j] * e[-j];
        s = gm_block_sum(s, red);
        if (tid == 0) out_row[k * N] = s;
    }
}

// LDS: key GLWE of one (block, level) [(k+1)][N] | digit extension [2N + 4] int32 | reduction [512]
template <int N>
__global__ void __launch_bounds__(GM_THREADS) glwe_relin_kernel(GlweMultLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EXT = 2 * N + GM_PAD, TP = N / 4, G = GM_THREADS / TP;
    constexpr int NS = N > GM_THREADS ? N / GM_THREADS : 1;  // T/R coefficients decomposed per thread
    const int tid = threadIdx.x, k = a.k, L = a.level, beta = a.base_log;
    const size_t c = blockIdx.x;
    const int glwe = (k + 1) * N, nblk = gm_blocks(k);
    uint64_t *K = reinterpret_cast<uint64_t *>(smem);
    int32_t *D = reinterpret_cast<int32_t *>(K + glwe);
    uint64_t *red = reinterpret_cast<uint64_t *>(D + EXT);
    const uint64_t mask = (1ULL << beta) - 1;
    const uint64_t *tr_row = a.tr + c * (size_t)nblk * N;

    // output polynomials of this thread group: q = g, g + G (at most two: (k+1) N <= 4096); with
    // extract the body is no polynomial but one coefficient, summed over the workgroup at the end
    const int g = tid / TP, m0 = tid % TP;
    const int nq = a.extract ? k : k + 1;
    const bool has0 = g < nq, has1 = g + G < nq;
    int64_t acc0[4] = {0, 0, 0, 0}, acc1[4] = {0, 0, 0, 0};
    uint32_t hi0[4] = {0, 0, 0, 0}, hi1[4] = {0, 0, 0, 0};
    uint64_t body0 = 0;

    if (tid < 3) D[tid] = 0;
    if (tid == 3) D[EXT - 1] = 0;
    for (int n = 0; n < nblk; n++) {
        uint64_t state[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const int co = tid + i * GM_THREADS;
            state[i] = co < N ? closest_repr(tr_row[(size_t)n * N + co], beta, L) >> (64 - beta * L) : 0;
        }
        for (int l = 0; l < L; l++) {
            __syncthreads();  // the previous (block, level)'s reads of K and D
#pragma unroll
            for (int i = 0; i < NS; i++) {
                const int co = tid + i * GM_THREADS;
                const int32_t d = (int32_t)signed_digit64(state[i], beta, mask);
                if (co < N) {
                    D[3 + N + co] = d;
                    D[3 + co] = -d;
                }
            }
            const gm_u64x2 *src = reinterpret_cast<const gm_u64x2 *>(a.rlk + ((size_t)n * L + l) * glwe);
            gm_u64x2 *dst = reinterpret_cast<gm_u64x2 *>(K);
            for (int e = tid; e < glwe / 2; e += GM_THREADS) dst[e] = src[e];
            __syncthreads();
            if (has0) gm_mac_digit<N>(K + g * N, D, m0, acc0, hi0);
            if (has1) gm_mac_digit<N>(K + (g + G) * N, D, m0, acc1, hi1);
            if (a.extract) {
                const uint64_t *kb = K + k * N;
                const int32_t *e = D + 3 + N;
                for (int j = tid; j < N; j += GM_THREADS) body0 += kb[j] * (uint64_t)(int64_t)e[-j];
            }
        }
    }
    uint64_t *out_row = a.out + c * (size_t)(a.extract ? k * N + 1 : glwe);
    uint64_t v[4];
    if (has0) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = (uint64_t)acc0[r] + ((uint64_t)hi0[r] << 32);
        gm_store<N>(out_row, g, m0, v, a.extract, true);
    }
    if (has1) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = (uint64_t)acc1[r] + ((uint64_t)hi1[r] << 32);
        gm_store<N>(out_row, g + G, m0, v, a.extract, true);
    }
    if (a.extract) {
        __syncthreads();
        const uint64_t s = gm_block_sum(body0, red);
        if (tid == 0) out_row[k * N] += s;
    }
}

bool glwe_mult_supported(int N, int k) {
    return (N == 256 || N == 512 || N == 1024 || N == 2048) && k >= 1 && k <= 5 && (k + 1) * N <= 4096;
}

size_t glwe_mult_scratch_bytes(int N, int k, size_t count) { return count * (size_t)gm_blocks(k) * N * sizeof(uint64_t); }

template <int N>
static hipError_t launch_glwe_mult_t(const GlweMultLaunch &a, hipStream_t s) {
    const size_t ext = 2 * N + GM_PAD, glwe = (size_t)(a.k + 1) * N, red = GM_THREADS * sizeof(uint64_t);
    const size_t lds_tensor = 8 * glwe + 8 * (a.k + 1) * ext + red;
    const size_t lds_relin = 8 * glwe + 4 * ext + red;
    {
        TimedLaunch tl(a.timer, "glwe_tensor", s);
        hipLaunchKernelGGL((glwe_tensor_kernel<N>), dim3((unsigned)a.count), dim3(GM_THREADS), lds_tensor, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    {
        TimedLaunch tl(a.timer, "glwe_relin", s);
        hipLaunchKernelGGL((glwe_relin_kernel<N>), dim3((unsigned)a.count), dim3(GM_THREADS), lds_relin, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_glwe_mult(const GlweMultLaunch &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    if (!glwe_mult_supported(a.N, a.k) || a.log_p < 0 || a.log_p > 64 || (a.log_p & 1) || a.base_log < 1 ||
        a.base_log > 31 || a.level < 1 || a.base_log * a.level > 63 || a.count > 0x7fffffffull)
        return hipErrorInvalidValue;
    switch (a.N) {
    case 256: return launch_glwe_mult_t<256>(a, s);
    case 512: return launch_glwe_mult_t<512>(a, s);
    case 1024: return launch_glwe_mult_t<1024>(a, s);
    default: return launch_glwe_mult_t<2048>(a, s);
    }
}

}  // namespace tfhe_mi355
