// pfpks.hip -- batched private functional packing keyswitch on gfx950 (u64 wrapping arithmetic).
//
// Replaces private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext
// (algorithms/lwe_private_functional_packing_keyswitch.rs:21-89) applied with every key of an
// LwePrivateFunctionalPackingKeyswitchKeyList, the second stage of the circuit bootstrap
// (fft_impl/fft64/crypto/wop_pbs/mod.rs:333-342).
//
// Shape: out[c][g][j] = - sum_{i <= kN} sum_{lvl} d_lvl(in[c][i]) * K[g][i][lvl-1][j]
// i.e. a [count x (kN+1) L] x [(kN+1) L x (k+1)(k+1)N] product over Z/2^64.  Unlike the packing
// keyswitch of keyswitch.hip the input body (i = kN) is one more decomposed row, nothing is added
// to the output, and the decomposition is the PBS-sized one of the WoP sets (base_log up to 31:
// digits do not fit int8).  The key stays in the reference's memory order, level 1 first: the
// decomposer yields level L first, so digit l of the carry loop meets key row L-1-l.
//
// Two forms.  pfpks_kernel: the keyswitch_kernel tiling (64 ciphertexts x 64 columns per
// workgroup, int32 digits staged in LDS), for every decomposition.  pfpks_mfma_kernel: for
// base_log <= 15 every digit |d| <= 2^14 splits exactly as d = a0 + 256 a1 (a0 in [-128, 127],
// a1 in [-64, 64]), so with the key in byte planes K = sum_b 2^(8b) K_b
//   sum d K = sum_b 2^(8b) (A0 K_b) + sum_b 2^(8b+8) (A1 K_b)           (mod 2^64)
// and plane b+1 of A0 shares its weight with plane b of A1: one int32 accumulator per weight,
// 8 + 7 int8 MFMAs per 32-row step (A1 K_7 has weight 2^64 and vanishes).
#include "decompose64.h"
#include "engine.h"

namespace tfhe_mi355 {

namespace {
constexpr int PF_TJ = 64;      // output columns per workgroup
constexpr int PF_TC = 64;      // ciphertexts per workgroup
constexpr int PF_CPT = 16;     // ciphertexts per thread
constexpr int PF_ROWS = 128;   // (input word, level) digit rows staged per LDS chunk
constexpr int PF_DPARTS = 8;   // digit workgroups per ciphertext (MFMA form)
}  // namespace

__global__ void __launch_bounds__(256) pfpks_kernel(PfpksLaunch a) {
    __shared__ int32_t dig[PF_ROWS][PF_TC];
    const int tid = threadIdx.x;
    const int tj = tid & 63, tg = tid >> 6;
    const int J = blockIdx.x * PF_TJ + tj;
    const int c0 = blockIdx.y * PF_TC;
    const int in_rows = a.in_rows, L = a.level, beta = a.base_log;
    const uint64_t mask = (1ULL << beta) - 1;
    const bool jok = J < a.ncols;
    // column J = (key g, GLWE word j): a 64-column tile never straddles two keys ((k+1)N % 64 == 0)
    const int g = jok ? J / a.glwe : 0, j = jok ? J % a.glwe : 0;
    const uint64_t *kcol = a.key + (size_t)g * in_rows * L * a.glwe + j;
    const int ic = PF_ROWS / L;  // input words per chunk (L <= 63: at least 2)

    uint64_t acc[PF_CPT];
#pragma unroll
    for (int t = 0; t < PF_CPT; t++) acc[t] = 0;

    for (int i0 = 0; i0 < in_rows; i0 += ic) {
        __syncthreads();
        for (int q = tid; q < ic * PF_TC; q += 256) {
            const int ci = q % PF_TC, ii = q / PF_TC;
            const int c = c0 + ci, i = i0 + ii;
            uint64_t state = 0;
            if (c < a.count && i < in_rows)
                state = closest_repr(a.lwe_in[(size_t)c * in_rows + i], beta, L) >> (64 - beta * L);
            for (int l = 0; l < L; l++) {
                uint64_t res = state & mask;
                state >>= beta;
                uint64_t carry = ((res - 1) | state) & res;
                carry >>= beta - 1;
                state += carry;
                dig[ii * L + (L - 1 - l)][ci] = (int32_t)(int64_t)(res - (carry << beta));
            }
        }
        __syncthreads();
        const int nr = min(ic, in_rows - i0) * L;
        const uint64_t *kp = kcol + (size_t)i0 * L * a.glwe;
        for (int r = 0; r < nr; r++) {
            const uint64_t kv = jok ? kp[(size_t)r * a.glwe] : 0;
#pragma unroll
            for (int t = 0; t < PF_CPT; t++) {
                const int64_t d = dig[r][tg * PF_CPT + t];
                acc[t] -= (uint64_t)(d * (int64_t)kv);
            }
        }
    }
    if (!jok) return;
#pragma unroll
    for (int t = 0; t < PF_CPT; t++) {
        const int c = c0 + tg * PF_CPT + t;
        if (c >= a.count) break;
        a.glwe_out[(size_t)c * a.ncols + J] = acc[t];
    }
}

// ---------------------------------------------------------------------------------------
// int8-MFMA form.  Key planes Kt[b][J][m] = (int8)(byte_b(K[g][i][lvl-1][j]) - 128) with
// J = g (k+1)N + j and m = i L + lvl - 1, repacked once at upload; digit planes D0 / D1 [c][m].
// K_b = Kt_b + 128, so each product gains 128 * rowsum(D) per plane, added back in the epilogue.
// MFMA operand layout as in keyswitch.hip (ks_mfma_kernel).
// ---------------------------------------------------------------------------------------
typedef int pf_v4i __attribute__((ext_vector_type(4)));
typedef int pf_v16i __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256) pfpksk_repack_kernel(const uint64_t *__restrict__ key, int8_t *__restrict__ kt,
                                                            size_t keys, size_t rows, size_t glwe, size_t mpad,
                                                            size_t jpad) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= keys * rows * glwe) return;
    const size_t j = e % glwe, m = (e / glwe) % rows, g = e / (glwe * rows);
    const uint64_t v = key[e];
    const size_t J = g * glwe + j;
#pragma unroll
    for (int b = 0; b < 8; b++) kt[((size_t)b * jpad + J) * mpad + m] = (int8_t)(uint8_t)(((v >> (8 * b)) & 0xff) ^ 0x80);
}

__global__ void __launch_bounds__(256) pfpks_digits_kernel(PfpksLaunch a, int8_t *__restrict__ d0,
                                                           int8_t *__restrict__ d1, int *__restrict__ rowsum,
                                                           size_t mpad) {
    __shared__ int red0[256], red1[256];
    const int c = blockIdx.x / PF_DPARTS, part = blockIdx.x % PF_DPARTS;
    const int in_rows = a.in_rows, L = a.level, beta = a.base_log;
    const uint64_t mask = (1ULL << beta) - 1;
    const uint64_t *x = a.lwe_in + (size_t)c * in_rows;
    int8_t *p0 = d0 + (size_t)c * mpad, *p1 = d1 + (size_t)c * mpad;
    const int per = (in_rows + PF_DPARTS - 1) / PF_DPARTS, i0 = part * per, i1 = min(in_rows, i0 + per);
    int s0 = 0, s1 = 0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        uint64_t state = closest_repr(x[i], beta, L) >> (64 - beta * L);
        for (int l = 0; l < L; l++) {
            uint64_t res = state & mask;
            state >>= beta;
            uint64_t carry = ((res - 1) | state) & res;
            carry >>= beta - 1;
            state += carry;
            const int v = (int)(int64_t)(res - (carry << beta));
            const int lo = (int)(int8_t)(v & 0xff), hi = (v - lo) >> 8;  // v = lo + 256 hi exactly
            const size_t m = (size_t)i * L + (L - 1 - l);
            p0[m] = (int8_t)lo;
            p1[m] = (int8_t)hi;
            s0 += lo;
            s1 += hi;
        }
    }
    if (part == PF_DPARTS - 1)
        for (size_t m = (size_t)in_rows * L + threadIdx.x; m < mpad; m += 256) p0[m] = p1[m] = 0;
    red0[threadIdx.x] = s0;
    red1[threadIdx.x] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            red0[threadIdx.x] += red0[threadIdx.x + w];
            red1[threadIdx.x] += red1[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rowsum[((size_t)c * PF_DPARTS + part) * 2] = red0[0];
        rowsum[((size_t)c * PF_DPARTS + part) * 2 + 1] = red1[0];
    }
}

// workgroup tile: 64 ciphertexts x 64 output columns, 4 waves of 32 x 32, 8 weights each
__global__ void __launch_bounds__(256) pfpks_mfma_kernel(PfpksLaunch a, const int8_t *__restrict__ d0,
                                                         const int8_t *__restrict__ d1,
                                                         const int *__restrict__ rowsum,
                                                         const int8_t *__restrict__ kt, size_t mpad, size_t jpad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.y * 64 + 32 * (wave >> 1);
    const int j0 = blockIdx.x * 64 + 32 * (wave & 1);
    // digit rows past the batch (the tile's padding) read as zero, from row 0: no memset of the scratch
    const bool arow = c0 + r < a.count;
    const size_t aoff = (size_t)(arow ? c0 + r : 0) * mpad + 16 * h;
    const int8_t *pa0 = d0 + aoff, *pa1 = d1 + aoff;
    const int8_t *pb = kt + (size_t)(j0 + r) * mpad + 16 * h;  // j0 + r < jpad: the planes are padded
    const size_t plane = jpad * mpad;
    pf_v16i acc[8];
#pragma unroll
    for (int b = 0; b < 8; b++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[b][q] = 0;
    for (size_t k = 0; k < mpad; k += 32) {
        const pf_v4i z = {0, 0, 0, 0};
        const pf_v4i av0 = arow ? *reinterpret_cast<const pf_v4i *>(pa0 + k) : z;
        const pf_v4i av1 = arow ? *reinterpret_cast<const pf_v4i *>(pa1 + k) : z;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const pf_v4i bv = *reinterpret_cast<const pf_v4i *>(pb + (size_t)b * plane + k);
            acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av0, bv, acc[b], 0, 0, 0);
            if (b < 7) acc[b + 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av1, bv, acc[b + 1], 0, 0, 0);
        }
    }
    const int J = j0 + r;
    if (J >= a.ncols) return;
    // sum_b 2^(8b) * 128 = 128 * 0x0101010101010101 (mod 2^64)
    constexpr uint64_t kOffset = 0x8080808080808080ULL;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = c0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (c >= a.count) continue;
        int rs0 = 0, rs1 = 0;
#pragma unroll
        for (int p = 0; p < PF_DPARTS; p++) {
            rs0 += rowsum[((size_t)c * PF_DPARTS + p) * 2];
            rs1 += rowsum[((size_t)c * PF_DPARTS + p) * 2 + 1];
        }
        uint64_t v = (uint64_t)(int64_t)rs0 * kOffset + (uint64_t)(int64_t)rs1 * (kOffset << 8);
#pragma unroll
        for (int b = 0; b < 8; b++) v += (uint64_t)(int64_t)acc[b][q] << (8 * b);
        a.glwe_out[(size_t)c * a.ncols + J] = 0 - v;
    }
}

size_t pfpks_mfma_rows(int in_rows, int level) { return ((size_t)in_rows * level + 31) / 32 * 32; }
size_t pfpks_mfma_cols(int ncols) { return ((size_t)ncols + 63) / 64 * 64; }

bool pfpks_mfma_supported(int in_rows, int level, int base_log) {
    // one accumulator takes A0 K_b (|a0| <= 128) and A1 K_(b-1) (|a1| <= 64) against |K - 128| <= 128:
    // |partial| <= rows * (128 + 64) * 128 must stay below 2^31
    return base_log <= 15 && (double)pfpks_mfma_rows(in_rows, level) * 192.0 * 128.0 < 2147483648.0;
}

size_t pfpks_mfma_scratch_bytes(int in_rows, int level, int count) {
    const size_t cp = ((size_t)count + 63) / 64 * 64;
    return 2 * cp * pfpks_mfma_rows(in_rows, level) + cp * PF_DPARTS * 2 * sizeof(int) + 256;
}

hipError_t launch_pfpksk_repack(const uint64_t *key, int8_t *kt, int keys, int in_rows, int level, int glwe,
                                hipStream_t s) {
    const size_t rows = (size_t)in_rows * level, total = (size_t)keys * rows * glwe;
    const size_t mpad = pfpks_mfma_rows(in_rows, level), jpad = pfpks_mfma_cols(keys * glwe);
    if ((total + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(kt, 0, 8 * mpad * jpad, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pfpksk_repack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, key, kt,
                       (size_t)keys, rows, (size_t)glwe, mpad, jpad);
    return hipGetLastError();
}

hipError_t launch_pfpks_mfma(const PfpksLaunch &a, const int8_t *kt, void *scratch, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    if (!pfpks_mfma_supported(a.in_rows, a.level, a.base_log)) return hipErrorInvalidValue;
    const size_t mpad = pfpks_mfma_rows(a.in_rows, a.level), jpad = pfpks_mfma_cols(a.ncols);
    const size_t cpad = ((size_t)a.count + 63) / 64 * 64;
    int8_t *d0 = reinterpret_cast<int8_t *>(scratch);
    int8_t *d1 = d0 + cpad * mpad;
    int *rowsum = reinterpret_cast<int *>(reinterpret_cast<char *>(scratch) + ((2 * cpad * mpad + 255) / 256) * 256);
    hipLaunchKernelGGL(pfpks_digits_kernel, dim3((unsigned)a.count * PF_DPARTS), dim3(256), 0, s, a, d0, d1, rowsum,
                       mpad);
    hipLaunchKernelGGL(pfpks_mfma_kernel, dim3((unsigned)(jpad / 64), (unsigned)(cpad / 64)), dim3(256), 0, s, a, d0,
                       d1, rowsum, kt, mpad, jpad);
    return hipGetLastError();
}

hipError_t launch_pfpks(const PfpksLaunch &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    if (a.base_log < 1 || a.base_log > 31 || a.level < 1 || a.base_log * a.level > 63 || a.glwe % PF_TJ)
        return hipErrorInvalidValue;
    dim3 grid((a.ncols + PF_TJ - 1) / PF_TJ, (a.count + PF_TC - 1) / PF_TC);
    hipLaunchKernelGGL(pfpks_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
