// keyswitch32.hip -- batched LWE keyswitch on the 32-bit torus (gfx950).
//
// keyswitch_lwe_ciphertext (tfhe/src/core_crypto/algorithms/lwe_keyswitch.rs:96-170) on
// LweCiphertextOwned<u32> under a LweKeyswitchKeyOwned<u32>, as the boolean module calls it
// (boolean/engine/bootstrapping.rs:299-391), with the 32-bit SignedDecomposer
// (commons/math/decomposition/decomposer.rs:99-153, iter.rs:134-141):
//   out[c][j] = (j == out_dim ? in[c][in_dim] : 0) - sum_{i,l} d[c][i][l] * KSK[i][l][j]   (mod 2^32)
// The digits are the values the u64 decomposer gives for word << 32 (closest_representable rounds
// at bit 31 - base_log * level).  Two arms, as keyswitch.hip: a plain integer kernel, and the
// int8-MFMA GEMM over FOUR byte planes of the key.
#include <algorithm>

#include "engine.h"

namespace tfhe_mi355 {

namespace {
constexpr int KS_TJ = 64;     // output columns per workgroup
constexpr int KS_TC = 64;     // ciphertexts per workgroup
constexpr int KS_CPT = 16;    // ciphertexts per thread
constexpr int KS_IC = 8;      // input coefficients per LDS chunk
constexpr int KS_MAXL = 16;   // max decomposition levels
constexpr int KS_DPARTS = 8;  // digit workgroups per ciphertext (MFMA arm)

// closest_representable(x) >> (32 - base_log * level), base_log * level <= 30; when the rounding
// overflows (the reference's wraps to 0) the state is 2^(base_log level): every digit is 0 too
__device__ __forceinline__ uint32_t decomp32_state(uint32_t x, int bits) { return ((x >> (31 - bits)) + 1) >> 1; }
// one step of the balanced digit iteration, level L first
__device__ __forceinline__ int decomp32_digit(uint32_t &state, int beta, uint32_t mask) {
    uint32_t res = state & mask;
    state >>= beta;
    uint32_t carry = ((res - 1) | state) & res;
    carry >>= beta - 1;
    state += carry;
    return (int)(res - (carry << beta));
}
}  // namespace

__global__ void __launch_bounds__(256) keyswitch32_kernel(Keyswitch32Launch a) {
    __shared__ int16_t dig[KS_IC][KS_MAXL][KS_TC];
    const int tid = threadIdx.x;
    const int tj = tid & 63, tg = tid >> 6;
    const int j = blockIdx.x * KS_TJ + tj;
    const int c0 = blockIdx.y * KS_TC;
    const int in_dim = a.in_dim, out_dim = a.out_dim, L = a.level, beta = a.base_log;
    const uint32_t mask = (1u << beta) - 1;
    const size_t in_stride = (size_t)in_dim + 1, out_stride = (size_t)out_dim + 1;
    const bool jok = j <= out_dim;

    uint32_t acc[KS_CPT];
#pragma unroll
    for (int t = 0; t < KS_CPT; t++) acc[t] = 0;

    for (int i0 = 0; i0 < in_dim; i0 += KS_IC) {
        __syncthreads();
        for (int q = tid; q < KS_IC * KS_TC; q += 256) {
            const int ci = q % KS_TC, ii = q / KS_TC;
            const int c = c0 + ci, i = i0 + ii;
            uint32_t state = 0;
            if (c < a.count && i < in_dim) state = decomp32_state(a.lwe_in[(size_t)c * in_stride + i], beta * L);
            for (int l = 0; l < L; l++) dig[ii][l][ci] = (int16_t)decomp32_digit(state, beta, mask);
        }
        __syncthreads();
        const int ni = min(KS_IC, in_dim - i0);
        for (int ii = 0; ii < ni; ii++) {
            for (int l = 0; l < L; l++) {
                const uint32_t k = jok ? a.ksk[((size_t)(i0 + ii) * L + l) * out_stride + j] : 0;
#pragma unroll
                for (int t = 0; t < KS_CPT; t++) acc[t] -= (uint32_t)(int)dig[ii][l][tg * KS_CPT + t] * k;
            }
        }
    }
    if (!jok) return;
#pragma unroll
    for (int t = 0; t < KS_CPT; t++) {
        const int c = c0 + tg * KS_CPT + t;
        if (c >= a.count) break;
        const uint32_t body = (j == out_dim) ? a.lwe_in[(size_t)c * in_stride + in_dim] : 0;
        a.lwe_out[(size_t)c * out_stride + j] = body + acc[t];
    }
}

// ---------------------------------------------------------------------------------------
// int8-MFMA arm (keyswitch.hip's, on four planes).  With D[c][m] the signed digits and the key
// split into byte planes K[m][j] = sum_{b<4} 2^(8b) K_b[m][j], K_b in [0, 256):
//   sum_m D K = sum_b 2^(8b) (D (K_b - 128) + 128 rowsum(D))          (mod 2^32)
// each plane an exact int8 x int8 -> int32 product (v_mfma_i32_32x32x32_i8): the same bound
// |partial| <= M 2^(beta-1) 128 < 2^31 as keyswitch.hip:88-96 is checked by ks32_mfma_supported.
// Kt[b][j][m] = (int8)(byte_b(K[m][j]) - 128), column-major (a lane's 16 consecutive m of one
// column are one 16-B load).  Operand layout as probed for keyswitch.hip: lane l, r = l & 31,
// h = l >> 5 holds A[r][16h + j] and B[16h + j][r]; C/D col = r, row = (reg&3) + 8(reg>>2) + 4h.
// ---------------------------------------------------------------------------------------
typedef int ks32_v4i __attribute__((ext_vector_type(4)));
typedef int ks32_v16i __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256) ksk32_repack_kernel(const uint32_t *__restrict__ ksk, int8_t *__restrict__ kt,
                                                           size_t rows, size_t cols, size_t mpad, size_t jpad) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cols) return;
    const size_t m = e / cols, j = e % cols;
    const uint32_t v = ksk[e];
#pragma unroll
    for (int b = 0; b < 4; b++) kt[((size_t)b * jpad + j) * mpad + m] = (int8_t)(uint8_t)(((v >> (8 * b)) & 0xff) ^ 0x80);
}

// KS_DPARTS workgroups per ciphertext: digits D[c][i*L + l] (levels L..1 as the KSK rows) of an
// eighth of the inputs each, and that part's digit sum
__global__ void __launch_bounds__(256) ks32_digits_kernel(Keyswitch32Launch a, int8_t *__restrict__ dig,
                                                          int *__restrict__ rowsum, size_t mpad, int zero_out) {
    __shared__ int red[256];
    const int c = blockIdx.x / KS_DPARTS, part = blockIdx.x % KS_DPARTS;
    if (zero_out && part == 0) {  // split-K: the GEMM's workgroups add their partial products into a zeroed row
        uint32_t *o = a.lwe_out + (size_t)c * ((size_t)a.out_dim + 1);
        for (int j = threadIdx.x; j <= a.out_dim; j += 256) o[j] = 0;
    }
    const int in_dim = a.in_dim, L = a.level, beta = a.base_log;
    const uint32_t mask = (1u << beta) - 1;
    const uint32_t *x = a.lwe_in + (size_t)c * (in_dim + 1);
    int8_t *d = dig + (size_t)c * mpad;
    const int per = (in_dim + KS_DPARTS - 1) / KS_DPARTS, i0 = part * per, i1 = min(in_dim, i0 + per);
    int sum = 0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        uint32_t state = decomp32_state(x[i], beta * L);
        for (int l = 0; l < L; l++) {
            const int v = decomp32_digit(state, beta, mask);
            d[(size_t)i * L + l] = (int8_t)v;
            sum += v;
        }
    }
    if (part == KS_DPARTS - 1)
        for (size_t m = (size_t)in_dim * L + threadIdx.x; m < mpad; m += 256) d[m] = 0;
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) rowsum[(size_t)c * KS_DPARTS + part] = red[0];
}

// workgroup tile: 64 ciphertexts x 64 output columns, 4 waves of 32 x 32, 4 byte planes each
__global__ void __launch_bounds__(256) ks32_mfma_kernel(Keyswitch32Launch a, const int8_t *__restrict__ dig,
                                                        const int *__restrict__ rowsum,
                                                        const int8_t *__restrict__ kt, size_t mpad, size_t jpad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.y * 64 + 32 * (wave >> 1);
    const int j0 = blockIdx.x * 64 + 32 * (wave & 1);
    const int8_t *pa = dig + (size_t)(c0 + r) * mpad + 16 * h;
    const int8_t *pb = kt + (size_t)(j0 + r) * mpad + 16 * h;
    const size_t plane = jpad * mpad;
    ks32_v16i acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[b][q] = 0;
    // split K (gridDim.z > 1, small batches): slice z of the rows, the partial products combined by
    // 32-bit atomic adds into an output zeroed beforehand (sums mod 2^32: order-independent, exact)
    const size_t steps = mpad / 32;
    const size_t kbeg = 32 * (steps * blockIdx.z / gridDim.z), kend = 32 * (steps * (blockIdx.z + 1) / gridDim.z);
    // digit rows past the batch (the tile's padding) read as zero: no memset of the scratch
    const bool arow = c0 + r < a.count;
    for (size_t k = kbeg; k < kend; k += 32) {
        const ks32_v4i av = arow ? *reinterpret_cast<const ks32_v4i *>(pa + k) : ks32_v4i{0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const ks32_v4i bv = *reinterpret_cast<const ks32_v4i *>(pb + (size_t)b * plane + k);
            acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc[b], 0, 0, 0);
        }
    }
    const int j = j0 + r;
    if (j > a.out_dim) return;
    const size_t in_stride = (size_t)a.in_dim + 1, out_stride = (size_t)a.out_dim + 1;
    constexpr uint32_t kOffset = 0x80808080u;  // sum_b 2^(8b) * 128 (mod 2^32)
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = c0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (c >= a.count) continue;
        const bool first = blockIdx.z == 0;
        int rs = 0;
        if (first)
#pragma unroll
            for (int p = 0; p < KS_DPARTS; p++) rs += rowsum[(size_t)c * KS_DPARTS + p];
        uint32_t v = (uint32_t)rs * kOffset;
#pragma unroll
        for (int b = 0; b < 4; b++) v += (uint32_t)acc[b][q] << (8 * b);
        const uint32_t body = (first && j == a.out_dim) ? a.lwe_in[(size_t)c * in_stride + a.in_dim] : 0;
        uint32_t *o = a.lwe_out + (size_t)c * out_stride + j;
        if (gridDim.z == 1) *o = body - v;
        else atomicAdd(o, body - v);
    }
}

bool ks32_mfma_supported(int in_dim, int level, int base_log) {
    // the digits are int8 and |partial| <= M * 2^(beta-1) * 128 must stay below 2^31
    return base_log >= 1 && base_log <= 7 && base_log * level <= 30 &&
           (double)ks_mfma_rows(in_dim, level) * (double)(1 << (base_log - 1)) * 128.0 < 2147483648.0;
}

size_t ks32_mfma_scratch_bytes(int in_dim, int level, int count) {
    const size_t cp = ((size_t)count + 63) / 64 * 64;
    return (cp * ks_mfma_rows(in_dim, level) + 255) / 256 * 256 + cp * KS_DPARTS * sizeof(int) + 256;
}

hipError_t launch_ksk32_repack(const uint32_t *ksk, int8_t *kt, int in_dim, int level, int out_dim, hipStream_t s) {
    const size_t rows = (size_t)in_dim * level, cols = (size_t)out_dim + 1;
    const size_t mpad = ks_mfma_rows(in_dim, level), jpad = ks_mfma_cols(out_dim);
    hipError_t e = hipMemsetAsync(kt, 0, 4 * mpad * jpad, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ksk32_repack_kernel, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, s, ksk, kt, rows,
                       cols, mpad, jpad);
    return hipGetLastError();
}

hipError_t launch_keyswitch32_mfma(const Keyswitch32Launch &a, const int8_t *kt, void *scratch, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    if (!ks32_mfma_supported(a.in_dim, a.level, a.base_log)) return hipErrorInvalidValue;
    const size_t mpad = ks_mfma_rows(a.in_dim, a.level), jpad = ks_mfma_cols(a.out_dim);
    const int cpad = (a.count + 63) / 64 * 64;
    int8_t *dig = reinterpret_cast<int8_t *>(scratch);
    int *rowsum = reinterpret_cast<int *>(reinterpret_cast<char *>(scratch) + (((size_t)cpad * mpad + 255) / 256) * 256);
    // few output tiles (small batches): split K over up to ~1024 workgroups, >= 2 k-steps each, as
    // launch_keyswitch_mfma; ks32_digits_kernel zeroes the rows the slices' atomics accumulate into
    const unsigned tiles = (unsigned)(jpad / 64) * (unsigned)(cpad / 64);
    unsigned split = 1;
    if (tiles < 128) split = (unsigned)std::min<size_t>((1024u + tiles - 1) / tiles, mpad / 64);
    if (split < 2) split = 1;
    hipLaunchKernelGGL(ks32_digits_kernel, dim3((unsigned)a.count * KS_DPARTS), dim3(256), 0, s, a, dig, rowsum, mpad,
                       split > 1 ? 1 : 0);
    hipLaunchKernelGGL(ks32_mfma_kernel, dim3((unsigned)(jpad / 64), (unsigned)(cpad / 64), split), dim3(256), 0, s, a,
                       dig, rowsum, kt, mpad, jpad);
    return hipGetLastError();
}

bool keyswitch32_scalar_supported(int base_log, int level) {
    return base_log >= 1 && base_log <= 15 && level >= 1 && level <= KS_MAXL && base_log * level <= 30;
}

hipError_t launch_keyswitch32(const Keyswitch32Launch &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    if (!keyswitch32_scalar_supported(a.base_log, a.level)) return hipErrorInvalidValue;
    dim3 grid((a.out_dim + 1 + KS_TJ - 1) / KS_TJ, (a.count + KS_TC - 1) / KS_TC);
    hipLaunchKernelGGL(keyswitch32_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
