// lwe_ingress.hip -- compressed ciphertext ingress: expanded LWE rows written on the GPU from the two forms a
// client uploads (the ciphertext half).
//
//   compact list   expand_lwe_compact_ciphertext_list (core_crypto/algorithms/
//                  lwe_compact_ciphertext_list_expansion.rs:12-58): the container holds one mask per bin of n
//                  ciphertexts, then one body per ciphertext.  Row i of bin b = i / n, t = i % n has the mask
//                  mask[b] * X^(n - (t + 1)) in Z[X]/(X^n + 1) (polynomial_wrapping_monic_monomial_mul_assign):
//                  with d = n - (t + 1), out[j] = -mask[b][j + n - d] for j < d, mask[b][j - d] otherwise.
//   seeded rows    decompress_seeded_lwe_ciphertext (seeded_lwe_ciphertext_decompression.rs:50-73), a batch of
//                  them: row r's mask is bytes [1, 1 + 8n) of the AES-CTR stream keyed with ITS seed, so the
//                  round keys are expanded on the device, per row, into LDS.
//   seeded list    decompress_seeded_lwe_ciphertext_list (seeded_lwe_ciphertext_list_decompression.rs:13-100):
//                  one stream for all rows; csprng.hip's mask and body kernels serve it from the tables that
//                  aes_schedule_kernel writes for a seed that is device data.
//
// Rows are n + 1 words, so every second row of an output starts at 8 modulo 16: the compact kernel stores
// 16 bytes per lane from the first 16-byte boundary of the row and the odd word in front or behind alone.
#include "aes_device.h"
#include "engine.h"

namespace tfhe_mi355 {

// one workgroup per row, rows grid-strided; write-bound (the bin masks stay in L2)
__global__ void __launch_bounds__(256) lwe_compact_expand_kernel(const uint64_t *__restrict__ masks,
                                                                 const uint64_t *__restrict__ bodies, size_t n,
                                                                 size_t first, size_t count,
                                                                 uint64_t *__restrict__ out) {
    for (size_t r = blockIdx.x; r < count; r += gridDim.x) {
        const size_t i = first + r, t = i % n;
        const size_t d = n - (t + 1);
        const uint64_t *m = masks + (i / n) * n;
        uint64_t *row = out + r * (n + 1);
        auto word = [&](size_t j) -> uint64_t {
            if (j == n) return bodies[r];
            return j < d ? (uint64_t)0 - m[j + n - d] : m[j - d];
        };
        const size_t head = ((uintptr_t)row >> 3) & 1;  // a row at 8 mod 16: one word, then 16-byte pairs
        const size_t pairs = (n + 1 - head) / 2;
        if (threadIdx.x == 0 && head) row[0] = word(0);
        for (size_t p = threadIdx.x; p < pairs; p += 256) {
            const size_t j = head + 2 * p;
            *reinterpret_cast<ulonglong2 *>(row + j) = make_ulonglong2(word(j), word(j + 1));
        }
        if (threadIdx.x == 0 && ((n + 1 - head) & 1)) row[n] = word(n);
    }
}

hipError_t launch_lwe_compact_expand(const uint64_t *d_masks, const uint64_t *d_bodies, size_t n, size_t first,
                                     size_t count, uint64_t *d_out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min(std::min<size_t>(count, (size_t)1 << 20), grid_cap());
    hipLaunchKernelGGL(lwe_compact_expand_kernel, dim3(grid), dim3(256), 0, s, d_masks, d_bodies, n, first, count,
                       d_out);
    return hipGetLastError();
}

// the tables of a seed held in device memory: Te0 and the S-box copied, the round keys expanded by one thread
__global__ void __launch_bounds__(256) aes_schedule_kernel(const AesTables *__restrict__ base,
                                                           const uint64_t *__restrict__ seed,
                                                           AesTables *__restrict__ tab) {
    tab->te0[threadIdx.x] = base->te0[threadIdx.x];
    tab->sbox[threadIdx.x] = base->sbox[threadIdx.x];
    if (threadIdx.x == 0) {
        const uint32_t key[4] = {(uint32_t)seed[0], (uint32_t)(seed[0] >> 32), (uint32_t)seed[1],
                                 (uint32_t)(seed[1] >> 32)};
        uint32_t rk[44];
        aes128_expand_key(base->sbox, key, rk);
        for (int i = 0; i < 44; i++) tab->rk[i] = rk[i];
    }
}

hipError_t launch_aes_schedule(const void *d_base_tables, const uint64_t *d_seed, void *d_tables, hipStream_t s) {
    hipLaunchKernelGGL(aes_schedule_kernel, dim3(1), dim3(256), 0, s,
                       reinterpret_cast<const AesTables *>(d_base_tables), d_seed,
                       reinterpret_cast<AesTables *>(d_tables));
    return hipGetLastError();
}

// One workgroup per row (rows grid-strided).  Thread 0 expands the row's key schedule into LDS and writes
// the body; then each pass encrypts 256 consecutive counters, thread t counter a = A + t: its bytes 1..8 are
// mask word 2a, its bytes 9..15 with byte 0 of counter a + 1 (handed over through LDS) are word 2a + 1.
// The last thread of a pass only hands its byte over, so a pass writes 510 words, 16 contiguous bytes a lane.
__global__ void __launch_bounds__(256) csprng_rows_kernel(const AesTables *__restrict__ base,
                                                          const uint64_t *__restrict__ seeds,
                                                          const uint64_t *__restrict__ bodies, size_t n, size_t count,
                                                          uint64_t *__restrict__ out) {
    __shared__ uint32_t te[256];
    __shared__ uint8_t sb[256];
    __shared__ uint32_t rk[44];
    __shared__ uint8_t next0[2][256];
    const unsigned tid = threadIdx.x;
    te[tid] = base->te0[tid];
    sb[tid] = base->sbox[tid];
    __syncthreads();
    const size_t last = (n + 1) / 2;  // the highest counter touching words [0, n)
    for (size_t r = blockIdx.x; r < count; r += gridDim.x) {
        uint64_t *row = out + r * (n + 1);
        if (tid == 0) {
            const uint64_t lo = seeds[2 * r], hi = seeds[2 * r + 1];
            const uint32_t key[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            aes128_expand_key(sb, key, rk);
            row[n] = bodies[r];
        }
        __syncthreads();
        int buf = 0;
        for (size_t A = 0; 2 * A < n; A += 255, buf ^= 1) {
            const size_t a = A + tid;
            uint32_t s[4] = {(uint32_t)a, (uint32_t)((uint64_t)a >> 32), 0u, 0u};  // u128 counter, LE
            if (a <= last) aes128_encrypt_block(rk, te, sb, s);
            next0[buf][tid] = (uint8_t)s[0];
            __syncthreads();
            if (tid < 255) {
                const uint64_t lo = (uint64_t)s[0] | ((uint64_t)s[1] << 32), hi = (uint64_t)s[2] | ((uint64_t)s[3] << 32);
                const size_t w0 = 2 * a;
                if (w0 < n) row[w0] = (lo >> 8) | (hi << 56);
                if (w0 + 1 < n) row[w0 + 1] = (hi >> 8) | ((uint64_t)next0[buf][tid + 1] << 56);
            }
        }
        __syncthreads();  // the next row rewrites rk
    }
}

hipError_t launch_csprng_rows(const void *d_base_tables, const uint64_t *d_seeds, const uint64_t *d_bodies, size_t n,
                              size_t count, uint64_t *d_out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min(std::min<size_t>(count, (size_t)1 << 20), grid_cap());
    hipLaunchKernelGGL(csprng_rows_kernel, dim3(grid), dim3(256), 0, s,
                       reinterpret_cast<const AesTables *>(d_base_tables), d_seeds, d_bodies, n, count, d_out);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
