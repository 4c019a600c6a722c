// lwe_ops.hip -- batched LWE linear algebra and trivial PBS on device, for the integer layer
// (tfhe_mi355/integer.py) keeping radix ciphertexts resident in HBM between PBS layers.
//
// Replaces, batched over rows of u64 words:
//   shortint unchecked_add_assign / unchecked_scalar_mul_assign
//       (core_crypto/algorithms/lwe_linear_algebra.rs: lwe_ciphertext_add_assign,
//        lwe_ciphertext_cleartext_mul_assign; shortint/server_key/add.rs, scalar_mul.rs)
//   the bivariate packing  left = left * factor + right  (shortint/server_key/bivariate_pbs.rs:167-182)
//   trivial_pbs_assign     (shortint/server_key/mod.rs:763-781)
// All arithmetic is wrapping mod 2^64, as the reference's.
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "fft_device.h"

namespace tfhe_mi355 {

// y[r][w] = y[r][w] * scalar + (x ? x[r][w] : 0)
__global__ void __launch_bounds__(256) lwe_scalar_mul_add_kernel(uint64_t *__restrict__ y, const uint64_t *__restrict__ x,
                                                                 uint64_t scalar, size_t rows, size_t words,
                                                                 size_t y_stride, size_t x_stride) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * words) return;
    const size_t r = e / words, w = e % words;
    uint64_t v = y[r * y_stride + w] * scalar;
    if (x) v += x[r * x_stride + w];
    y[r * y_stride + w] = v;
}

// One layer of block arithmetic in one launch: for the op of blockIdx.y, every row r < rows and word w < words,
//   dst[r][w] = sum over the present terms of scalar_t * src_t[r][w] + (w == words - 1 ? body_add : 0).
// Replaces, for a whole layer of a radix DAG at once, the packing / subtraction / negation with its correcting
// term that the reference runs block by block between two PBS layers (pack_block_chunk, compare_block_assign:
// integer/server_key/comparator.rs:182-220; unchecked_neg_assign: radix/neg.rs:56-73) and the copies around the
// batched PBS.  The table travels by value in the kernel arguments and is indexed by blockIdx.y alone, so an
// entry is read with scalar loads; lanes run along w (8-byte accesses, 512 B per wave: rows are only 8-byte
// aligned, lwe_size being odd).  Tiles of 256 words are handed out grid-stride over (row, tile of the row); a
// term that is the destination itself (same pointer, same stride) is read and written by the same lane.
struct BlockLayerTable {
    BlockLayerOp op[BLOCK_LAYER_OPS_PER_LAUNCH];
};

__global__ void __launch_bounds__(256) lwe_block_layer_kernel(const BlockLayerTable table, uint32_t rows, uint32_t words,
                                                              uint32_t tiles_per_row) {
    const BlockLayerOp &op = table.op[blockIdx.y];
    const uint32_t tiles = rows * tiles_per_row;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t r = t / tiles_per_row;
        const uint32_t w = (t - r * tiles_per_row) * 256 + threadIdx.x;
        if (w >= words) continue;
        uint64_t v = w + 1 == words ? op.body_add : 0;
#pragma unroll
        for (int i = 0; i < BLOCK_LAYER_TERMS; i++)
            if (op.term[i].src) v += op.term[i].scalar * op.term[i].src[(size_t)r * op.term[i].stride + w];
        op.dst[(size_t)r * op.dst_stride + w] = v;
    }
}

// The block layer with a clear digit per row: lwe_block_layer_kernel's loop, and for the row of the tile
//   digit = ((negate ? 0 - d_clear[r] : d_clear[r]) >> clear_shift) & (2^clear_bits - 1)
// times clear_scale on the body, lut_base + digit into d_lut_index[r].  Replaces the plaintext a scalar's digit
// adds to or subtracts from a block before the LUT (radix/scalar_add.rs:53-65, scalar_sub.rs:109-122,
// comparator.rs:226-238) and the choice of the LUT by the digit (radix_parallel/scalar_bitwise_op.rs,
// scalar_comparison.rs:312-336), which the reference does on the host per scalar.  A second kernel, not a
// template of the first: the plain kernel's code stays as it is.  The row of a tile is the same for the whole
// workgroup, so d_clear[r] is one uniform load per tile; the lane of w == words - 1 adds the plaintext, lane 0 of
// the row's first tile (w == 0 < words) stores the index, once per row.
struct ClearBlockLayerTable {
    ClearBlockLayerOp op[CLEAR_BLOCK_LAYER_OPS_PER_LAUNCH];
};
static_assert(sizeof(ClearBlockLayerTable) + 3 * sizeof(uint32_t) <= 4096, "the table travels in the kernel arguments");

__global__ void __launch_bounds__(256) lwe_clear_block_layer_kernel(const ClearBlockLayerTable table, uint32_t rows,
                                                                    uint32_t words, uint32_t tiles_per_row) {
    const ClearBlockLayerOp &c = table.op[blockIdx.y];
    const BlockLayerOp &op = c.op;
    const uint32_t tiles = rows * tiles_per_row;
    const uint64_t mask = ((uint64_t)1 << c.clear_bits) - 1;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t r = t / tiles_per_row;
        const uint32_t tile = t - r * tiles_per_row;
        const uint32_t w = tile * 256 + threadIdx.x;
        uint64_t digit = 0;
        if (c.d_clear) {
            const uint64_t clear = c.d_clear[r];
            digit = ((c.clear_negate ? 0 - clear : clear) >> c.clear_shift) & mask;
        }
        if (c.d_lut_index && tile == 0 && threadIdx.x == 0) c.d_lut_index[r] = c.lut_base + (uint32_t)digit;
        if (w >= words) continue;
        uint64_t v = w + 1 == words ? op.body_add + digit * c.clear_scale : 0;
#pragma unroll
        for (int i = 0; i < BLOCK_LAYER_TERMS; i++)
            if (op.term[i].src) v += op.term[i].scalar * op.term[i].src[(size_t)r * op.term[i].stride + w];
        op.dst[(size_t)r * op.dst_stride + w] = v;
    }
}

// trivial ciphertexts (zero mask): body <- LUT body at the box of body / delta (negated past the
// padding bit); the mask stays zero
__global__ void __launch_bounds__(256) trivial_pbs_kernel(uint64_t *__restrict__ body, size_t rows, size_t stride,
                                                          const uint64_t *__restrict__ lut_body, uint64_t delta,
                                                          uint64_t modulus_sup, uint64_t box) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint64_t value = body[r * stride] / delta;
    const uint64_t entry = lut_body[(value % modulus_sup) * box];
    body[r * stride] = value >= modulus_sup ? 0 - entry : entry;
}

// words[0, n) = 0: the reset of a launcher's ticket and flag words (engine.h launch_zero_words)
__global__ void __launch_bounds__(256) zero_words_kernel(uint32_t *__restrict__ words, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) words[e] = 0;
}

// Diagnostic: the PBS kernels' backward torus conversion (fft_device.h frac_to_torus) applied to
// given fractions: acc[i] += X(fr[i]) and set[i] = X(fr[i]), X = rint(fr * 2^64) mod 2^64.
__global__ void __launch_bounds__(256) torus_from_fraction_kernel(const double *__restrict__ fr,
                                                                  uint64_t *__restrict__ acc,
                                                                  uint64_t *__restrict__ set, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double k32 = torus_k32();
    if (e >= n) return;
    uint64_t c = acc[e];
    torus_add_frac(c, fr[e], k32);
    acc[e] = c;
    set[e] = torus_from_frac(fr[e], k32);
}

// ---- glue of bit extraction and circuit bootstrap (wop_pbs/mod.rs:158-224, 369-444) ----------------
// dst[r][w] = (src[r / reps][w] << shift) + (body ? body_add : 0): the shift on the padding bit
// (extract_bits :160-166), the cleartext multiplication by 2^(63 - delta_log) with q/4 on the body,
// one copy per circuit-bootstrap level (homomorphic_shift_boolean :398-407), and the store of the
// keyswitch output into its slot of the output list (:182-184, shift 0)
__global__ void __launch_bounds__(256) wop_shift_rows_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src,
                                                             size_t rows, size_t words, size_t dst_stride, size_t reps,
                                                             int shift, uint64_t body_add) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * words) return;
    const size_t r = e / words, w = e % words;
    dst[r * dst_stride + w] = (src[(r / reps) * words + w] << shift) + (w + 1 == words ? body_add : 0);
}

// body of row r += 2^(first - step * (r % mod))  (:194, :219, :442-443)
__global__ void __launch_bounds__(256) wop_add_body_kernel(uint64_t *__restrict__ buf, size_t rows, size_t words,
                                                           int first, int step, size_t mod) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    buf[r * words + words - 1] += (uint64_t)1 << (first - step * (int)(r % mod));
}

// cur -= x + (body ? body_add : 0)  (:219-223)
__global__ void __launch_bounds__(256) wop_sub_rows_kernel(uint64_t *__restrict__ cur, const uint64_t *__restrict__ x,
                                                           size_t rows, size_t words, uint64_t body_add) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * words) return;
    cur[e] -= x[e] + (e % words + 1 == words ? body_add : 0);
}

// LUT l = trivial GLWE, body all -2^(first - step * l) (:198-205, :423-427); lut_indexes[r] = r % nluts
__global__ void __launch_bounds__(256) wop_fill_luts_kernel(uint64_t *__restrict__ luts, size_t nluts, size_t glwe,
                                                            size_t body_off, int first, int step,
                                                            uint32_t *__restrict__ lut_indexes, size_t rows) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nluts * glwe) {
        const size_t l = e / glwe, w = e % glwe;
        luts[e] = w < body_off ? 0 : 0 - ((uint64_t)1 << (first - step * (int)l));
    }
    if (lut_indexes && e < rows) lut_indexes[e] = (uint32_t)(e % nluts);
}

hipError_t launch_wop_shift_rows(uint64_t *dst, const uint64_t *src, size_t rows, size_t words, size_t dst_stride,
                                 size_t reps, int shift, uint64_t body_add, hipStream_t s) {
    const size_t n = rows * words;
    if (n == 0) return hipSuccess;
    if (shift < 0 || shift > 63 || reps == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wop_shift_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, rows,
                       words, dst_stride, reps, shift, body_add);
    return hipGetLastError();
}

hipError_t launch_wop_add_body(uint64_t *buf, size_t rows, size_t words, int first, int step, size_t mod,
                               hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (mod == 0 || first > 63 || first - step * (int)(mod - 1) < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wop_add_body_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, buf, rows, words,
                       first, step, mod);
    return hipGetLastError();
}

hipError_t launch_wop_sub_rows(uint64_t *cur, const uint64_t *x, size_t rows, size_t words, uint64_t body_add,
                               hipStream_t s) {
    const size_t n = rows * words;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(wop_sub_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cur, x, rows, words,
                       body_add);
    return hipGetLastError();
}

hipError_t launch_wop_fill_luts(uint64_t *luts, size_t nluts, size_t glwe, size_t body_off, int first, int step,
                                uint32_t *lut_indexes, size_t rows, hipStream_t s) {
    if (nluts == 0) return hipSuccess;
    if (first > 63 || first - step * (int)(nluts - 1) < 0) return hipErrorInvalidValue;
    const size_t n = std::max(nluts * glwe, lut_indexes ? rows : 0);
    hipLaunchKernelGGL(wop_fill_luts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, luts, nluts, glwe,
                       body_off, first, step, lut_indexes, rows);
    return hipGetLastError();
}

hipError_t launch_zero_words(uint32_t *words, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n > ((size_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, words, n);
    return hipGetLastError();
}

hipError_t launch_torus_from_fraction(const double *fr, uint64_t *acc, uint64_t *set, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(torus_from_fraction_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fr, acc, set, n);
    return hipGetLastError();
}

hipError_t launch_lwe_scalar_mul_add(uint64_t *y, const uint64_t *x, uint64_t scalar, size_t rows, size_t words,
                                     size_t y_stride, size_t x_stride, hipStream_t s) {
    const size_t n = rows * words;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(lwe_scalar_mul_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, x, scalar,
                       rows, words, y_stride, x_stride);
    return hipGetLastError();
}

hipError_t launch_lwe_block_layer(const BlockLayerOp *ops, size_t n_ops, size_t rows, size_t words, hipStream_t s) {
    if (n_ops == 0 || rows == 0 || words == 0) return hipSuccess;
    const size_t tiles_per_row = (words + 255) / 256;
    if (words > 0xFFFFFFFFull || rows > 0xFFFFFFFFull / tiles_per_row) return hipErrorInvalidValue;
    const size_t tiles = rows * tiles_per_row;
    // lists longer than one table: several launches, in stream order
    for (size_t first = 0; first < n_ops; first += BLOCK_LAYER_OPS_PER_LAUNCH) {
        const size_t n = std::min(n_ops - first, (size_t)BLOCK_LAYER_OPS_PER_LAUNCH);
        BlockLayerTable table;
        std::memset(&table, 0, sizeof table);
        std::memcpy(table.op, ops + first, n * sizeof(BlockLayerOp));
        // about eight workgroups per compute unit over the whole launch; the grid-stride loop takes the rest
        const size_t per_op = std::max((size_t)1, BLOCK_LAYER_MAX_WORKGROUPS / n);
        hipLaunchKernelGGL(lwe_block_layer_kernel, dim3((unsigned)std::min(tiles, per_op), (unsigned)n), dim3(256), 0, s,
                           table, (uint32_t)rows, (uint32_t)words, (uint32_t)tiles_per_row);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_lwe_clear_block_layer(const ClearBlockLayerOp *ops, size_t n_ops, size_t rows, size_t words,
                                        hipStream_t s) {
    if (n_ops == 0 || rows == 0 || words == 0) return hipSuccess;
    const size_t tiles_per_row = (words + 255) / 256;
    if (words > 0xFFFFFFFFull || rows > 0xFFFFFFFFull / tiles_per_row) return hipErrorInvalidValue;
    const size_t tiles = rows * tiles_per_row;
    // lists longer than one table: several launches, in stream order
    for (size_t first = 0; first < n_ops; first += CLEAR_BLOCK_LAYER_OPS_PER_LAUNCH) {
        const size_t n = std::min(n_ops - first, (size_t)CLEAR_BLOCK_LAYER_OPS_PER_LAUNCH);
        ClearBlockLayerTable table;
        std::memset(&table, 0, sizeof table);
        std::memcpy(table.op, ops + first, n * sizeof(ClearBlockLayerOp));
        // the plain layer's grid: about eight workgroups per compute unit, the grid-stride loop takes the rest
        const size_t per_op = std::max((size_t)1, BLOCK_LAYER_MAX_WORKGROUPS / n);
        hipLaunchKernelGGL(lwe_clear_block_layer_kernel, dim3((unsigned)std::min(tiles, per_op), (unsigned)n), dim3(256),
                           0, s, table, (uint32_t)rows, (uint32_t)words, (uint32_t)tiles_per_row);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_trivial_pbs(uint64_t *body, size_t rows, size_t stride, const uint64_t *lut_body, uint64_t delta,
                              uint64_t modulus_sup, uint64_t box, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(trivial_pbs_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, body, rows, stride,
                       lut_body, delta, modulus_sup, box);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
