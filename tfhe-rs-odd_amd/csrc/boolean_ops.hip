// boolean_ops.hip -- the linear parts of the reference's boolean gates on u32 LWE rows (gfx950).
//
// tfhe/src/boolean/engine/mod.rs: every binary gate is a linear combination of its two inputs and a
// constant added to the body, followed by a bootstrap with the constant-T accumulator
// (apply_bootstrapping_pattern, bootstrapping.rs:392-401).  With T = PLAINTEXT_TRUE = 1 << 29 and
// F = PLAINTEXT_FALSE = 7 << 29 (boolean/mod.rs:77-80), all arithmetic wrapping mod 2^32:
//   AND   (a + b) + F       mod.rs:633-641        OR    (a + b) + T        mod.rs:749-755
//   NAND -(a + b) + T       mod.rs:672-679        XOR   2 (a + b) + 2T     mod.rs:786-795
//   NOR  -(a + b) + F       mod.rs:710-718        XNOR -2 (a + b) - 2T     mod.rs:826-837
// MUX (mod.rs:515-543): cond + then + F and -cond + else + F before the two bootstraps,
// pbs1 + pbs2 + T after them.  NOT negates every word (mod.rs:377-398).
#include <algorithm>

#include "engine.h"
#include "fft_device.h"

namespace tfhe_mi355 {

namespace {
constexpr uint32_t BOOL_T = 1u << 29, BOOL_F = 7u << 29;
}

// one mixed batch: item i = blockIdx.y, opcode ops[i] (0 AND, 1 NAND, 2 NOR, 3 OR, 4 XOR, 5 XNOR)
__global__ void __launch_bounds__(256) bool_gates_prologue_kernel(const uint8_t *__restrict__ ops,
                                                                  const uint32_t *__restrict__ lhs,
                                                                  const uint32_t *__restrict__ rhs,
                                                                  uint32_t *__restrict__ out, size_t words) {
    const size_t i = blockIdx.y;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint32_t s, c;
    switch (ops[i]) {
    case 0: s = 1u, c = BOOL_F; break;
    case 1: s = 0u - 1u, c = BOOL_T; break;
    case 2: s = 0u - 1u, c = BOOL_F; break;
    case 3: s = 1u, c = BOOL_T; break;
    case 4: s = 2u, c = 2u * BOOL_T; break;
    case 5: s = 0u - 2u, c = 0u - 2u * BOOL_T; break;
    default: s = 0u, c = 0u; break;  // refused by the host-pointer entry point
    }
    const size_t e = i * words + w;
    out[e] = s * (lhs[e] + rhs[e]) + (w == words - 1 ? c : 0u);
}

__global__ void __launch_bounds__(256) bool_mux_prologue_kernel(const uint32_t *__restrict__ cond,
                                                                const uint32_t *__restrict__ then_,
                                                                const uint32_t *__restrict__ else_,
                                                                uint32_t *__restrict__ out, size_t words) {
    const size_t i = blockIdx.y;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const size_t e = i * words + w;
    const uint32_t f = w == words - 1 ? BOOL_F : 0u;
    out[2 * i * words + w] = cond[e] + then_[e] + f;
    out[(2 * i + 1) * words + w] = (0u - cond[e]) + else_[e] + f;
}

__global__ void __launch_bounds__(256) bool_mux_epilogue_kernel(const uint32_t *__restrict__ in,
                                                                uint32_t *__restrict__ out, size_t words) {
    const size_t i = blockIdx.y;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    out[i * words + w] = in[2 * i * words + w] + in[(2 * i + 1) * words + w] + (w == words - 1 ? BOOL_T : 0u);
}

__global__ void __launch_bounds__(256) bool_negate_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                          size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) out[e] = 0u - in[e];
}

// diagnostic (tfhe_mi355_debug_torus32_from_fraction): the backward conversion's last step alone
__global__ void __launch_bounds__(256) torus32_from_fraction_kernel(const double *__restrict__ fr,
                                                                    uint32_t *__restrict__ acc,
                                                                    uint32_t *__restrict__ set, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t x = torus32_from_frac(fr[e]);
    acc[e] += x;
    set[e] = x;
}

namespace {
// rows in grid.y, 65535 at a time
template <class F>
hipError_t for_row_slices(size_t count, F &&f) {
    for (size_t r0 = 0; r0 < count; r0 += 65535) {
        f(r0, (unsigned)std::min<size_t>(65535, count - r0));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_bool_gates_prologue(const uint8_t *ops, const uint32_t *lhs, const uint32_t *rhs, uint32_t *out,
                                      size_t count, size_t words, hipStream_t s) {
    const unsigned bx = (unsigned)((words + 255) / 256);
    return for_row_slices(count, [&](size_t r0, unsigned rows) {
        hipLaunchKernelGGL(bool_gates_prologue_kernel, dim3(bx, rows), dim3(256), 0, s, ops + r0, lhs + r0 * words,
                           rhs + r0 * words, out + r0 * words, words);
    });
}

hipError_t launch_bool_mux_prologue(const uint32_t *cond, const uint32_t *then_, const uint32_t *else_, uint32_t *out,
                                    size_t count, size_t words, hipStream_t s) {
    const unsigned bx = (unsigned)((words + 255) / 256);
    return for_row_slices(count, [&](size_t r0, unsigned rows) {
        hipLaunchKernelGGL(bool_mux_prologue_kernel, dim3(bx, rows), dim3(256), 0, s, cond + r0 * words,
                           then_ + r0 * words, else_ + r0 * words, out + 2 * r0 * words, words);
    });
}

hipError_t launch_bool_mux_epilogue(const uint32_t *in, uint32_t *out, size_t count, size_t words, hipStream_t s) {
    const unsigned bx = (unsigned)((words + 255) / 256);
    return for_row_slices(count, [&](size_t r0, unsigned rows) {
        hipLaunchKernelGGL(bool_mux_epilogue_kernel, dim3(bx, rows), dim3(256), 0, s, in + 2 * r0 * words,
                           out + r0 * words, words);
    });
}

hipError_t launch_bool_negate(const uint32_t *in, uint32_t *out, size_t total, hipStream_t s) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(bool_negate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, total);
    return hipGetLastError();
}

hipError_t launch_torus32_from_fraction(const double *fr, uint32_t *acc, uint32_t *set, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(torus32_from_fraction_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fr, acc, set,
                       n);
    return hipGetLastError();
}

}  // namespace tfhe_mi355
