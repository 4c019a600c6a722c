// Issue rate of the 32-bit integer multiplies of gfx950 that csrc/glwe_mult.hip is made of, against
// v_add_u32: eight independent chains per lane, four waves per SIMD on every CU, inline asm so that
// the instruction under test is the one that runs.  Prints ns per wave-instruction per SIMD and the
// ratio to v_add_u32.
//   hipcc --offload-arch=gfx950 -O2 -o scripts/probes/imul_rate_probe scripts/probes/imul_rate_probe.hip && scripts/probes/imul_rate_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

constexpr int ITERS = 4096, CHAINS = 8;

#define PROBE32(name, text)                                                                         \
    __global__ void __launch_bounds__(256) name(uint32_t *out, uint32_t seed) {                      \
        uint32_t x[CHAINS], y = seed + threadIdx.x;                                                  \
        for (int c = 0; c < CHAINS; c++) x[c] = y * (c + 3);                                         \
        for (int i = 0; i < ITERS; i++)                                                              \
            for (int c = 0; c < CHAINS; c++) asm volatile(text " %0, %0, %1" : "+v"(x[c]) : "v"(y)); \
        uint32_t s = 0;                                                                              \
        for (int c = 0; c < CHAINS; c++) s ^= x[c];                                                  \
        out[blockIdx.x * 256 + threadIdx.x] = s;                                                     \
    }
#define PROBE64(name, text)                                                                                           \
    __global__ void __launch_bounds__(256) name(uint32_t *out, uint32_t seed) {                                        \
        uint64_t x[CHAINS];                                                                                            \
        uint32_t y = seed + threadIdx.x, z = seed * 7 + threadIdx.x;                                                   \
        for (int c = 0; c < CHAINS; c++) x[c] = (uint64_t)y * (c + 3);                                                 \
        for (int i = 0; i < ITERS; i++)                                                                                \
            for (int c = 0; c < CHAINS; c++) asm volatile(text " %0, vcc, %1, %2, %0" : "+v"(x[c]) : "v"(y), "v"(z) : "vcc"); \
        uint64_t s = 0;                                                                                                \
        for (int c = 0; c < CHAINS; c++) s ^= x[c];                                                                    \
        out[blockIdx.x * 256 + threadIdx.x] = (uint32_t)(s ^ (s >> 32));                                               \
    }

PROBE32(k_add_u32, "v_add_u32")
PROBE32(k_mul_lo_u32, "v_mul_lo_u32")
PROBE32(k_mul_hi_u32, "v_mul_hi_u32")
PROBE32(k_mul_u32_u24, "v_mul_u32_u24")
PROBE64(k_mad_u64_u32, "v_mad_u64_u32")
PROBE64(k_mad_i64_i32, "v_mad_i64_i32")

template <class K>
static double run(K kernel, uint32_t *out, int blocks) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    double best = 1e30;
    for (int rep = 0; rep < 6; rep++) {  // the first two warm up
        hipEventRecord(a, 0);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, out, (uint32_t)rep + 1);
        hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) return -1;
        float ms = 0;
        hipEventElapsedTime(&ms, a, b);
        if (rep >= 2 && ms < best) best = ms;
    }
    return best;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount, blocks = cus * 4;  // 16 waves per CU, 4 per SIMD
    uint32_t *out;
    if (hipMalloc(&out, (size_t)blocks * 256 * 4) != hipSuccess) return 1;
    const double per_simd = 4.0 * ITERS * CHAINS;  // wave-instructions each SIMD issues
    struct { const char *name; double ms; } r[] = {
        {"v_add_u32", run(k_add_u32, out, blocks)},         {"v_mul_lo_u32", run(k_mul_lo_u32, out, blocks)},
        {"v_mul_hi_u32", run(k_mul_hi_u32, out, blocks)},   {"v_mul_u32_u24", run(k_mul_u32_u24, out, blocks)},
        {"v_mad_u64_u32", run(k_mad_u64_u32, out, blocks)}, {"v_mad_i64_i32", run(k_mad_i64_i32, out, blocks)}};
    printf("{\"cus\": %d, \"waves_per_simd\": 4, \"rates\": {", cus);
    for (size_t i = 0; i < sizeof r / sizeof r[0]; i++)
        printf("%s\"%s\": {\"ns_per_wave_instruction\": %.3f, \"vs_add\": %.2f}", i ? ", " : "", r[i].name,
               r[i].ms * 1e6 / per_simd, r[i].ms / r[0].ms);
    printf("}}\n");
    hipFree(out);
    return 0;
}
