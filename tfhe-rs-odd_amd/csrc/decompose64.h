// decompose64.h -- the 64-bit SignedDecomposer shared by the integer kernels (keyswitch.hip,
// pfpks.hip, glwe_mult.hip): closest_representable (commons/math/decomposition/decomposer.rs:99-119)
// and one step of the balanced digit iteration (iter.rs:134-141), least significant digit (level L)
// first.  1 <= base_log, base_log * level <= 63.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfhe_mi355 {

__device__ __forceinline__ uint64_t closest_repr(uint64_t x, int base_log, int level) {
    int shift = 64 - base_log * level - 1;
    uint64_t res = x >> shift;
    res += 1;
    res &= ~(uint64_t)1;
    return res << shift;
}

// state = closest_repr(x) >> (64 - base_log * level) before the first call; mask = 2^base_log - 1
__device__ __forceinline__ int64_t signed_digit64(uint64_t &state, int beta, uint64_t mask) {
    uint64_t res = state & mask;
    state >>= beta;
    uint64_t carry = ((res - 1) | state) & res;
    carry >>= beta - 1;
    state += carry;
    return (int64_t)(res - (carry << beta));
}

}  // namespace tfhe_mi355
