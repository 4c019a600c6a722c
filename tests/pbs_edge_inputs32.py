"""The n = 1 crafted case of pbs_edge_inputs.py transposed to the 32-bit torus (test_boolean.py,
test_boolean_gpu.py).

The worst-case words of a (base_log, level) decomposition with base_log * level <= 30 live in the top 32
bits of the u64 families (the rounding bit is 63 - base_log * level >= 33), so D32 = D64 >> 32 has the
same digits; the accumulator with X acc - acc = D32 is solved mod 2^32.  With acc as the LUT, mask word
unit_mask32(N) (a~ = 1) and body 0 the first and only CMUX decomposes exactly D32: ties, carries, the
+2^(B-1) digit and the rounding overflow.
"""
import numpy as np

from pbs_edge_inputs import edge_positions, pbs_edge_words

U32 = np.uint32


def unit_mask32(N):
    """the u32 mask word whose modulus switch to 2N is 1."""
    return U32(1 << (32 - (2 * N).bit_length() + 1))


def negacyclic_mul_x32(p):
    return np.concatenate([(U32(0) - p[..., -1:]).astype(U32), p[..., :-1]], axis=-1)


def crafted_lut32(D, free, seed=0):
    """(acc, D'): acc [(k+1)][N] u32 with X acc - acc = D' mod 2^32; D' = D up to bit 0 of one free word per
    polynomial whose sum is odd."""
    D = np.array(D, dtype=U32)
    rng = np.random.default_rng(seed)
    cand = np.nonzero(free)[0]
    for row in D:
        if int(np.sum(row, dtype=np.uint64)) & 1:
            row[rng.choice(cand)] ^= U32(1)
    tail = np.cumsum(D[:, 1:].astype(np.uint64), axis=1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    twice = (tail[:, -1] - D[:, 0].astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    assert not (twice & np.uint64(1)).any()
    acc = np.empty(D.shape, dtype=np.uint64)
    acc[:, 0] = twice >> np.uint64(1)
    acc[:, 1:] = (acc[:, :1] - tail) & np.uint64(0xFFFFFFFF)
    acc = acc.astype(U32)
    assert np.array_equal((negacyclic_mul_x32(acc) - acc).astype(U32), D)
    return acc, D


def crafted_case32(B, L, N, k, seed):
    """(cts [3][2] u32, lut [(k+1) N] u32, D [(k+1)][N] u32): a~ = 1 with b = 0 (the CMUX decomposes D),
    b~ = N (-D) and b~ = 2N (D again, through the body's rounding overflow)."""
    assert B * L <= 30
    D = np.stack([(pbs_edge_words(B, L, N, seed + r) >> np.uint64(32)).astype(U32) for r in range(k + 1)])
    acc, D = crafted_lut32(D, ~edge_positions(N), seed)
    cts = np.empty((3, 2), dtype=U32)
    cts[:, 0] = unit_mask32(N)
    cts[:, 1] = [0, 1 << 31, (1 << 32) - 1]
    return cts, acc.ravel(), D
