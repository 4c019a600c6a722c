"""Inputs shared by the CPU and GPU tests of the 128-bit-torus PBS (test infrastructure)."""
from __future__ import annotations

import math
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tfhe-rs-odd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pbs128_reference as R  # noqa: E402
from tfhe_mi355.parameters import ClassicPBSParameters  # noqa: E402

GLWE_STD = 8.6457178e-32  # TEST_PARAMS_4_BITS_NATIVE_U128


def params(n: int, N: int, k: int, level: int, base_log: int) -> ClassicPBSParameters:
    return ClassicPBSParameters(lwe_dimension=n, glwe_dimension=k, polynomial_size=N, lwe_modular_std_dev=2.0 ** -70,
                                glwe_modular_std_dev=GLWE_STD, pbs_base_log=base_log, pbs_level=level, ks_base_log=3,
                                ks_level=5, message_modulus=16, carry_modulus=1, name=f"u128_{N}_{k}_{level}_{base_log}")


def forward_edge_words() -> list:
    """0, 1, 2^127 - 1, 2^127, 2^128 - 1 and values around 2^104 (the branch in u128_to_f64) and 2^53."""
    e = [0, 1, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, (1 << 128) - 1, (1 << 128) - 2]
    for p in (53, 54, 104, 105, 106, 126):
        for d in (-2, -1, 0, 1, 2):
            e += [(1 << p) + d, (1 << 128) - (1 << p) + d, (1 << p) + (1 << (p - 53)) + d, (3 << (p - 1)) + d]
    return e


def _dd(x_num: int, x_log_den: int):
    """The normalised double-double of the dyadic rational x_num / 2^x_log_den (exact when it fits)."""
    from fractions import Fraction

    x = Fraction(x_num, 1 << x_log_den)
    hi = x.numerator / x.denominator
    lo_q = x - Fraction(hi)
    lo = lo_q.numerator / lo_q.denominator
    return hi, lo


def backward_inputs(count: int, seed: int):
    """(hi, lo) float64 arrays: fractions +-1/2, ties of the final rounding, values just below 1 and just
    below an integer, tiny negatives, and `count` random double-doubles whose value the double-double
    pipeline holds exactly (dyadic rationals of at most 106 bits in (-4, 4), and tiny positive values)."""
    pairs = [(0.5, 0.0), (-0.5, 0.0), (0.5, -(2.0 ** -130)), (0.5, 2.0 ** -130), (0.0, 0.0), (1.0, 0.0), (-1.0, 0.0),
             (2.0 ** -129, 0.0), (3 * 2.0 ** -129, 0.0), (0.25, 2.0 ** -129), (0.25, -(2.0 ** -129)),
             (0.25, 3 * 2.0 ** -129), (1.0 - 2.0 ** -53, 0.0), (1.0 - 2.0 ** -53, 2.0 ** -54 - 2.0 ** -106),
             (1.0, -(2.0 ** -130)), (1.0, -(2.0 ** -128)), (3.0, -(2.0 ** -127)), (-(2.0 ** -100), 0.0),
             (-(2.0 ** -128), 0.0), (-(2.0 ** -129), 0.0), (-(2.0 ** -130), 0.0), (-(2.0 ** -140), 0.0),
             (2.0 ** -130, 0.0), (-3.75, 2.0 ** -60)]
    rng = np.random.default_rng(seed)
    for i in range(count):
        if i % 2 == 0:
            num = int(rng.integers(0, 1 << 62)) << 44 | int(rng.integers(0, 1 << 44))  # 106 bits
            num = num if rng.integers(0, 2) else -num
            pairs.append(_dd(num, 104))
        else:  # a tiny positive value: the final rounding decides
            e = int(rng.integers(100, 150))
            pairs.append(_dd(int(rng.integers(0, 1 << 53)) << 53 | int(rng.integers(0, 1 << 53)), e + 106))
    a = np.array(pairs, dtype=np.float64)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def mask_for_rotation(rot: int, N: int) -> int:
    """A u128 mask element whose modulus switch (common.rs:26-43) is `rot` (0 <= rot <= 2N)."""
    return (rot << (128 - int(math.log2(N)) - 1)) & R.MASK128


def cmux_bound(N: int, k: int, level: int, base_log: int) -> int:
    """(k+1) L 2^(128 - (100 - base_log - log2 N)): the reference's product bound (tests.rs:165-175) with
    the digit magnitude in place of 16, once per accumulated product."""
    return (k + 1) * level << (128 - (100 - base_log - int(math.log2(N))))


_cmux_cases = {}


def one_cmux_case(N: int, k: int, level: int, base_log: int, rotation: int):
    """n = 1, key bit 1, body 0, a uniform general accumulator: the blind rotation is one CMUX by X^rotation."""
    key = (N, k, level, base_log)
    if key not in _cmux_cases:
        glwe_sk = R.binary_key(31, k * N)
        bsk = R.gen_bsk(32 + N + k, np.ones(1, dtype=np.uint64), glwe_sk, k, N, base_log, level, GLWE_STD)
        acc = R.uniform(33 + N, (k + 1) * N)
        _cmux_cases[key] = (bsk, acc)
    bsk, acc = _cmux_cases[key]
    lwe = R.to_words([mask_for_rotation(rotation, N), 0]).reshape(1, 2, 2)
    return SimpleNamespace(params=params(1, N, k, level, base_log), bsk=bsk, acc=acc, lwe=lwe)


def parity_case(N: int, k: int, level: int, base_log: int, batch: int, n: int = 5):
    """Uniform key, two uniform general accumulators with lut_indexes, and inputs that hit the modulus
    switch's corners: mask element 1 zero, element 2 just below 2^128 (switches to 2N = rotation 0 by
    rounding), bodies switching to 0, N and 2N in the first three rows."""
    p = params(n, N, k, level, base_log)
    bsk = R.uniform(41 + N + 10 * k + level, n * level * (k + 1) * (k + 1) * N).reshape(n, level, k + 1, k + 1, N, 2)
    luts = R.uniform(42 + N + k, 2 * (k + 1) * N).reshape(2, (k + 1) * N, 2)
    lwe = R.uniform(43 + N + k + batch, batch * (n + 1)).reshape(batch, n + 1, 2)
    lwe[:, 1, :] = 0
    lwe[:, 2, :] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for row, rot in enumerate((0, N, 2 * N)):
        if row < batch:
            lwe[row, n] = R.to_words([mask_for_rotation(rot, N) - (1 if rot == 2 * N else 0)])[0]
    idx = (np.arange(batch) % 2).astype(np.uint32)
    return SimpleNamespace(params=p, bsk=bsk, luts=luts, lwe=lwe, idx=idx)
