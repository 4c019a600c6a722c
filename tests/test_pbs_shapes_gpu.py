"""GPU parity tests of every PBS shape and decomposition width the context accepts (capi.cpp
validate_parameters), most of which no named parameter set reaches: the 26 classic kernels
(pbs_classic.hip), (2048,1,1) in its latency and throughput forms, the 12 large (N, L) pairs
(pbs_large.hip) with the three CMUX forms at N = 4096 / 8192, multi-bit at its widest bases, and the
edges of the accepted envelope.

Bar: bit-exact u64 equality with the oracle.  Inputs are random words (any u64 is a valid ciphertext
word) with edge masks and bodies, plus the crafted case of tests/pbs_edge_inputs.py, whose first
CMUX decomposes chosen worst-case words: ties and carries, the +2^(B-1) digit, the rounding overflow.
LWE dimensions are 1 ... 6: a kernel does not depend on n beyond its CMUX count.
"""
import numpy as np
import pytest

from conftest import KeySet
from pbs_edge_inputs import crafted_case, pbs_edge_words, unit_mask

pytestmark = pytest.mark.gpu
U64 = np.uint64
ONES = U64((1 << 64) - 1)

# PBS_CLASSIC_SHAPES (csrc/pbs_classic.hip), every (N, k, L) instantiated there
CLASSIC_SHAPES = [(2048, 1, 1), (2048, 1, 2),
                  (1024, 1, 1), (1024, 1, 2), (1024, 1, 3), (1024, 1, 4),
                  (1024, 2, 1), (1024, 2, 2), (1024, 2, 3), (1024, 2, 4),
                  (1024, 3, 1), (1024, 3, 2), (1024, 3, 3),
                  (512, 1, 1), (512, 1, 2), (512, 1, 3), (512, 1, 4),
                  (512, 2, 1), (512, 2, 2), (512, 2, 3), (512, 2, 4),
                  (512, 3, 1), (512, 3, 2), (512, 3, 3), (512, 3, 4),
                  (256, 5, 1)]


def test_classic_shape_list_is_the_macro():
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tfhe-rs-odd_amd", "csrc",
                       "pbs_classic.hip")
    with open(src) as f:
        macro = re.search(r"#define PBS_CLASSIC_SHAPES\(X\)((?:.*\\\n)*.*)\n", f.read()).group(1)
    shapes = [tuple(map(int, m)) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", macro)]
    assert len(shapes) == 26 and shapes == CLASSIC_SHAPES


def _params(N, k, L, B, n, g=0):
    from tfhe_mi355.parameters import ClassicPBSParameters

    return ClassicPBSParameters(lwe_dimension=n, glwe_dimension=k, polynomial_size=N,
                                lwe_modular_std_dev=2.0 ** -20, glwe_modular_std_dev=2.0 ** -50,
                                pbs_base_log=B, pbs_level=L, ks_base_log=3, ks_level=5, message_modulus=4,
                                carry_modulus=4, grouping_factor=g, name=f"N{N}_k{k}_L{L}_B{B}_n{n}_g{g}")


def _engine(p, bsk):
    from tfhe_mi355 import Engine

    e = Engine(p, 0)
    e.upload_bootstrap_key(bsk)
    return e


def _large_keys(orc, p, seed):
    """the engine's client-side keygen (exact FFT products; the oracle's schoolbook keygen is too slow
    at the larger N), fed to both sides as standard u64 keys."""
    from tfhe_mi355 import client

    lwe_sk = client.gen_binary_key(seed, 1, p.lwe_dimension)
    glwe_sk = client.gen_binary_key(seed, 2, p.big_lwe_dimension)
    if p.grouping_factor:
        bsk = client.gen_multi_bit_bootstrap_key(seed + 1, lwe_sk, glwe_sk, 1, p.polynomial_size, p.pbs_base_log,
                                                 p.pbs_level, p.grouping_factor, p.glwe_modular_std_dev, threads=8)
        return bsk, orc.MultiBitFourierBsk(bsk, p.lwe_dimension, 1, p.polynomial_size, p.pbs_base_log, p.pbs_level,
                                           p.grouping_factor)
    bsk = client.gen_bootstrap_key(seed + 1, lwe_sk, glwe_sk, 1, p.polynomial_size, p.pbs_base_log, p.pbs_level,
                                   p.glwe_modular_std_dev)
    return bsk, orc.FourierBsk(bsk, p.lwe_dimension, 1, p.polynomial_size, p.pbs_base_log, p.pbs_level)


def _cus():
    """Compute units of device 0: the CMUX form thresholds of capi_pbs.cpp scale with it."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _ran(eng, f):
    """f()'s result and the kernel families it launched (the engine's kernel timer)."""
    eng.kernel_timing(1)
    out = f()
    ran = set(eng.kernel_times())
    eng.kernel_timing(0)
    return out, ran


def _same(got, exp, what):
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    assert bad.size == 0, f"{what}: rows {bad[:20]} differ ({np.count_nonzero(got != exp)} words)"


def _crafted_rows(cts, first, N):
    """rows first .. first + 2 become the crafted triple: a~_0 = 1 and b = 0, b~ = N, b~ = 2N (the other
    mask words stay as they are: later CMUXes decompose data-dependent words)."""
    cts[first:first + 3, 0] = unit_mask(N)
    cts[first:first + 3, -1] = [0, 1 << 63, (1 << 64) - 1]


# ---- 1. every classic shape ---------------------------------------------------------------------

def _widths(L):
    return [30 // L, 2]  # the widest base the context accepts and a narrow one


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
@pytest.mark.parametrize("shape", CLASSIC_SHAPES, ids=lambda s: "N%d_k%d_L%d" % s)
def test_classic_shape_bit_exact(orc, shape, wide):
    """19 random ciphertexts at n = 5 (row 0: every a~ = 0; row 1: b~ = 2N), two random LUTs taken in
    turn, one count-1 call, PBS and blind rotation."""
    N, k, L = shape
    B = _widths(L)[0 if wide else 1]
    p = _params(N, k, L, B, 5)
    keys = KeySet(orc, p, seed=7)
    eng = _engine(p, keys.bsk)
    try:
        rng = np.random.default_rng(1000 * N + 10 * k + L + B)
        cts = rng.integers(0, 2 ** 64, (19, 6), dtype=U64)
        cts[0, :-1] = 0
        cts[1, -1] = ONES
        luts = rng.integers(0, 2 ** 64, (2, (k + 1) * N), dtype=U64)
        idx = (np.arange(19) % 2).astype(np.uint32)
        exp = keys.fbsk.pbs(cts, luts, idx, threads=8)
        _same(eng.programmable_bootstrap(cts, luts, idx), exp, "pbs")
        _same(eng.programmable_bootstrap(cts[7:8], luts, idx[7:8]), exp[7:8], "pbs of one")
        _same(eng.blind_rotate(cts, luts, idx), keys.fbsk.blind_rotate(cts, luts, idx, threads=8), "blind rotation")
    finally:
        eng.close()


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
@pytest.mark.parametrize("shape", CLASSIC_SHAPES, ids=lambda s: "N%d_k%d_L%d" % s)
def test_classic_shape_crafted_digits(orc, shape, wide):
    """n = 1, a~ = 1, the crafted LUT: the one CMUX decomposes the edge words of (B, L) (b = 0 and
    b~ = 2N) and their negation (b~ = N), one polynomial of them per GLWE row."""
    N, k, L = shape
    B = _widths(L)[0 if wide else 1]
    p1 = _params(N, k, L, B, 1)
    keys = KeySet(orc, p1, seed=9)
    eng = _engine(p1, keys.bsk)
    try:
        cts, lut, _ = crafted_case(B, L, N, k, seed=N + k + L)
        _same(eng.programmable_bootstrap(cts, lut), keys.fbsk.pbs(cts, lut, threads=3), "crafted pbs")
        _same(eng.blind_rotate(cts, lut), keys.fbsk.blind_rotate(cts, lut, threads=3), "crafted blind rotation")
    finally:
        eng.close()


@pytest.mark.parametrize("shape", [(128, 1, 1), (128, 3, 2), (1024, 3, 4), (2048, 2, 1)], ids=str)
def test_shape_outside_the_classic_list_is_refused(shape):
    from tfhe_mi355 import Engine
    from tfhe_mi355._lib import EngineError

    N, k, L = shape
    with pytest.raises(EngineError, match="no kernel"):
        Engine(_params(N, k, L, 4, 5), 0)


# ---- 2. (2048, 1, 1): latency and throughput kernels ----------------------------------------------

@pytest.mark.parametrize("B", [2, 30])
def test_2048_latency_and_throughput_kernels(orc, B):
    """n = 2.  One call of 200 rows (pbs_latency_kernel) and one of 1100 (pbs_classic_kernel): rows
    0 .. 2 are the crafted triple under the crafted LUT, the others random under either LUT; the rows in
    common identical, 16 sampled rows equal to the oracle."""
    N, k, L, small, big = 2048, 1, 1, 200, 1100
    p = _params(N, k, L, B, 2)
    keys = KeySet(orc, p, seed=13)
    eng = _engine(p, keys.bsk)
    try:
        rng = np.random.default_rng(B)
        cts = rng.integers(0, 2 ** 64, (big, 3), dtype=U64)
        _crafted_rows(cts, 0, N)
        cts[3, :-1] = 0
        cts[4, -1] = ONES
        luts = np.stack([crafted_case(B, L, N, k, seed=B)[1], rng.integers(0, 2 ** 64, (k + 1) * N, dtype=U64)])
        idx = (np.arange(big) % 2).astype(np.uint32)
        idx[:3] = 0
        thr, ran = _ran(eng, lambda: eng.programmable_bootstrap(cts, luts, idx))
        assert "pbs_classic_kernel" in ran, ran
        lat, ran = _ran(eng, lambda: eng.programmable_bootstrap(cts[:small], luts, idx[:small]))
        assert ran == {"pbs_latency_kernel"}, ran
        _same(lat, thr[:small], "latency against throughput kernel")
        sample = np.r_[0:8, 100, 199, 200, 201, 600, 1023, 1024, 1099]
        assert sample.size == 16
        _same(thr[sample], keys.fbsk.pbs(cts[sample], luts, idx[sample], threads=16), "oracle sample")
    finally:
        eng.close()


# ---- 3. large shapes and widths ------------------------------------------------------------------

LARGE = [(4096, 3, 11), (8192, 3, 11), (4096, 3, 15), (16384, 3, 15), (32768, 3, 15),
         (16384, 1, 22), (32768, 1, 22), (16384, 1, 30),
         (4096, 2, 2), (8192, 2, 8), (16384, 2, 2), (32768, 2, 8), (16384, 2, 15)]


@pytest.mark.parametrize("case", LARGE, ids=lambda c: "N%d_L%d_B%d" % c)
def test_large_shape_bit_exact(orc, case):
    """n = 3: six random ciphertexts with the edge masks of test_split_pbs_bit_exact_vs_oracle (every
    a~ = 0, a~ = N, b~ = 2N, alternating all-ones words), two random LUTs, one count-1 call."""
    N, L, B = case
    p = _params(N, 1, L, B, 3)
    bsk, fbsk = _large_keys(orc, p, 51)
    eng = _engine(p, bsk)
    try:
        rng = np.random.default_rng(N + 100 * L + B)
        cts = rng.integers(0, 2 ** 64, (6, 4), dtype=U64)
        cts[0, :-1] = 0
        cts[1, :-1] = U64(1 << 63)
        cts[2, -1] = ONES
        cts[3, ::2] = ONES
        luts = rng.integers(0, 2 ** 64, (2, 2 * N), dtype=U64)
        idx = np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32)
        _same(eng.programmable_bootstrap(cts, luts, idx), fbsk.pbs(cts, luts, lut_idx=idx, threads=6), "pbs")
        _same(eng.programmable_bootstrap(cts[4:5], luts[1]), fbsk.pbs(cts[4:5], luts[1], threads=1), "pbs of one")
    finally:
        eng.close()


@pytest.mark.parametrize("case", LARGE, ids=lambda c: "N%d_L%d_B%d" % c)
def test_large_shape_crafted_digits(orc, case):
    """n = 1, a~ = 1, the crafted LUT: the one CMUX decomposes the edge words of (B, L) and their negation."""
    N, L, B = case
    p1 = _params(N, 1, L, B, 1)
    bsk, fbsk = _large_keys(orc, p1, 53)
    eng = _engine(p1, bsk)
    try:
        cts, lut, _ = crafted_case(B, L, N, 1, seed=N + L)
        _same(eng.programmable_bootstrap(cts, lut), fbsk.pbs(cts, lut, threads=3), "crafted pbs")
    finally:
        eng.close()


@pytest.mark.parametrize("B", [30, 31])
@pytest.mark.parametrize("N", [4096, 8192])
def test_one_level_three_cmux_forms(orc, N, B):
    """N = 4096 / 8192, L = 1 at base 2^30 (the last 32-bit digit) and 2^31 (the 64-bit one-level arm:
    quad_cmux_kernel / onchip_cmux_kernel <N, false, 1> and decompose64<1> in the top stage): the same
    rows through the on-chip CMUX (one call above capi_pbs.cpp onchip_min), the quad / duo CMUX (calls of
    1, 7 and CUs/R - 12 rows, at most quad_max) and the split CMUX (the rest, between the two), each
    kernel checked by the engine's kernel timer; every row identical, 9 sampled rows equal to the
    oracle, the crafted triple (rows 0 .. 2, crafted LUT) among them."""
    L, n = 1, 3
    p = _params(N, 1, L, B, n)
    bsk, fbsk = _large_keys(orc, p, 79)
    eng = _engine(p, bsk)
    try:
        cus = _cus()
        R = N // 2048
        Q, O = cus // R, cus * (5 if R == 2 else 3) // 8  # capi_pbs.cpp quad_max, onchip_min
        C = max(O + 35, Q - 4 + (Q + O) // 2)  # the last call (Q - 4 .. C) lands between Q and O
        rng = np.random.default_rng(N + B)
        cts = rng.integers(0, 2 ** 64, (C, n + 1), dtype=U64)
        _crafted_rows(cts, 0, N)
        cts[3, :-1] = 0
        cts[4, :-1] = U64(1 << 63)
        cts[5, -1] = ONES
        cts[6, ::2] = ONES
        luts = np.stack([crafted_case(B, L, N, 1, seed=N + B)[1], rng.integers(0, 2 ** 64, 2 * N, dtype=U64)])
        idx = (np.arange(C) % 3 == 2).astype(np.uint32)
        idx[:3] = 0
        whole, ran = _ran(eng, lambda: eng.programmable_bootstrap(cts, luts, lut_indexes=idx))
        assert "onchip_cmux_kernel" in ran, ran
        parts = []
        for a, b, kern in ((0, 1, "quad_cmux_kernel"), (1, 8, "quad_cmux_kernel"), (8, Q - 4, "quad_cmux_kernel"),
                           (Q - 4, C, "large_sub_kernel")):
            assert 0 < b - a <= Q if kern.startswith("quad") else Q < b - a < O
            out, ran = _ran(eng, lambda: eng.programmable_bootstrap(cts[a:b], luts, lut_indexes=idx[a:b]))
            assert kern in ran and "onchip_cmux_kernel" not in ran, (a, b, ran)
            parts.append(out)
        _same(np.concatenate(parts), whole, "quad and split against on-chip CMUX")
        sample = np.array([0, 1, 2, 3, 7, 8, Q - 5, Q - 4, C - 1])
        _same(whole[sample], fbsk.pbs(cts[sample], luts, lut_idx=idx[sample], threads=9), "oracle sample")
    finally:
        eng.close()


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("shape", [(2048, 1, 30), (8192, 2, 15)], ids=lambda s: "N%d_L%d_B%d" % s)
def test_multi_bit_widest_base(orc, shape, g):
    """Multi-bit at B L = 30, n = 6.  Its external products take the accumulator itself, so the edge
    words are the LUT: rows 0 .. 2 (b = 0, b~ = N, b~ = 2N) decompose them, their negation and them
    again in the first group.  N = 2048: 19 rows (pbs_mb_latency_kernel) inside 600 (pbs_multibit);
    N = 8192: 6 rows (spectra between the launches) inside 130 (packed digits, MB_DIGITS_MIN = 128).
    The rows in common identical, a sample equal to the oracle."""
    N, L, B = shape
    n = 6
    p = _params(N, 1, L, B, n, g)
    bsk, fb = _large_keys(orc, p, 101)
    eng = _engine(p, bsk)
    try:
        few, many = (19, 600) if N == 2048 else (6, 130)
        rng = np.random.default_rng(N + g)
        cts = rng.integers(0, 2 ** 64, (many, n + 1), dtype=U64)
        cts[:3, -1] = [0, 1 << 63, (1 << 64) - 1]
        cts[3, :-1] = 0
        cts[4, :-1] = U64(1 << 63)
        cts[5, ::2] = ONES
        edge = np.concatenate([pbs_edge_words(B, L, N, seed=g), pbs_edge_words(B, L, N, seed=g + 1)])
        luts = np.stack([edge, rng.integers(0, 2 ** 64, 2 * N, dtype=U64)])
        idx = (np.arange(many) % 2).astype(np.uint32)
        idx[:3] = 0
        big, ran_big = _ran(eng, lambda: eng.programmable_bootstrap(cts, luts, lut_indexes=idx))
        small, ran_small = _ran(eng, lambda: eng.programmable_bootstrap(cts[:few], luts, lut_indexes=idx[:few]))
        if N == 2048:
            assert "pbs_multibit" in ran_big and ran_small == {"pbs_mb_latency_kernel"}, (ran_big, ran_small)
        else:
            assert "mb_digits_init_kernel" in ran_big and "mb_digits_init_kernel" not in ran_small, (ran_big, ran_small)
            assert "large_mb_pair2_kernel" in ran_big and "large_mb_pair2_kernel" in ran_small, (ran_big, ran_small)
        _same(small, big[:few], "small against large call")
        _same(eng.programmable_bootstrap(cts[1:2], luts[0]), big[1:2], "pbs of one")
        sample = np.r_[0:6, few - 1, few, many - 1]
        _same(big[sample], fb.pbs(cts[sample], luts, lut_idx=idx[sample], threads=9), "oracle sample")
    finally:
        eng.close()


# ---- 4. the edge of what is accepted -------------------------------------------------------------

@pytest.mark.parametrize("N,k,L,B,g,msg", [
    (4096, 1, 1, 32, 0, "base_log 32 > 31"),     # decompose64 returns int32 digits: +2^31 would wrap
    (8192, 1, 1, 32, 0, "base_log 32 > 31"),
    (16384, 1, 1, 63, 0, "base_log 63 > 31"),
    (32768, 1, 1, 40, 0, "base_log 40 > 31"),
    (2048, 1, 1, 31, 0, "base_log\\*level"),     # N <= 2048 and multi-bit decompose in 32-bit registers
    (512, 3, 4, 8, 0, "base_log\\*level"),
    (1024, 1, 2, 16, 0, "base_log\\*level"),
    (2048, 1, 1, 31, 3, "base_log\\*level"),
    (8192, 1, 2, 16, 2, "base_log\\*level"),
    (4096, 1, 2, 16, 0, "base_log 16 > 15"),     # int16 digits between the passes of the split CMUX
    (16384, 1, 3, 16, 0, "base_log 16 > 15"),
    (32768, 1, 2, 16, 0, "base_log 16 > 15"),
    (2048, 1, 1, 1, 0, "base_log\\*level"),      # base_log 1: no digit (0 as well)
    (4096, 1, 3, 1, 0, "base_log\\*level"),
    (8192, 1, 2, 0, 0, "base_log\\*level"),
])
def test_decomposition_outside_the_envelope_is_refused(N, k, L, B, g, msg):
    from tfhe_mi355 import Engine
    from tfhe_mi355._lib import EngineError

    with pytest.raises(EngineError, match=msg):
        Engine(_params(N, k, L, B, 6, g), 0)


@pytest.mark.parametrize("N,k,L,B,g", [(16384, 1, 1, 31, 0), (32768, 1, 1, 31, 0), (2048, 1, 1, 30, 0),
                                       (512, 3, 4, 7, 0), (4096, 1, 3, 15, 0), (2048, 1, 1, 30, 2),
                                       (1024, 2, 3, 2, 0)])
def test_decomposition_on_the_envelope_is_accepted(N, k, L, B, g):
    """(base 2^31 at N = 4096 / 8192 runs bit-exact in test_one_level_three_cmux_forms.)"""
    from tfhe_mi355 import Engine

    Engine(_params(N, k, L, B, 6, g), 0).close()
