"""CPU checks of tests/pbs_edge_inputs.py (the chosen decomposer inputs of test_pbs_shapes_gpu.py) and of
the one-level 64-bit decomposer's digit width (csrc/pbs_large.hip decompose64)."""
import numpy as np
import pytest

from ggsw_reference import Ref, torus_distance
from pbs_edge_inputs import (crafted_case, crafted_lut, edge_families, edge_positions, negacyclic_mul_x,
                             pbs_edge_words, unit_mask)

U64 = np.uint64
# every (base_log, level) test_pbs_shapes_gpu.py runs: the classic shapes' widest and narrowest bases,
# the large shapes' list, the one-level 31 of the 64-bit decomposer
DECOMPOSITIONS = [(30, 1), (15, 2), (10, 3), (7, 4), (2, 1), (2, 2), (2, 3), (2, 4),
                  (11, 3), (15, 3), (22, 1), (8, 2), (31, 1)]


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096, 8192, 16384, 32768])
def test_crafted_lut_identity(N, k):
    """X acc - acc = D for random D, with an independent rotation (np.roll and a sign flip); odd sums are
    mended in the lowest bit of one word per polynomial, at a free position only."""
    rng = np.random.default_rng(N + k)
    D = rng.integers(0, 1 << 64, (k + 1, N), dtype=U64)
    D[0, 5] ^= U64(int(np.sum(D[0], dtype=U64)) & 1 ^ 1)   # row 0 odd, row 1 even
    D[1, 5] ^= U64(int(np.sum(D[1], dtype=U64)) & 1)
    free = ~edge_positions(N)
    acc, D2 = crafted_lut(D, free=free, seed=3)
    rot = np.roll(acc, 1, axis=1)
    rot[:, 0] = U64(0) - rot[:, 0]
    assert np.array_equal(rot - acc, D2)
    assert np.array_equal(negacyclic_mul_x(acc), rot)
    diff = D ^ D2
    assert diff[0].sum() == 1 and diff[1].sum() == 0 and (diff.sum(axis=1) <= 1).all()
    assert not diff[:, ~free].any()
    assert not (np.sum(D2, axis=1, dtype=U64) & U64(1)).any()


@pytest.mark.parametrize("N", [256, 2048, 32768])
def test_unit_mask_switches_to_one(orc, N):
    log2n = N.bit_length() - 1
    assert orc.pbs_modulus_switch(int(unit_mask(N)), log2n) == 1
    assert orc.pbs_modulus_switch(0, log2n) == 0
    assert orc.pbs_modulus_switch(1 << 63, log2n) == N
    assert orc.pbs_modulus_switch((1 << 64) - 1, log2n) % (2 * N) == 0


@pytest.mark.parametrize("dec", DECOMPOSITIONS, ids=str)
def test_edge_words_extreme_digits(orc, dec):
    """The closed-form digits of every family (asserted inside pbs_edge_words against Ref.digits) equal
    the oracle's scalar decomposer, one level included; every family is present many times."""
    B, L = dec
    half = 1 << (B - 1)
    fam = edge_families(B, L)
    assert len(fam) == L + 7
    for name, w, exp in fam:
        got = [int(v) for v in np.array(orc.decompose(w, B, L), dtype=U64).astype(np.int64)]
        assert got == exp[::-1], (name, hex(w), B, L)  # the oracle yields level L first
    by = {name: exp for name, _, exp in fam}
    assert by["single_1"][0] == half and by["round_up"][-1] == half and by["heavy_pos"] == [half - 1] * L
    assert by["heavy_neg"][-1] == (half if L == 1 else -half)
    x = pbs_edge_words(B, L, 256, seed=4)
    words = np.array([w for _, w, _ in fam], dtype=U64)
    assert all(np.count_nonzero(x[::2] == w) >= 128 // len(fam) for w in words)
    d = Ref(None, 0, 0, B, L).digits(x).astype(np.int64)
    assert d.max() == half and (d.min() == -half if L > 1 else d.min() > -half)
    # random words too
    for w in x[1:12:2]:
        got = [int(v) for v in np.array(orc.decompose(int(w), B, L), dtype=U64).astype(np.int64)]
        assert got == [int(v) for v in Ref(None, 0, 0, B, L).digits(np.array([w])).astype(np.int64)[::-1, 0]]


@pytest.mark.parametrize("dec", [(30, 1), (15, 2), (2, 4), (31, 1)], ids=str)
def test_crafted_case_first_cmux_decomposes_D(orc, dec):
    """The oracle's blind rotation of the n = 1 crafted case under a one-GGSW key (random words) is
    acc + G (x) D' for the b = 0 row and -acc + G (x) -D' for b~ = N, with G (x) d computed from the
    digits of d itself by exact negacyclic products (Ref.external_product_exact).  The oracle's
    product goes through the f64 FFT: digits below 2^30 times 64-bit words over (k+1) L = 2 .. 8
    polynomials of 256 coefficients sum to under 2^106, so its rounding error stays near 2^53 -- while
    one digit off by one anywhere moves every output coefficient by a random key word, 2^62 on
    average.  2^57 separates the two.  (Ref.external_product, which rebuilds d as -2 ((0 - d) >> 1),
    cannot serve: it adds one to every odd word, which carries round_down over the boundary.)"""
    B, L = dec
    k, N = 1, 256
    cts, lut, D = crafted_case(B, L, N, k, seed=6)
    rng = np.random.default_rng(8)
    ggsw = rng.integers(0, 1 << 64, L * (k + 1) * (k + 1) * N, dtype=U64)
    f = orc.FourierBsk(ggsw, 1, k, N, B, L)
    got = f.blind_rotate(cts, lut.reshape(1, -1))
    ref = Ref(orc, k, N, B, L)
    assert torus_distance(got[0] - lut, ref.external_product_exact(ggsw, D)).max() < 2.0 ** 57
    assert torus_distance(got[1] + lut, ref.external_product_exact(ggsw, U64(0) - D)).max() < 2.0 ** 57
    assert np.array_equal(got[2], got[0])
    # the bound does tell a single digit apart: round_down + 1 rounds up
    D1 = D.copy()
    D1[0, np.nonzero(D[0] == U64(dict((n, w) for n, w, _ in edge_families(B, L))["round_down"]))[0][0]] += U64(1)
    assert torus_distance(got[0] - lut, ref.external_product_exact(ggsw, D1)).max() > 2.0 ** 60


def _decompose64_one_level(x, beta):
    """csrc/pbs_large.hip decompose64<1>, its int32_t digit included, widened back to int64."""
    x = np.asarray(x, dtype=U64)
    st = ((x >> U64(64 - beta - 1)) + U64(1)) >> U64(1)
    res = st & U64((1 << beta) - 1)
    st = st >> U64(beta)
    carry = (((res - U64(1)) | st) & res) >> U64(beta - 1)
    return (res - (carry << U64(beta))).astype(np.uint32).astype(np.int32).astype(np.int64)


def test_one_level_digit_fits_int32_up_to_base_log_31_only():
    """decompose64 returns int32_t digits.  A one-level digit lies in (-2^(beta-1), 2^(beta-1)]: it fits
    for beta <= 31, wraps at +2^31 for beta = 32 and loses its high bits beyond -- why context creation
    refuses pbs_base_log > 31 with one level at N >= 4096 (capi.cpp validate_parameters)."""
    for beta in (22, 30, 31):
        x = pbs_edge_words(beta, 1, 4096, seed=beta)
        exp = Ref(None, 0, 0, beta, 1).digits(x).astype(np.int64)[0]
        assert exp.max() == 1 << (beta - 1)
        assert np.array_equal(_decompose64_one_level(x, beta), exp)
    for beta in (32, 33, 40, 63):
        x = pbs_edge_words(beta, 1, 4096, seed=beta)
        exp = Ref(None, 0, 0, beta, 1).digits(x).astype(np.int64)[0]
        got = _decompose64_one_level(x, beta)
        bad = got != exp
        assert bad.any()
        if beta == 32:  # only the digit +2^31 is lost: it comes out as -2^31
            assert (exp[bad] == 1 << 31).all() and (got[bad] == -(1 << 31)).all()
