"""GGSW external product, CMUX and vertical packing: the CPU reference (tests/ggsw_reference.py,
built from the oracle's blind rotation) checked against itself, against exact arithmetic and by
decryption; client.gen_ggsw_list; the core_crypto shape checks.  No GPU needed.

Shapes (N, k, base_log, level): (2048, 1, 5, 3) is the circuit-bootstrap decomposition of
WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS; (512, 3, 4, 6) has the deepest level loop of the GPU tests.
"""
import numpy as np
import pytest

from ggsw_reference import Ref, ggsw_words, index_bits, lut_value, torus_distance, vp_lut

U64 = np.uint64
GLWE_STD = 2.94036859086e-16  # 2^-51.6, the WoP 2_2 GLWE noise


def _keys(k, N, seed):
    from tfhe_mi355 import client

    return client.gen_binary_key(seed, 2, k * N)


def _ggsws(bits, sk, k, N, B, L, seed):
    from tfhe_mi355 import client

    return client.gen_ggsw_list(seed, bits, sk, k, N, B, L, GLWE_STD)


def test_gen_ggsw_list_layout():
    k, N, B, L = 1, 256, 5, 3
    sk = _keys(k, N, 3)
    g = _ggsws([1, 0, 1], sk, k, N, B, L, 4)
    assert g.shape == (3, L, k + 1, (k + 1) * N) and g.dtype == np.uint64
    assert g[0].size == ggsw_words(k, N, L)


def test_reference_constructions_agree(orc):
    """nr = 3 rotation steps as ONE oracle blind rotation == three single CMUXes, each the external-
    product construction applied to an explicitly rotated accumulator: word for word."""
    k, N, B, L = 1, 2048, 5, 3
    ref = Ref(orc, k, N, B, L)
    sk = _keys(k, N, 5)
    g = _ggsws([1, 0, 1], sk, k, N, B, L, 6)
    acc = np.random.default_rng(7).integers(0, 1 << 64, (k + 1) * N, dtype=U64)
    a = ref.rotation_phase(g, acc)
    b = ref.rotation_phase_by_cmuxes(g, acc)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, acc)


def test_vectorised_digits_match_the_oracle(orc):
    rng = np.random.default_rng(8)
    for B, L in ((5, 3), (4, 6), (16, 2), (32, 1), (14, 1)):
        ref = Ref(orc, 1, 256, B, L)
        x = np.concatenate([rng.integers(0, 1 << 64, 64, dtype=U64),
                            np.array([0, 1 << 63, (1 << 64) - 1, (1 << 63) - 1, 1 << (63 - B * L)], dtype=U64)])
        d = ref.digits(x)
        for i, v in enumerate(x):
            assert [int(t) for t in d[::-1, i]] == orc.decompose(int(v), B, L)


@pytest.mark.parametrize("N,k,B,L", [(2048, 1, 5, 3), (512, 3, 4, 6)])
def test_reference_external_product_within_fft_bound(orc, N, k, B, L):
    """The reference external product against the exact one (signed digits x standard-domain rows,
    exact negacyclic products).  Bound: the reference's FFT error bound 2^(64 - (52 - 16 - log2 N))."""
    ref = Ref(orc, k, N, B, L)
    sk = _keys(k, N, 9)
    g = _ggsws([1], sk, k, N, B, L, 10)[0]
    d = np.random.default_rng(11).integers(0, 1 << 64, (k + 1) * N, dtype=U64)
    got = ref.external_product(g, d)[0]
    exact = ref.external_product_exact(g, d)
    err = torus_distance(got, exact).max()
    bound = 2.0 ** (64 - (52 - 16 - (N.bit_length() - 1)))
    print(f"(N, k, B, L) = {(N, k, B, L)}: max |fft - exact| = 2^{np.log2(max(err, 1.0)):.1f}, bound 2^{np.log2(bound):.0f}")
    assert err < bound


def test_gen_ggsw_list_bit_selects_the_phase(orc):
    """GGSW(1) (x) ct keeps the phase of ct, GGSW(0) (x) ct annihilates it.

    Bound 2^56 at (2048, 1, 5, 3): the product is taken on ct rounded to base_log * level = 15 bits,
    an error uniform in +-2^48 per coefficient; through the phase it meets the body and at most kN key
    bits, so its standard deviation is at most 2^48 sqrt((kN + 1) / 3) = 2^52.7, and 2^56 is more than
    8 of those.  The encryption noise (digits <= 16, std 2^12.4, L (k+1) N terms: 2^23) and the FFT
    error (< 2^39) are far below."""
    k, N, B, L = 1, 2048, 5, 3
    ref = Ref(orc, k, N, B, L)
    sk = _keys(k, N, 12)
    g = _ggsws([1, 0], sk, k, N, B, L, 13)
    rng = np.random.default_rng(14)
    m = rng.integers(0, 1 << 64, N, dtype=U64)
    ct = rng.integers(0, 1 << 64, (k + 1) * N, dtype=U64)
    ct[k * N:] = 0
    ct[k * N:] = m - ref.phase(sk, ct)  # noiseless encryption of m under a random mask
    assert np.array_equal(ref.phase(sk, ct), m)
    kept = torus_distance(ref.phase(sk, ref.external_product(g[0], ct)[0]), m).max()
    gone = torus_distance(ref.phase(sk, ref.external_product(g[1], ct)[0]), np.zeros(N, dtype=U64)).max()
    print(f"bit 1: max phase error 2^{np.log2(kept):.1f}; bit 0: max phase 2^{np.log2(max(gone, 1.0)):.1f}")
    assert kept < 2.0 ** 56
    assert gone < 2.0 ** 56


def test_core_crypto_shape_checks_raise():
    from tfhe_mi355 import core_crypto as cc

    k, N, B, L = 1, 2048, 5, 3
    glwe = (k + 1) * N
    with pytest.raises(ValueError, match="multiple of one GGSW"):
        cc.GgswCiphertextList(np.zeros(ggsw_words(k, N, L) + 1, dtype=U64), k + 1, N, B, L)
    two = cc.GgswCiphertextList(np.zeros(2 * ggsw_words(k, N, L), dtype=U64), k + 1, N, B, L)
    assert len(two) == 2
    ok = np.zeros((2, glwe), dtype=U64)
    with pytest.raises(ValueError, match="GlweSize"):
        cc.add_external_product_assign(ok.copy(), two, np.zeros((2, glwe - N), dtype=U64), None)
    with pytest.raises(ValueError, match="GlweSize"):
        cc.add_external_product_assign(np.zeros((2, glwe + N), dtype=U64), two, ok, None)
    with pytest.raises(ValueError, match="GGSWs for"):
        cc.add_external_product_assign(np.zeros((3, glwe), dtype=U64), two, np.zeros((3, glwe), dtype=U64), None)
    with pytest.raises(ValueError, match="GlweSize"):
        cc.cmux_assign(ok.copy(), np.zeros((2, 2 * glwe), dtype=U64), two, None)
    with pytest.raises(ValueError, match="differ in shape"):
        cc.cmux_assign(ok.copy(), np.zeros((3, glwe), dtype=U64), two, None)
    with pytest.raises(ValueError, match="GGSWs for"):
        cc.cmux_assign(np.zeros((3, glwe), dtype=U64), np.zeros((3, glwe), dtype=U64), two, None)
    out = np.zeros(k * N + 1, dtype=U64)
    with pytest.raises(ValueError, match="power of two"):
        cc.vertical_packing(np.zeros((3, N), dtype=U64), out, two, None)
    with pytest.raises(ValueError, match="PolynomialSize"):
        cc.vertical_packing(np.zeros((2, N // 2), dtype=U64), out, two, None)
    with pytest.raises(ValueError, match="need 3 GGSWs"):
        cc.vertical_packing(np.zeros((8, N), dtype=U64), out, two, None)
    with pytest.raises(ValueError, match="LweDimension"):
        cc.vertical_packing(np.zeros((2, N), dtype=U64), np.zeros(k * N, dtype=U64), two, None)
    small = cc.GgswCiphertextList(np.zeros(9 * ggsw_words(1, 256, 1), dtype=U64), 2, 256, 14, 1)
    with pytest.raises(ValueError, match="rotation bits"):
        cc.vertical_packing(np.zeros((1, 256), dtype=U64), np.zeros(257, dtype=U64), small, None)


def test_reference_vertical_packing_decrypts(orc):
    """2 tree bits + 3 rotation bits, a 4-bit LUT at delta = 2^60: every index decrypts to LUT[index]
    (error against delta / 2 = 2^59 printed)."""
    k, N, B, L = 1, 2048, 5, 3
    nt, nr, delta = 2, 3, 1 << 60
    ref = Ref(orc, k, N, B, L)
    sk = _keys(k, N, 15)
    lut = vp_lut(1 << nt, N, nr, delta)
    worst = 0.0
    for n, index in enumerate((0, 5, 13, 22, 31)):
        g = _ggsws(index_bits(index, nt + nr), sk, k, N, B, L, 16 + n)
        out = ref.vertical_packing(g, lut)
        pt = orc.lwe_decrypt(sk, out[None])[0]
        want = lut_value(index)
        worst = max(worst, torus_distance(pt, U64(want * delta)).max())
        assert int((int(pt) + (delta >> 1)) >> 60) % 16 == want, (index, hex(int(pt)))
    print(f"max decryption error 2^{np.log2(worst):.1f} against delta / 2 = 2^59")
    assert worst < 2.0 ** 59
