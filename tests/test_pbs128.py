"""128-bit-torus PBS on the CPU: the restatement of DESIGN.md 3b (tests/pbs_ref128.c) against exact
arithmetic and the reference's own tolerances (fft128/math/fft/tests.rs:46-56, 165-175), and the
core_crypto mirrors driven by the reference engine.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pbs128_cases as C  # noqa: E402
import pbs128_reference as R  # noqa: E402
from tfhe_mi355 import core_crypto as cc  # noqa: E402
from tfhe_mi355.parameters import ClassicPBSParameters  # noqa: E402

SIZES = [256, 512, 1024, 2048]


def _max_distance(a, b) -> int:
    return max(R.mod_distance(x, y) for x, y in zip(R.to_ints(a), R.to_ints(b)))


def test_tables_against_mpmath():
    import mpmath  # a dependency of torch: the cross-check the tables' own big-integer code does not share

    mpmath.mp.prec = 400
    for N in SIZES:
        tw, w = R.tables(N)
        for j in [0, 1, 2, N // 8, N // 4 - 1, N // 4, N // 4 + 1, N // 2 - 1]:
            for plane, x in ((0, mpmath.cos(mpmath.pi * j / N)), (2, mpmath.sin(mpmath.pi * j / N))):
                hi, lo = float(tw[plane, j]), float(tw[plane + 1, j])
                assert hi == float(x), (N, j)  # mpf -> float rounds to nearest
                assert lo == float(x - mpmath.mpf(hi)), (N, j)
        for t in [0, 1, N // 16, N // 8 - 1, N // 8 + 1, N // 4 - 1]:
            z = mpmath.expj(-2 * mpmath.pi * t / (N // 2))
            assert w[0, t] == float(z.real) and w[2, t] == float(z.imag), (N, t)
            assert w[1, t] == float(z.real - mpmath.mpf(float(w[0, t]))), (N, t)
            assert w[3, t] == float(z.imag - mpmath.mpf(float(w[2, t]))), (N, t)


@pytest.mark.parametrize("N", SIZES)
def test_roundtrip(N):
    poly = R.uniform(100 + N, N)
    d = _max_distance(poly, R.roundtrip(poly))
    print(f"N={N}: round trip distance 2^{math.log2(max(d, 1)):.2f}")
    assert d < 1 << 28  # fft128/math/fft/tests.rs:46-56


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("bits", [16, 23])
def test_product_against_exact(N, bits):
    rng = np.random.default_rng(N + bits)
    bound = 1 << (128 - (100 - bits - int(math.log2(N))))  # tests.rs:165-175 with `bits` for the magnitude
    worst = 0
    for draw in range(10):
        torus = R.uniform(1000 * bits + 10 * N + draw, N)
        integer = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), N)
        worst = max(worst, _max_distance(R.exact_product(torus, integer), R.fft_product(torus, integer)))
    print(f"N={N} bits={bits}: product error 2^{math.log2(max(worst, 1)):.2f}, bound 2^{math.log2(bound):.0f}")
    assert worst <= bound


def test_forward_conversion():
    words = C.forward_edge_words() + R.to_ints(R.uniform(7, 10000))
    hi, lo = R.to_signed_dd(R.to_words(words))
    for x, h, l in zip(words, hi.tolist(), lo.tolist()):
        eh, el = R.exact_signed_dd(x)
        assert (h, l) == (eh, el), hex(x)


def test_backward_conversion():
    hi, lo = C.backward_inputs(10000, seed=11)
    acc = R.uniform(12, len(hi))
    got = R.to_ints(R.torus_from_f128(hi, lo, acc))
    for h, l, a, g in zip(hi.tolist(), lo.tolist(), R.to_ints(acc), got):
        assert g == (a + R.exact_torus_from_dd(h, l)) & R.MASK128, (h, l)


@pytest.mark.parametrize("base_log,level", [(7, 1), (7, 3), (23, 1), (23, 3)])
def test_decomposer(base_log, level):
    edge = [0, 1, (1 << 128) - 1, 1 << 127, (1 << 127) - 1, 1 << (127 - base_log * level),
            (1 << (127 - base_log * level)) - 1, ((1 << 128) - 1) ^ ((1 << (128 - base_log * level)) - 1)]
    words = edge + R.to_ints(R.uniform(base_log * 10 + level, 2000))
    digits, closest = R.decompose(R.to_words(words), base_log, level)
    half = 1 << (base_log - 1)
    assert digits.min() >= -half and digits.max() <= half
    for i, x in enumerate(words):
        want = R.closest_representable(x, base_log, level)
        assert R.to_ints(closest[i:i + 1])[0] == want
        # digits[0] is level L (the least significant), digits[level-1] level 1
        rec = sum(int(digits[level - l, i]) << (128 - base_log * l) for l in range(1, level + 1))
        assert rec & R.MASK128 == want, hex(x)


@pytest.mark.parametrize("N,k,level,base_log", [(256, 2, 2, 7), (2048, 1, 1, 23)])
def test_one_cmux_against_exact(N, k, level, base_log):
    case = C.one_cmux_case(N, k, level, base_log, rotation=1)
    eng = R.RefEngine128(case.params)
    eng.upload_bootstrap_key_u128(case.bsk)
    got = eng.blind_rotate_u128(case.lwe, case.acc)[0]
    want = R.exact_cmux(case.acc, case.bsk[0], 1, N, k, base_log, level)
    d = _max_distance(got, want)
    bound = C.cmux_bound(N, k, level, base_log)
    print(f"({N},{k},{level},{base_log}): CMUX distance 2^{math.log2(max(d, 1)):.2f}, bound 2^{math.log2(bound):.1f}")
    assert d <= bound
    assert not np.array_equal(want, R._u64(case.acc).reshape(-1, 2))  # the CMUX did something


def _small_pbs(bits, modulus_log):
    p = ClassicPBSParameters(lwe_dimension=16, glwe_dimension=1, polynomial_size=256, lwe_modular_std_dev=2.0 ** -70,
                             glwe_modular_std_dev=8.6457178e-32, pbs_base_log=23, pbs_level=1, ks_base_log=3,
                             ks_level=5, message_modulus=1 << bits, carry_modulus=1, name="small_u128")
    lwe_sk, glwe_sk = R.binary_key(21, p.lwe_dimension), R.binary_key(22, p.polynomial_size)
    bsk = R.gen_bsk(23, lwe_sk, glwe_sk, 1, p.polynomial_size, p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev)
    fbsk = cc.convert_standard_lwe_bootstrap_key_to_fourier_128(bsk, p, engine=R.RefEngine128(p))
    delta = 1 << (modulus_log - bits - 1)
    msgs = list(range(1 << bits))
    cts = R.lwe_encrypt(24, lwe_sk, R.to_words([m * delta << (128 - modulus_log) for m in msgs]),
                        p.lwe_modular_std_dev)
    acc = R.identity_accumulator(p.polynomial_size, 1, bits, modulus_log=modulus_log)
    return p, glwe_sk, fbsk, msgs, cts, acc


def test_whole_pbs_native():
    p, glwe_sk, fbsk, msgs, cts, acc = _small_pbs(4, 128)
    out = cc.programmable_bootstrap_f128_lwe_ciphertext_batch(cts, acc, fbsk)
    assert R.decode(R.lwe_decrypt(glwe_sk, out), 4) == msgs
    one = np.zeros((p.polynomial_size + 1, 2), dtype=np.uint64)
    cc.programmable_bootstrap_f128_lwe_ciphertext(cts[5], one, acc, fbsk)
    assert np.array_equal(one, out[5])


def test_whole_pbs_modulus_127():
    p, glwe_sk, fbsk, msgs, cts, acc = _small_pbs(3, 127)
    out = cc.programmable_bootstrap_f128_lwe_ciphertext_batch(cts, acc, fbsk, ciphertext_modulus_log=127)
    assert not np.any(out[..., 0] & np.uint64(1))  # bit 0 of every output word
    assert R.decode(R.lwe_decrypt(glwe_sk, out), 3, modulus_log=127) == msgs


def test_mirrors_raise_on_dimensions():
    p, glwe_sk, fbsk, msgs, cts, acc = _small_pbs(4, 128)
    good_out = np.zeros((p.polynomial_size + 1, 2), dtype=np.uint64)
    with pytest.raises(ValueError, match="[Ii]nput"):
        cc.programmable_bootstrap_f128_lwe_ciphertext(cts[0][:-1], good_out, acc, fbsk)
    with pytest.raises(ValueError, match="[Oo]utput"):
        cc.programmable_bootstrap_f128_lwe_ciphertext(cts[0], good_out[:-1], acc, fbsk)
    with pytest.raises(ValueError, match="[Aa]ccumulator"):
        cc.programmable_bootstrap_f128_lwe_ciphertext(cts[0], good_out, acc[:-1], fbsk)
    with pytest.raises(ValueError, match="[Ii]nput"):
        cc.programmable_bootstrap_f128_lwe_ciphertext_batch(cts[:, :-1], acc, fbsk)
