"""The even transistor without a GPU: the numpy decomposer and the oracle's exact product that the
reference (tests/glwe_mult_reference.py) stands on, the client-side relinearisation key, and the whole
lwe_mult / woppbs_lut chain of gadget.ServerKey on the CPU reference engine, by decryption."""
import numpy as np
import pytest

import glwe_mult_reference as R

U64 = np.uint64


# ---- what the reference stands on ------------------------------------------------------------------
def test_numpy_decomposer_matches_reference_kats(orc):
    # decomposer.rs:95-96 (u32 KAT in the top 32 bits of a u64), term.rs:48 / :144
    assert int(R.closest_representable(1_340_987_234 << 32, 4, 3)[0]) >> 32 == 1_341_128_704
    terms = R.decompose(U64((2 ** 19) << 32), 4, 3)
    assert int(terms[0, 0]) == 1 and (int(terms[0, 0]) << (32 - 4 * 3)) == 1048576


@pytest.mark.parametrize("base_log,level", [(6, 4), (1, 3), (31, 2), (7, 9), (23, 1)])
def test_numpy_decomposer_matches_oracle(orc, base_log, level):
    rng = np.random.default_rng(base_log * 64 + level)
    x = np.concatenate([rng.integers(0, 1 << 64, 300, dtype=U64),
                        np.array([0, 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1], dtype=U64)])
    digits = R.decompose(x, base_log, level)
    assert digits.min() >= -(1 << (base_log - 1)) and digits.max() <= 1 << (base_log - 1)
    for c, v in enumerate(x):
        assert int(R.closest_representable(v, base_log, level)[0]) == orc.closest_representable(int(v), base_log, level)
        assert [int(d) % (1 << 64) for d in digits[:, c]] == orc.decompose(int(v), base_log, level)


def test_reference_product_matches_schoolbook(orc):
    """tensor_product at N = 16, k = 2 against products written out term by term in Python integers."""
    N, k, log_p = 16, 2, 4
    rng = np.random.default_rng(16)
    lhs, rhs = rng.integers(0, 1 << 64, (2, 3, (k + 1) * N), dtype=U64)

    def mul(a, b):
        out = [0] * N
        for i in range(N):
            for j in range(N):
                if i + j < N:
                    out[i + j] += int(a[i]) * int(b[j])
                else:
                    out[i + j - N] -= int(a[i]) * int(b[j])
        return out

    out, tr = R.tensor_product(orc, lhs, rhs, k, N, log_p)
    for c in range(3):
        A = (lhs[c] >> U64(30)).reshape(k + 1, N)
        B = (rhs[c] >> U64(30)).reshape(k + 1, N)
        want_out = [[x + y for x, y in zip(mul(A[i], B[k]), mul(B[i], A[k]))] for i in range(k)] + [mul(A[k], B[k])]
        want_tr = {R.block_index(i, i): mul(A[i], B[i]) for i in range(k)}
        want_tr[R.block_index(1, 0)] = [x + y for x, y in zip(mul(A[1], B[0]), mul(A[0], B[1]))]
        assert [[v % (1 << 64) for v in p] for p in want_out] == out[c].reshape(k + 1, N).tolist()
        for n, p in want_tr.items():
            assert [v % (1 << 64) for v in p] == tr[c, n].tolist()


def test_block_order_k5():
    pairs = R.block_pairs(5)
    assert pairs == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3),
                     (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)]
    assert [R.block_index(i, j) for i, j in pairs] == list(range(15))


# ---- the client's key ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N,B,L", [(2, 256, 6, 4), (1, 512, 5, 8), (5, 256, 31, 2)])
def test_client_relinearization_key_is_valid(orc, k, N, B, L):
    """Every GLWE of the key decrypts to (S_i S_j) << (64 - B lvl), level L first, within 2^(64 - 40): the
    phase error is the encryption noise alone, std 8.67e-19 * 2^64 = 16, so 2^24 is far beyond any tail."""
    from tfhe_mi355 import client

    std = 8.673617379884035e-19
    sk = client.gen_binary_key(77 + N, 2, k * N)
    rlk = client.gen_relinearization_key(78 + k, sk, k, N, B, L, std)
    assert rlk.shape == (k * (k + 1) // 2, L, (k + 1) * N) and rlk.dtype == U64
    S = sk.reshape(k, N)
    for n, (i, j) in enumerate(R.block_pairs(k)):
        prod = R.poly_mul(orc, S[i], S[j])
        for l in range(L):
            want = prod << U64(64 - B * (L - l))  # GLWE l of a block is level L - l
            assert R.torus_distance(R.glwe_phase(orc, sk, rlk[n, l], k, N), want).max() < 2.0 ** 24
    # the numpy generator of the reference module obeys the same rule
    ref = R.gen_relinearization_key(orc, np.random.default_rng(5), sk, k, N, B, L, std)
    assert ref.shape == rlk.shape
    want = R.poly_mul(orc, S[k - 1], S[0]) << U64(64 - B * L)
    assert R.torus_distance(R.glwe_phase(orc, sk, ref[R.block_index(k - 1, 0), 0], k, N), want).max() < 2.0 ** 24


# ---- the chain on the CPU reference engine --------------------------------------------------------------
@pytest.fixture(scope="module")
def server_keys():
    from tfhe_mi355 import gadget

    cache = {}

    def get(name):
        if name not in cache:
            P = R.mult_sets()[name]
            ck = gadget.ClientKey(P, seed=5)
            cache[name] = (ck, gadget.ServerKey(ck, engine=R.RefEngine(P)))
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["sha3", "default"])
def test_lwe_mult_decrypts_to_product(server_keys, name):
    """All 16 message pairs at p = 4 decrypt to m1 m2 mod 4, and the worst distance of a phase to the
    exact product m1 m2 2^62 stays 2 bits under the decision distance 2^64 / (2 p) = 2^61.

    Measured worst distance: 2^57.54 at the SHA3 shape (k = 5, N = 256), 2^57.65 at the default shape
    (k = 2, N = 512), both with the 6 x 4 keyswitch decomposition.  The floor is the algorithm's own (the
    truncating shift, and the cross terms of one operand's shift error with the other's unreduced phase).
    p = 16 decrypts all 86 pairs tried at both shapes but with worst distances 2^58.75 and 2^58.87, over
    the 2^57 that leaves two bits there, so it is not asserted."""
    from tfhe_mi355.gadget import Encoding

    ck, sk = server_keys(name)
    p = 4
    enc = Encoding.new_trivial_wopbs(p)
    pairs = [(a, b) for a in range(p) for b in range(p)]
    lhs = ck.encrypt_arithmetic_many([a for a, _ in pairs], enc)
    rhs = ck.encrypt_arithmetic_many([b for _, b in pairs], enc)
    out = sk.lwe_mult_batch(lhs, rhs, enc)
    assert all(c.encoding == enc for c in out)
    want = [a * b % p for a, b in pairs]
    exact = np.array([w * ((1 << 64) // p) for w in want], dtype=U64)
    worst = R.torus_distance(ck._phases(out), exact).max()
    print(f"{name}: worst distance to the exact product 2^{np.log2(worst):.2f}")
    assert ck.decrypt_many(out) == want
    assert worst <= 2.0 ** 64 / (2 * p) / 4
    single = sk.lwe_mult(lhs[7], rhs[7], enc)
    assert np.array_equal(single.ct, out[7].ct)


WOP_FUNCTIONS = {"x+1": lambda x: (x + 1) % 4, "3x^2+2": lambda x: (3 * x * x + 2) % 4}


@pytest.mark.parametrize("fname", list(WOP_FUNCTIONS))
def test_woppbs_lut_equals_clear_model(server_keys, fname):
    """woppbs_lut on Encoding.new_trivial_wopbs(4) inputs, all four messages, at the AES_23 shape with
    pbs 7 x 4 and ks 6 x 4: the chain decrypts to the clear model of glwe_mult_reference.woppbs_lut_clear,
    which is f(2x mod 4) -- [1, 3, 1, 3] for x + 1, [2, 2, 2, 2] for 3x^2 + 2 -- and not f(x): the
    reference's wopbs accumulator lays its p windows over half the torus."""
    from tfhe_mi355.gadget import Encoding

    ck, sk = server_keys("aes23")
    f = WOP_FUNCTIONS[fname]
    enc = Encoding.new_trivial_wopbs(4)
    cts = ck.encrypt_arithmetic_many([0, 1, 2, 3], enc)
    out = sk.woppbs_lut_batch(cts, enc, f)
    model = [R.woppbs_lut_clear(x, enc, enc, f) for x in range(4)]
    assert model == [f(2 * x % 4) for x in range(4)]
    assert ck.decrypt_many(out) == model
    assert np.array_equal(sk.woppbs_lut(cts[3], enc, f).ct, out[3].ct)


def test_python_side_refusals(server_keys):
    from tfhe_mi355 import gadget
    from tfhe_mi355.gadget import Encoding

    ck, sk = server_keys("sha3")
    enc4, enc8, enc16 = (Encoding.new_trivial_wopbs(p) for p in (4, 8, 16))
    a, b = ck.encrypt_arithmetic_many([1, 2], enc4)
    with pytest.raises(AssertionError, match="odd"):  # p = 8: log_p = 3
        sk.lwe_mult(ck.encrypt_arithmetic(1, enc8), ck.encrypt_arithmetic(1, enc8), enc8)
    with pytest.raises(AssertionError, match="unequal moduli"):
        sk.lwe_mult(a, ck.encrypt_arithmetic(1, enc16), enc4)
    with pytest.raises(ValueError, match="trivial"):
        sk.lwe_mult(a, sk.trivial_encrypt(1), enc4)
    with pytest.raises(ValueError, match="trivial"):
        sk.woppbs_lut(sk.trivial_encrypt(1), enc4, lambda x: x)
    small = gadget.ServerKey.__new__(gadget.ServerKey)  # the order check comes before any key is touched
    small.pbs_order = "BootstrapKeyswitch"
    with pytest.raises(NotImplementedError, match="BootstrapKeyswitch"):
        small.lwe_mult(a, b, enc4)
