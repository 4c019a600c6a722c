"""The integer layer's device glue (csrc/lwe_ops.hip: lwe_scalar_mul_add_kernel, trivial_pbs_kernel)
against numpy u64 arithmetic, on engines with no keys: one of 2_2, and for the trivial PBS one of each of 1_1,
2_2, 3_3 and 4_4.  Elsewhere these kernels run only inside the radix integer DAGs, at their strides and LUTs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = np.uint64
SENTINEL = 0xA5C3_0FF0_5A3C_F00F
WORDS = 743  # one small LWE of 2_2; 3 rows x 743 words = 2229 elements, 8 workgroups and 181 threads of a ninth


@pytest.fixture(scope="module")
def eng(params_2_2):
    from tfhe_mi355 import Engine

    return Engine(params_2_2, 0)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=U64, order="C").view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _sync():
    import torch

    torch.cuda.current_stream().synchronize()


@pytest.mark.parametrize("scalar", [0, 1, 3, 2 ** 64 - 1, 2 ** 63])
def test_lwe_scalar_mul_add(eng, scalar):
    """y = block 3 of a [3 rows][5 blocks][743 words] tensor (row stride 5 x 743); x = block 1 of a
    [3][4][743] one (stride 4 x 743), block 0 of y's own tensor, or none.  Every other word of both
    tensors stays as it was."""
    rng = np.random.default_rng(scalar % 1000)
    Y = rng.integers(0, 1 << 64, (3, 5, WORDS), dtype=U64)
    X = rng.integers(0, 1 << 64, (3, 4, WORDS), dtype=U64)
    assert (3 * WORDS) % 256
    for src in ("other", "own", None):
        d_y, d_x = _dev(Y), _dev(X)
        y_ptr = d_y.data_ptr() + 8 * 3 * WORDS
        exp = Y.copy()
        exp[:, 3] = Y[:, 3] * U64(scalar)
        if src == "other":
            eng.lwe_scalar_mul_add_async(y_ptr, d_x.data_ptr() + 8 * WORDS, scalar, 3, WORDS, 5 * WORDS, 4 * WORDS)
            exp[:, 3] += X[:, 1]
        elif src == "own":
            eng.lwe_scalar_mul_add_async(y_ptr, d_y.data_ptr(), scalar, 3, WORDS, 5 * WORDS, 5 * WORDS)
            exp[:, 3] += Y[:, 0]
        else:
            eng.lwe_scalar_mul_add_async(y_ptr, None, scalar, 3, WORDS, 5 * WORDS)
        _sync()
        got = _host(d_y)
        assert np.array_equal(got[:, 3], exp[:, 3]), f"x = {src}"
        assert np.array_equal(got, exp), f"x = {src}: a neighbouring block was written"
        assert np.array_equal(_host(d_x), X)


def test_lwe_scalar_mul_add_refuses_a_stride_below_the_row(eng):
    from tfhe_mi355 import EngineError

    d_y = _dev(np.zeros((3, WORDS), dtype=U64))
    with pytest.raises(EngineError, match="stride smaller than the row"):
        eng.lwe_scalar_mul_add_async(d_y.data_ptr(), None, 3, 3, WORDS, WORDS - 1)
    with pytest.raises(EngineError, match="stride smaller than the row"):
        eng.lwe_scalar_mul_add_async(d_y.data_ptr(), d_y.data_ptr(), 3, 3, WORDS, WORDS, WORDS - 1)


# (set, words of a row): the big LWE size of each set, and the 743 words of the 2_2 instance this test began with.
# delta, modulus_sup, box, k: 2^61, 4, 128, 3 | 2^59, 16, 128, 1 | 2^57, 64, 128, 1 | 2^55, 256, 128, 1
TRIVIAL_PBS = [("2_2", WORDS), ("1_1", 3 * 512 + 1), ("2_2", 2048 + 1), ("3_3", 8192 + 1), ("4_4", 32768 + 1)]


@pytest.mark.parametrize("name,words", TRIVIAL_PBS, ids=[f"{n}-{w}" for n, w in TRIVIAL_PBS])
def test_trivial_pbs(orc, name, words):
    """bodies v delta and v delta + delta - 1 for every v in [0, 2 msup), and 2^64 - 1 (v = 2 msup - 1),
    cycled over 257 rows at least (a second workgroup) of stride words + 7: the body becomes the LUT's box value
    of v mod msup, negated from the padding bit on; the (zero) masks and the words between the rows stay.
    One engine per set, no keys: the kernel takes delta, modulus_sup, box and the body's offset k N in the LUT
    from the engine's parameters."""
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import SHORTINT_ALL

    m, c = name.split("_")
    p = SHORTINT_ALL[f"PARAM_MESSAGE_{m}_CARRY_{c}_KS_PBS"]
    eng = Engine(p, 0)
    WORDS = words  # noqa: N806  (the body below is the 2_2 test's, word for word)
    N, k = p.polynomial_size, p.glwe_dimension
    assert words == 743 or words == k * N + 1
    msup, delta = p.message_modulus * p.carry_modulus, p.delta
    box = N // msup
    f = lambda m: (5 * m + 3) % msup  # noqa: E731  (a bijection: every box differs)
    lut = orc.fill_accumulator(N, k, p.message_modulus, p.carry_modulus, f)
    lut_body = lut[k * N:]
    assert [int(lut_body[v * box]) for v in range(msup)] == [f(v) * delta for v in range(msup)]
    vs = list(range(2 * msup))
    bodies = [v * delta for v in vs] + [v * delta + delta - 1 for v in vs] + [2 ** 64 - 1]
    values = vs + vs + [2 * msup - 1]
    rows, stride = max(257, len(bodies)), WORDS + 7       # 4_4 has 1025 bodies: every one gets a row
    pick = np.arange(rows) % len(bodies)
    buf = np.zeros((rows, stride), dtype=U64)
    buf[:, WORDS:] = U64(SENTINEL)
    buf[:, WORDS - 1] = np.array(bodies, dtype=U64)[pick]
    exp = buf.copy()
    want = [(f(v % msup) * delta * (-1 if v >= msup else 1)) % 2 ** 64 for v in values]
    exp[:, WORDS - 1] = np.array(want, dtype=U64)[pick]
    d_buf = _dev(buf)
    eng.trivial_pbs_async(d_buf.data_ptr() + 8 * (WORDS - 1), rows, stride, _dev(lut))
    _sync()
    got = _host(d_buf)
    bad = np.flatnonzero(got[:, WORDS - 1] != exp[:, WORDS - 1])
    assert bad.size == 0, f"rows {bad.tolist()[:16]} (value = row % {len(bodies)})"
    assert not got[:, :WORDS - 1].any()
    assert np.array_equal(got, exp)
