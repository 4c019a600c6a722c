"""A plain numpy reference of the keyswitch GEMM (csrc/keyswitch.hip) and the edge rows the keyswitch
tests run, checked here on the CPU against the oracle; test_keyswitch_gpu.py imports both.

    out[c][j] = (j == body ? in[c][in_dim] : 0) - sum_{i, l} d[c][i][l] * K[i][l][j]      (mod 2^64)

body = out_dim for the LWE -> LWE keyswitch and kN for the LWE -> GLWE packing keyswitch; d are the
signed digits of tests/ggsw_reference.py (Ref.digits, the SignedDecomposer vectorised), the key rows
of one input word are stored level L first.
"""
import numpy as np
import pytest

from ggsw_reference import Ref

U64 = np.uint64
# (base_log, level): 2_2, the widest base at two and at 7 x 9 = 63 bits (rounding shift 0), the
# narrowest base, WoP 1_2
DECOMPOSITIONS = [(3, 5), (7, 7), (7, 9), (1, 16), (2, 4)]
N_EDGE = 7
ZERO, BODY_ONLY, TOP_BIT, ALL_ONES, SINGLE_FIELD, HEAVY_NEG, HEAVY_POS = range(N_EDGE)


def digits(base_log, level, x):
    """signed digits as int64, [level index l-1][...]."""
    return Ref(None, 0, 0, base_log, level).digits(x).astype(np.int64)


def edge_rows(base_log, level, width, count, seed):
    """max(count, N_EDGE + 1) rows of `width` words (the last word is the body):
    all zero; only the body nonzero; every word 1 << 63; every word all ones (the rounding overflow
    wraps to 0); word i with the single field 2^(B-1) at level 1 + i % L (the digit +2^(B-1), the
    fields around it zero); the heavy row, every field of every word 2^(B-1) (the carries run
    through every level: digits -2^(B-1), -(2^(B-1) - 1), ...); its positive counterpart, every field
    2^(B-1) - 1; random rows from there on."""
    B, L = base_log, level
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 64, (max(count, N_EDGE + 1), width), dtype=U64)
    x[ZERO] = 0
    x[BODY_ONLY] = 0
    x[BODY_ONLY, -1] = rng.integers(1, 1 << 64, dtype=U64)
    x[TOP_BIT] = U64(1 << 63)
    x[ALL_ONES] = ~U64(0)
    x[SINGLE_FIELD] = np.array([1 << (64 - B * (1 + i % L) + B - 1) for i in range(width)], dtype=U64)
    half = 1 << (B - 1)
    x[HEAVY_NEG] = U64(sum(half << (64 - B * lvl) for lvl in range(1, L + 1)))
    x[HEAVY_POS] = U64(sum((half - 1) << (64 - B * lvl) for lvl in range(1, L + 1)))
    d = digits(B, L, x[:N_EDGE])
    assert not d[:, ALL_ONES].any() and not d[:, ZERO].any()
    assert (np.abs(d[:, HEAVY_NEG]) >= half - 1).all() and (np.abs(d[:, HEAVY_POS]) >= half - 1).all()
    assert (d[L - 1, HEAVY_NEG] == -half).all() and (d[:, HEAVY_POS] == half - 1).all()
    assert all(d[lvl, SINGLE_FIELD].max() == half for lvl in range(L))  # +2^(B-1) at every level
    return x


def keyswitch_reference(key, in_dim, ncols, body_col, base_log, level, lwe_in):
    """[count][in_dim + 1] -> [count][ncols] under key [in_dim][level][ncols] (levels L..1)."""
    K = np.ascontiguousarray(key, dtype=U64).reshape(in_dim, level, ncols)
    x = np.ascontiguousarray(lwe_in, dtype=U64).reshape(-1, in_dim + 1)
    d = Ref(None, 0, 0, base_log, level).digits(x[:, :in_dim])  # wrapping u64
    out = np.zeros((x.shape[0], ncols), dtype=U64)
    out[:, body_col] = x[:, in_dim]
    for lvl in range(1, level + 1):
        out -= d[lvl - 1] @ K[:, level - lvl]  # integer matmul wraps mod 2^64
    return out


@pytest.fixture(scope="module")
def cases(orc):
    """per decomposition: the edge rows, two random keys and the oracle's outputs (shared, read-only)."""
    in_dim, out_dim, k, N = 64, 5, 1, 64
    out = {}
    for B, L in DECOMPOSITIONS:
        rng = np.random.default_rng(100 * B + L)
        x = edge_rows(B, L, in_dim + 1, 12, seed=B + 10 * L)
        ksk = rng.integers(0, 1 << 64, in_dim * L * (out_dim + 1), dtype=U64)
        pksk = rng.integers(0, 1 << 64, in_dim * L * (k + 1) * N, dtype=U64)
        c = dict(x=x, ksk=ksk, pksk=pksk, ks=orc.keyswitch(ksk, in_dim, out_dim, B, L, x),
                 pks=orc.packing_keyswitch(pksk, in_dim, k, N, B, L, x))
        for a in c.values():
            a.setflags(write=False)
        out[(B, L)] = c
    return out


@pytest.mark.parametrize("dec", DECOMPOSITIONS, ids=str)
def test_reference_equals_oracle_keyswitch(cases, dec):
    B, L = dec
    c = cases[dec]
    got = keyswitch_reference(c["ksk"], 64, 6, 5, B, L, c["x"])
    assert np.array_equal(got, c["ks"])
    assert not c["ks"][ZERO].any()
    for r in (BODY_ONLY, ALL_ONES):  # no digit: the body alone
        assert np.array_equal(c["ks"][r], np.array([0] * 5 + [c["x"][r, -1]], dtype=U64))


@pytest.mark.parametrize("dec", DECOMPOSITIONS, ids=str)
def test_reference_equals_oracle_packing_keyswitch(cases, dec):
    """(k, N) = (1, 64): 128 columns, the body on column kN = 64."""
    B, L = dec
    c = cases[dec]
    got = keyswitch_reference(c["pksk"], 64, 128, 64, B, L, c["x"])
    assert np.array_equal(got, c["pks"])
    assert not c["pks"][ZERO].any()
    for r in (BODY_ONLY, ALL_ONES):
        exp = np.zeros(128, dtype=U64)
        exp[64] = c["x"][r, -1]
        assert np.array_equal(c["pks"][r], exp)


@pytest.mark.parametrize("dec", DECOMPOSITIONS + [(3, 17), (7, 2), (4, 3)], ids=str)
def test_edge_row_digits_equal_the_oracle_decomposer(orc, dec):
    """Ref.digits against the oracle's scalar decomposer on three words of every edge row and of five
    random rows."""
    B, L = dec
    x = edge_rows(B, L, 19, 12, seed=7)  # at least L words: the single field visits every level
    words = [int(x[r, i]) for r in range(12) for i in (0, 3, 18)]
    d = digits(B, L, np.array(words, dtype=U64))
    for j, w in enumerate(words):
        got = [int(v) for v in np.array(orc.decompose(w, B, L), dtype=U64).astype(np.int64)]
        # the oracle yields level L first
        assert got == [int(d[lvl - 1, j]) for lvl in range(L, 0, -1)], (hex(w), B, L)
