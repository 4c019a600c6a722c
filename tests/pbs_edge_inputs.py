"""Chosen decomposer inputs for the PBS parity tests (test_pbs_shapes_gpu.py), checked on the CPU by
test_pbs_edge_inputs.py.

The decomposer of a blind rotation never sees the caller's words: CMUX i decomposes the difference
X^(a~_i) acc - acc.  crafted_lut solves that for the FIRST CMUX: for target polynomials D it returns
the accumulator acc with X acc - acc = D (negacyclic, mod 2^64), so that with acc as the LUT, body
b = 0 (no initial rotation) and mask word UNIT_MASK(N) (a~ = 1) the first CMUX decomposes exactly
D; every later CMUX decomposes data-dependent words.

    D[j] = acc[j-1] - acc[j]  (j >= 1),   D[0] = -acc[N-1] - acc[0]
    =>  acc[j] = acc[0] - sum(D[1..j]),   2 acc[0] = sum(D[1:]) - D[0]

which has a solution when sum(D) is even; otherwise the lowest bit of one free word of D (far below
every decomposed bit) is flipped.

pbs_edge_words fills one polynomial of D with the worst-case words of a (base_log, level)
decomposition: the families of test_keyswitch_reference.edge_rows plus the two words on either side
of the rounding boundary, with the one-level expectations edge_rows does not cover.
"""
import numpy as np

from ggsw_reference import Ref

U64 = np.uint64


def unit_mask(N):
    """the mask word whose modulus switch to 2N is 1."""
    return U64(1 << (64 - (2 * N).bit_length() + 1))


def negacyclic_mul_x(p):
    """X p for polynomials along the last axis."""
    return np.concatenate([U64(0) - p[..., -1:], p[..., :-1]], axis=-1)


def crafted_lut(D, free=None, seed=0):
    """(acc, D'): acc [(k+1)][N] u64 with X acc - acc = D' and D' = D up to the lowest bit of one word
    per polynomial whose sum is odd, chosen (seeded) among the positions where `free` (bool [N],
    default everywhere) holds."""
    D = np.array(D, dtype=U64)
    assert D.ndim == 2
    N = D.shape[1]
    rng = np.random.default_rng(seed)
    cand = np.arange(N) if free is None else np.nonzero(free)[0]
    for row in D:
        if int(np.sum(row, dtype=U64)) & 1:
            row[rng.choice(cand)] ^= U64(1)
    tail = np.cumsum(D[:, 1:], axis=1, dtype=U64)           # sum(D[1..j]), wrapping
    twice = tail[:, -1] - D[:, 0]
    assert not (twice & U64(1)).any()
    acc = np.empty_like(D)
    acc[:, 0] = twice >> U64(1)
    acc[:, 1:] = acc[:, :1] - tail
    assert np.array_equal(negacyclic_mul_x(acc) - acc, D)
    return acc, D


def edge_families(B, L):
    """[(name, word, expected signed digits level 1..L)] of the (B, L) decomposition."""
    half = 1 << (B - 1)
    field = lambda v, lvl: v << (64 - B * lvl)  # noqa: E731
    every = lambda v: sum(field(v, lvl) for lvl in range(1, L + 1))  # noqa: E731
    rnd = 63 - B * L  # the rounding bit
    assert rnd >= 0
    fam = [("zero", 0, [0] * L),
           ("top_bit", 1 << 63, [half] + [0] * (L - 1)),       # a tie with nothing above: +2^(B-1)
           ("all_ones", (1 << 64) - 1, [0] * L)]               # the rounding overflow: every digit 0
    for lvl in range(1, L + 1):                                # +2^(B-1): the int16 edge at B = 15
        fam.append((f"single_{lvl}", field(half, lvl), [half if m == lvl else 0 for m in range(1, L + 1)]))
    # every field 2^(B-1): the tie at level L carries (the field above has its top bit set) and the
    # carries run through every level; with one level nothing is above the tie: +2^(B-1)
    fam.append(("heavy_neg", every(half), [half] if L == 1 else [-(half - 1)] * (L - 1) + [-half]))
    fam.append(("heavy_pos", every(half - 1), [half - 1] * L))
    # below the rounding boundary the fields stay; at it the lowest field rounds up into the tie,
    # which does not carry (the field above, 2^(B-1) - 1, has its top bit clear)
    fam.append(("round_down", every(half - 1) | ((1 << rnd) - 1), [half - 1] * L))
    fam.append(("round_up", every(half - 1) | (1 << rnd), [half - 1] * (L - 1) + [half]))
    return fam


def edge_positions(N):
    """bool [N]: the positions pbs_edge_words fills with edge words (the others are random)."""
    return np.arange(N) % 2 == 0


def pbs_edge_words(B, L, N, seed):
    """[N] u64, one polynomial of D: the edge families in turn at the even positions (each many times,
    so every wave and lane of a kernel meets them, the order rotated by the seed), random words at
    the odd ones.  The digits of the edge words are asserted against their closed forms."""
    fam = edge_families(B, L)
    words = np.array([w for _, w, _ in fam], dtype=U64)
    d = Ref(None, 0, 0, B, L).digits(words).astype(np.int64)   # [level - 1][family]
    for j, (name, _, exp) in enumerate(fam):
        assert [int(v) for v in d[:, j]] == exp, (name, B, L, d[:, j], exp)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 64, N, dtype=U64)
    even = np.nonzero(edge_positions(N))[0]
    x[even] = words[(np.arange(even.size) + seed) % len(fam)]
    return x


def crafted_case(B, L, N, k, seed):
    """(cts [3][2], lut [(k+1) N], D [(k+1)][N]) of the n = 1 crafted case: a~ = 1 and b = 0 (the
    first and only CMUX decomposes exactly D), b~ = N (it decomposes -D) and b~ = 2N (D again, through
    the body's rounding overflow)."""
    D = np.stack([pbs_edge_words(B, L, N, seed + r) for r in range(k + 1)])
    acc, D = crafted_lut(D, free=~edge_positions(N), seed=seed)
    cts = np.empty((3, 2), dtype=U64)
    cts[:, 0] = unit_mask(N)
    cts[:, 1] = [0, 1 << 63, (1 << 64) - 1]
    return cts, acc.ravel(), D
