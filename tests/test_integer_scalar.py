"""The radix operations with a clear operand (tfhe_mi355/integer.py: scalar_add, scalar_sub, the scalar bitwise ops,
the scalar comparisons, scalar_max / scalar_min) on the host path, oracle engine, at lwe_dimension = 8: every row of
every case of integer_scalar_cases.py against plain Python integers, pbs_count and launches against the restated loop
structure of the reference, every row of a per-row batch against the one-int form called with that row's scalar, the
host statement of the clear block layer, and the refusals."""
import numpy as np
import pytest

import integer_scalar_cases as C
from conftest import OracleEngine


@pytest.fixture(scope="module")
def host_key():
    return C.keys(OracleEngine(C.params(), threads=4))


def test_case_list_is_complete():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids)) == len(C.BLOCKS) * len(C.OPS) * 4 * 2 and len(C.OPS) == 13
    for nb in C.BLOCKS:
        T = C.BITS * nb
        M = 2 ** T
        assert {0, 1, C.MSG - 1, C.MSG, M - 1, M, M + 3, C.top_zero(nb)} == set(C.SCALARS("scalar_add", nb))
        assert set(C.SCALARS("scalar_lt", nb)) == set(C.SCALARS("scalar_add", nb)) | {-1}
        if nb > 1:
            z = C.top_zero(nb)
            assert z // C.MSG ** (nb - 1) == 0 and (z // C.MSG ** (nb - 2)) % C.MSG != 0
    for case in C.CASES:
        if case.form == "rows":
            v, c = C.values(case), C.clear_rows(case)
            M, top = C.MSG ** case.nb, C.MSG ** (case.nb - 1)
            assert len(v) == len(c) == 3 * C.K and all(0 <= x < M for x in c)
            assert c[0] == M - 1 and c[1] == (C.MSG - 1) * top and c[3] == 0 and c[4] == v[4]
            assert c[5] == v[5] + 1 or v[5] == M - 1
            assert c[6] == v[6] - 1 or v[6] == 0
            assert c[7] < top
            assert C.full_width(case, 0) and not C.full_width(case, 1)     # one batch of every op is full-width
            if case.variant != "trivial":
                assert c[5] == v[5] + 1 and c[6] == v[6] - 1


def test_plain_semantics():
    assert C.plain("scalar_add", 14, 5, 2) == 3 and C.plain("scalar_sub", 3, 5, 2) == 14
    assert C.plain("scalar_sub", 3, 16 + 5, 2) == 14 and C.plain("scalar_bitor", 5, 16 + 2, 2) == 7
    assert C.plain("scalar_lt", 15, 16, 2) == 1 and C.plain("scalar_ge", 0, -1, 2) == 1 and C.plain("scalar_eq", 3, 19, 2) == 0
    assert C.plain("scalar_max", 7, 19, 2) == 3 and C.plain("scalar_min", 7, 19, 2) == 7      # the scalar modulo 2^T
    assert C.plain("scalar_max", 7, -1, 2) == 7 and C.plain("scalar_min", 7, -1, 2) == 15


# (pbs_count, launches) of K = 3 rows worked out by hand from the reference, against the restated loops; clean operands.
#   scalar_bitand b5 by 3: one digit, one LUT; by 2^T - 1: five.   scalar_add default b8: add-b8's propagation (99, 5).
#   scalar_eq b8 by 2^T - 1: 4 packed pairs, then one chunk of 4: 5 LUTs in 2 passes.
#   scalar_eq b8 by 1: one packed pair and compare_blocks_with_zero of 6 blocks (chunks of 5: 2) in one joined pass,
#     then one chunk of 3: 4 LUTs in 2 passes.   scalar_eq b8 by 0: 8 blocks against zero (2 chunks), then 1: 3 in 2.
#   scalar_lt b8 by 2^T - 1: 4 signs, 2, 1, the map: 8 LUTs in 4 passes.
#   scalar_lt b8 by 3: one digit: the sign of block 0 (one pass, no tree), joined with 7 blocks against zero (2 chunks),
#     their reduction (1), the LUT to a sign (1): passes of 3, 1, 1; then the two signs (1), then the map (1): 7 in 5.
#   scalar_lt b8 by 2^T and by -1: a trivial sign, the map is a trivial PBS: nothing.
#   scalar_max b3 by 2^T - 1: 2 signs, 1; then the cmux: 3 + 3 blocks, then 3 message extractions: 12 in 4.
#   scalar_max b3 by 2^T + 3: the sign is a trivial 0 and decides; lhs is zeroed, the sum is trivial: nothing.
#   scalar_min b3 by 2^T + 3: lhs is kept, 3 message extractions.
HAND = {("scalar_bitand", 5, 3): (3, 1), ("scalar_bitand", 5, 2 ** 10 - 1): (15, 1), ("scalar_add", 8, 1): (99, 5),
        ("scalar_eq", 8, 2 ** 16 - 1): (15, 2), ("scalar_eq", 8, 1): (12, 2), ("scalar_eq", 8, 0): (9, 2),
        ("scalar_lt", 8, 2 ** 16 - 1): (24, 4), ("scalar_lt", 8, 3): (21, 5), ("scalar_lt", 8, 2 ** 16): (0, 0),
        ("scalar_lt", 8, -1): (0, 0), ("scalar_max", 3, 63): (36, 4), ("scalar_max", 3, 67): (0, 0),
        ("scalar_min", 3, 67): (9, 1)}


def test_restated_loops_give_the_hand_counts():
    got = {}
    for op, nb, scalar in HAND:
        case = next(c for c in C.CASES if (c.op, c.variant, c.nb, c.form) == (op, "clean", nb, "int"))
        got[(op, nb, scalar)] = C.shadow(case, C.SCALARS(op, nb).index(scalar))
    assert got == HAND
    for op in ("scalar_eq", "scalar_lt", "scalar_max"):               # per row: the scalar 2^T - 1
        rows = next(c for c in C.CASES if (c.op, c.variant, c.nb, c.form) == (op, "clean", 8, "rows"))
        one = next(c for c in C.CASES if (c.op, c.variant, c.nb, c.form) == (op, "clean", 8, "int"))
        assert C.shadow(rows, 1) == C.shadow(one, C.SCALARS(op, 8).index(2 ** 16 - 1))


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_scalar_case(host_key, case):
    ck, sks = host_key
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc]
    want, nblocks = C.expected(case), C.result_blocks(case)
    total = C.MSG * C.CARRY
    for b in range(case.batches):
        clear = C.clear_operand(case, b)
        keep = clear.copy() if case.form == "rows" else clear
        res, lhs = C.run(case, sks, enc, b)
        out = sks.to_host(res)
        assert (sks.pbs_count, sks.launches) == C.shadow(case, b), (b, sks.pbs_count, sks.launches)
        assert C.decrypt(ck, out, nblocks) == want[b * C.K:(b + 1) * C.K], b
        assert out.num_blocks == nblocks and out.count == C.K
        assert all(0 <= d < total for d in out.degree), out.degree          # the scalar fitted: no block overflows
        if case.variant != "unchecked" or case.op not in C.ARITHMETIC:
            assert out.block_carries_are_empty(C.MSG)
        if case.op in C.BOOLEAN:
            assert out.degree[0] <= 1
        lhs0 = C.operand(case, sks, enc, b)           # the operand as it was handed in
        if b == 0 or not C.has_assign(case.op):       # the returning form: a dirty operand is propagated on a clone
            assert np.array_equal(lhs.data, lhs0.data) and lhs.degree == lhs0.degree and lhs.noise == lhs0.noise
        assert np.array_equal(clear, keep)
        if case.form == "rows":                       # every row against the one-int form with that row's scalar
            exact = case.op in C.ARITHMETIC or C.full_width(case, b)
            if case.variant == "trivial" and case.op in C.BITWISE + C.EQUALITY:
                exact = False                         # a LUT per row: a trivial block goes through the batched PBS
            for r, c in enumerate(int(x) for x in clear):
                one, _ = C.run(case, sks, enc, b, clear=c)
                one = sks.to_host(one)
                # max / min: the cmux skips a block of degree 0, which a zero digit of the one-int form gives
                if exact and (case.op not in C.SELECT or all((c >> (C.BITS * j)) % C.MSG for j in range(case.nb))):
                    assert np.array_equal(out.data[r], one.data[r]), (b, r, c)
                assert C.decrypt(ck, one, nblocks)[r] == want[b * C.K + r], (b, r, c)
    assert all(np.array_equal(e.data, d) for e, d in zip(enc, before))


def test_a_torch_tensor_serves_the_host_path_as_the_array_does(host_key):
    """form (c) on a key without a device: the tensor is read as the array is"""
    import torch

    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == "scalar_lt-clean-b3-rows")
    enc = C.encrypt(ck, case)
    clear = C.clear_operand(case, 1)
    a, _ = C.run(case, sks, enc, 1)
    t, _ = C.run(case, sks, enc, 1, clear=torch.from_numpy(clear.view(np.int64)))
    assert np.array_equal(a.data, t.data)


def test_host_clear_block_layer_is_the_formula():
    """_HostOps.clear_block_layer, the oracle of the device kernel, against the formula written out row by row"""
    from tfhe_mi355.integer import _ClearRows, _HostOps

    rng = np.random.default_rng(5)
    rows, words, ones = 4, 5, (1 << 64) - 1
    a = rng.integers(0, 1 << 64, (rows, words), dtype=np.uint64)
    y = rng.integers(0, 1 << 64, (rows, words), dtype=np.uint64)
    z = rng.integers(0, 1 << 64, (rows, words), dtype=np.uint64)
    clear = np.array([0, ones, 0x8000000000000005, 77], dtype=np.uint64)
    idx = np.full(2 * rows, 99, dtype=np.uint32)
    y0 = y.copy()
    part = dict(rows=_ClearRows(host=clear), negate=1, shift=62, bits=8, scale=3, index=idx[:rows], lut_base=10)
    none = dict(rows=None, negate=0, shift=0, bits=0, scale=7, index=None, lut_base=4)
    _HostOps(None).clear_block_layer([(y, 5, [(y, 2), (a, ones)], part), (z, 1, [], none)])
    for r in range(rows):
        digit = (((1 << 64) - int(clear[r])) % (1 << 64)) >> 62
        want = [(2 * int(y0[r, w]) - int(a[r, w])) % (1 << 64) for w in range(words)]
        want[-1] = (want[-1] + 5 + 3 * digit) % (1 << 64)
        assert [int(v) for v in y[r]] == want and int(idx[r]) == 10 + digit
    assert [int(x) for x in idx[:rows]] == [10, 10, 11, 13] and (idx[rows:] == 99).all()
    assert not z[:, :-1].any() and (z[:, -1] == 1).all()


# ---- refusals ------------------------------------------------------------------------------------------------------
class _NoEngine:
    def upload_bootstrap_key(self, bsk):
        pass

    def upload_keyswitch_key(self, ksk):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached on a refused call")


def _inert_key(name):
    from tfhe_mi355 import integer, shortint
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[name]
    sks = integer.ServerKey(shortint.ServerKey(None, engine=_NoEngine(), parameters=P))
    sks.lwe_size = 3
    return P, sks


def _inert_operand(sks, P, nb, degree=None, noise=1):
    x = sks.create_trivial_zero(2, nb)
    x.degree, x.noise = [P.message_modulus - 1 if degree is None else degree] * nb, [noise] * nb
    return x


def _all_methods():
    return [C.method(op, unchecked, assign) for op in C.OPS for unchecked in (True, False)
            for assign in ((False, True) if C.has_assign(op) else (False,))]


def test_every_form_exists():
    from tfhe_mi355 import integer

    names = _all_methods()
    assert len(names) == len(set(names)) == 5 * 4 + 8 * 2
    assert {"unchecked_scalar_add", "unchecked_scalar_sub_assign", "scalar_add_assign_parallelized",
            "unchecked_scalar_bitxor_assign_parallelized", "scalar_lt_parallelized", "unchecked_scalar_min_parallelized"} <= set(names)
    for name in names:
        assert callable(getattr(integer.ServerKey, name)), name


def test_clear_operands_are_checked_before_the_first_launch():
    import torch

    P, sks = _inert_key("PARAM_MESSAGE_2_CARRY_2_KS_PBS")
    x, wide = _inert_operand(sks, P, 3), _inert_operand(sks, P, 33)          # T = 6 and T = 66
    ok = np.array([1, 63], dtype=np.uint64)
    for name in _all_methods():
        f = getattr(sks, name)
        for bad in ([1, 2], 1.5, True, "3", ok.astype(np.int64), ok.astype(np.uint32), torch.tensor([1, 2], dtype=torch.int32)):
            with pytest.raises(TypeError, match=f"{name}: the clear operand is one Python int, a numpy uint64 array"):
                f(x, bad)
        for bad in (np.array([1, 2, 3], dtype=np.uint64), ok.reshape(2, 1), torch.tensor([1], dtype=torch.int64)):
            with pytest.raises(ValueError, match=f"{name}: 2 rows against clear operands of shape"):
                f(x, bad)
        with pytest.raises(ValueError, match=f"{name}: a clear operand per row must be below 2\\^6"):
            f(x, np.array([1, 64], dtype=np.uint64))
        for rows in (ok, torch.tensor([1, 2], dtype=torch.int64)):
            with pytest.raises(NotImplementedError, match=f"{name}: .*one clear operand per row is one u64, and the "
                                                          "ciphertexts hold 66 bits"):
                f(wide, rows)
        if not any(op in name for op in C.COMPARISONS):
            with pytest.raises(ValueError, match=f"{name}: the clear operand must not be negative"):
                f(x, -1)
    assert sks.pbs_count == 0 and sks.launches == 0 and not x.data.any() and not wide.data.any()


# set -> (propagation, bivariate packing, comparison) refused
RULE = {
    "PARAM_MESSAGE_2_CARRY_2_KS_PBS": (False, False, False),
    "PARAM_MESSAGE_1_CARRY_1_KS_PBS": (True, False, True),
    "PARAM_MESSAGE_2_CARRY_1_KS_PBS": (True, True, True),
    "PARAM_MESSAGE_2_CARRY_3_KS_PBS": (True, False, False),
    "PARAM_MESSAGE_3_CARRY_2_KS_PBS": (False, True, False),
    "PARAM_MESSAGE_4_CARRY_4_KS_PBS": (False, False, False),
}


@pytest.mark.parametrize("name", list(RULE))
def test_every_form_refuses_by_the_rule_before_the_first_launch(name):
    """eq / ne need carry >= msg (scalar_comparison.rs:399); the order comparisons and max / min what Comparator::new
    asks and the packing; the default forms of a dirty operand what the propagation asks; per-row operands alike"""
    P, sks = _inert_key(name)
    propagation, bivariate, comparison = RULE[name]
    assert (sks.propagation_refusal is not None, sks.bivariate_refusal is not None,
            sks.comparison_refusal is not None) == RULE[name]
    x = _inert_operand(sks, P, 3)
    dirty = _inert_operand(sks, P, 3, degree=2 * P.message_modulus - 2, noise=2)
    for clear in (1, np.array([1, 2], dtype=np.uint64)):
        for op in C.OPS:
            for unchecked in (True, False):
                f = getattr(sks, C.method(op, unchecked))
                label = f"{C.method(op, unchecked)}: {name} "
                if op in C.EQUALITY and bivariate:
                    with pytest.raises(NotImplementedError, match=label + ".*carry_modulus < message_modulus"):
                        f(x, clear)
                elif op in C.ORDERED + C.SELECT and comparison:
                    with pytest.raises(NotImplementedError, match=label + ".*at least 4 bits of space"):
                        f(x, clear)
                elif op in C.ORDERED + C.SELECT and bivariate:
                    with pytest.raises(NotImplementedError, match=label + ".*carry_modulus < message_modulus"):
                        f(x, clear)
                elif op in C.ARITHMETIC and propagation and not unchecked:
                    with pytest.raises(NotImplementedError, match=label + ".*is not supported: "):
                        f(x, clear)
                elif propagation and not unchecked:
                    with pytest.raises(NotImplementedError, match=f"full_propagate: {name} .*is not supported: "):
                        f(dirty, clear)
    assert sks.pbs_count == 0 and sks.launches == 0 and not x.data.any() and not dirty.data.any()
