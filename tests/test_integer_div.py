"""The unsigned radix division (div_rem, div, rem) and unsigned_overflowing_sub (tfhe_mi355/integer.py) on the host
path, oracle engine, at lwe_dimension = 8: every row of every case of integer_div_cases.py against plain Python
integers, pbs_count and launches against the restated loop structure of the reference, the zero-test helpers' edge
forms, the refusals, and a set with 3 message bits."""
import numpy as np
import pytest

import integer_div_cases as C
from conftest import OracleEngine


@pytest.fixture(scope="module")
def host_key():
    return C.keys(OracleEngine(C.params(), threads=4))


def test_case_list_is_complete():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids)) == len(C.BLOCKS) * len(C.OPS) * len(C.VARIANTS) == 100
    assert C.BLOCKS == (1, 2, 3, 5, 8) and C.ROWS % C.K == 0 and C.ROWS >= C.CRAFTED + 2
    for nb in C.BLOCKS:
        M = C.MSG ** nb
        v = C.values(C.Case("div_rem", "clean", nb, 77))
        a, b = v["lhs"], v["rhs"]
        assert all(0 <= x < M for x in a + b)
        assert b[0] == 0 and b[1] == 1 and a[2] == b[2] != 0 and b[3] == a[3] + 1
        assert a[4] == b[4] == M - 1 and a[5] == 0 and b[5] != 0 and (a[6], b[6]) == (M - 1, 1)
        assert b[7] >= M // 2
        assert b[8] == C.MSG ** (nb // 2) and b[9] == 2 * C.MSG ** (nb // 2)      # bit 2 (nb // 2) and the bit above it
        assert all(x == C.TRIVIAL_DIVISOR(nb) for x in C.values(C.Case("div", "trivial_divisor", nb, 1))["rhs"])


def test_plain_semantics():
    assert C.plain("div_rem", 13, 4, 2) == (3, 1)
    assert C.plain("div_rem", 13, 0, 2) == (15, 13)                # the long-division loop on a zero divisor
    assert C.plain("div", 13, 14, 2) == (0,) and C.plain("rem", 13, 14, 2) == (13,)
    assert C.plain(C.SUB, 3, 5, 2) == (14, 1) and C.plain(C.SUB, 5, 5, 2) == (0, 0)


# launches of a clean division worked out by hand from the reference.  One iteration at live width L (the blocks of
# the remainder that can be non-zero) is one pass of trims and shifts, max(2 + ceil(log2 L), depth of the zero test)
# joined passes, one pass of zero-outs and quotient bit; one more pass cleans quotient and remainder.  At 2_2 the zero
# test of U upper blocks takes one pass for U <= 5 and two up to 75, never more than the sub at the same iteration
# except at L = 1, where both take two.  8 blocks, L = 1, 1, 2, 2, .. 8, 8:
#   (2 + 2 + 3 + 3 + 4 * 4 + 8 * 5) + 2 * 16 + 1 = 99;    16 blocks: 66 + 16 * 6 + 2 * 32 + 1 = 227.
def test_restated_loops_give_the_hand_counts(host_key):
    assert C.shadow_of_clean_division(8)[1] == 99 and C.shadow_of_clean_division(16)[1] == 227
    assert C.shadow(C.Case("div_rem", "clean", 8, 0))[1] == C.shadow(C.Case("rem", "unchecked", 8, 0))[1] == 99
    # the overflowing sub: every block in each of its 2 + ceil(log2 nb) passes but the prefix sum's, which take
    # nb - 1, nb - 2, nb - 4 blocks: 8 + (7 + 6 + 4) + 8 = 33 LUTs a row in 5 passes
    assert C.shadow(C.Case(C.SUB, "clean", 8, 0)) == (33 * C.K, 5)
    assert C.shadow(C.Case(C.SUB, "clean", 1, 0)) == (2 * C.K, 2)
    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == "div_rem-clean-b8")
    C.run(case, sks, C.encrypt(ck, case), 0)
    assert sks.launches == 99 and (sks.pbs_count, sks.launches) == C.shadow(case)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_div_case(host_key, case):
    ck, sks = host_key
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc["lhs"] + enc["rhs"]]
    want = C.expected(case)
    for b in range(C.ROWS // C.K):
        results, lhs, rhs = C.run(case, sks, enc, b)
        assert (sks.pbs_count, sks.launches) == C.shadow(case), (b, sks.pbs_count, sks.launches)
        out = [sks.to_host(r) for r in results]
        assert C.decrypted(ck, case, out) == want[b * C.K:(b + 1) * C.K], b
        for r, n in zip(out, C.result_blocks(case)):
            assert r.num_blocks == n and r.count == C.K
            assert r.block_carries_are_empty(C.MSG) and all(d < C.MSG for d in r.degree)
        if case.op == C.SUB:
            assert out[1].degree == [1]                # the form if_then_else_parallelized takes as its condition
        lhs0, rhs0 = C.operands(case, sks, enc, b)     # the operands as they were handed in
        if not C.assigns(case, b):
            assert np.array_equal(lhs.data, lhs0.data) and lhs.degree == lhs0.degree and lhs.noise == lhs0.noise
        assert np.array_equal(rhs.data, rhs0.data) and rhs.degree == rhs0.degree and rhs.noise == rhs0.noise
    assert all(np.array_equal(e.data, d) for e, d in zip(enc["lhs"] + enc["rhs"], before))


def test_the_overflow_block_is_a_condition(host_key):
    """min(a, b) spelled a - b overflowed ? a : b"""
    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == f"{C.SUB}-clean-b3")
    enc, v = C.encrypt(ck, case), C.values(case)
    lhs, rhs = C.operands(case, sks, enc, 0)
    _, overflowed = sks.unsigned_overflowing_sub_parallelized(lhs, rhs)
    assert overflowed.num_blocks == 1 and overflowed.degree == [1] and overflowed.data.shape == (C.K, 1, sks.lwe_size)
    res = sks.if_then_else_parallelized(overflowed, lhs, rhs)
    assert C.decrypt(ck, sks.to_host(res), 3) == [min(a, b) for a, b in zip(v["lhs"][:C.K], v["rhs"][:C.K])]


# ---- the zero tests -----------------------------------------------------------------------------------------------
def _drive(sks, branch):
    from tfhe_mi355.integer import _PbsLayer

    layer = _PbsLayer(sks)
    sks.pbs_count = sks.launches = 0
    return sks._join(layer, branch(layer))[0]


def test_zero_test_helpers_and_their_edge_forms(host_key):
    from tfhe_mi355 import integer

    ck, sks = host_key
    nb = 8
    rows = [0, 1 << 14, 5]                              # zero; only the top block set; only blocks 0 and 1
    x = integer.ClientKey(ck, nb).encrypt(np.asarray(rows, dtype=np.uint64))
    one = integer.ClientKey(ck, 1)
    blocks = [(x, j) for j in range(nb)]
    for equality in (False, True):
        cmp = _drive(sks, lambda layer: sks._compare_blocks_with_zero_steps(layer, blocks, equality))
        assert len(cmp) == 2 and (sks.pbs_count, sks.launches) == (2 * C.K, 1)     # chunks of 5 and 3 blocks
        got = [[int(v) for v in one.decrypt(integer.RadixBatch(rb.data[:, j:j + 1], [1], [1]))] for rb, j in cmp]
        want = [[int((r % 4 ** 5 == 0) == equality) for r in rows], [int((r >> 10 == 0) == equality) for r in rows]]
        assert got == want
        name = "_are_all_comparisons_block_true_steps" if equality else "_is_at_least_one_comparisons_block_true_steps"
        rb, j = _drive(sks, lambda layer: getattr(sks, name)(layer, C.K, cmp))
        assert (sks.pbs_count, sks.launches) == (C.K, 1)
        assert [int(v) for v in one.decrypt(integer.RadixBatch(rb.data[:, j:j + 1], [1], [1]))] == \
            [int((r == 0) == equality) for r in rows]
        # a single block is returned as it is, without a PBS
        assert _drive(sks, lambda layer: getattr(sks, name)(layer, C.K, cmp[1:])) == cmp[1]
        assert (sks.pbs_count, sks.launches) == (0, 0)
        # an empty list gives a trivial 1
        rb, j = _drive(sks, lambda layer: getattr(sks, name)(layer, C.K, []))
        assert (sks.pbs_count, sks.launches) == (0, 0) and rb.is_trivial_block(j) and rb.degree[j] == 1
        assert [int(v) for v in one.decrypt(integer.RadixBatch(rb.data[:, j:j + 1], [1], [0]))] == [1] * C.K
    assert _drive(sks, lambda layer: sks._compare_blocks_with_zero_steps(layer, [], False)) == []
    assert (sks.pbs_count, sks.launches) == (0, 0)


def test_lut_cache_does_not_grow_on_a_repeated_call(host_key):
    ck, sks = host_key
    for cid in ("div_rem-clean-b2", f"{C.SUB}-clean-b3"):
        case = next(c for c in C.CASES if c.id == cid)
        enc = C.encrypt(ck, case)
        first = C.run(case, sks, enc, 0)[0]
        luts = dict(sks._luts)
        again = C.run(case, sks, enc, 0)[0]
        assert sks._luts.keys() == luts.keys() and all(sks._luts[k] is v for k, v in luts.items())
        assert all(np.array_equal(a.data, b.data) for a, b in zip(first, again))
    stack = list(sks._div_luts().values())
    # 2 borrow, prefix, message, 2 shift, non-zero, 2 masks, 2 x 2 zero-outs, 2 quotient bits
    assert len(stack) == len({id(t) for t in stack}) == 15 and stack == list(sks._div_luts().values())


# ---- refusals ------------------------------------------------------------------------------------------------------
DIV_METHODS = [f"{u}{op}{a}_parallelized" for op in ("div", "rem") for u in ("unchecked_", "") for a in ("_assign", "")] + \
    ["unchecked_div_rem_parallelized", "div_rem_parallelized"]
SUB_METHODS = ["unchecked_unsigned_overflowing_sub_parallelized", "unsigned_overflowing_sub_parallelized"]


def test_every_form_exists():
    from tfhe_mi355 import integer

    assert len(DIV_METHODS) == 10 and len(set(DIV_METHODS)) == 10
    for name in DIV_METHODS + SUB_METHODS:
        assert callable(getattr(integer.ServerKey, name)), name
        assert getattr(integer.ServerKey, name).__name__ == name


def _rule(msg, carry):
    """div_refusal's conditions, restated: True where the division is refused"""
    total = msg * carry
    power_of_two = msg >= 2 and msg & (msg - 1) == 0
    hillis_steele = total >= 16                         # the only borrow propagation there is
    difference_fits = 2 * msg - 1 < total               # lhs - rhs + msg
    states_fit = 3 <= msg and 2 * msg + 2 < total       # borrow states 0, 1, 2 and two of them packed
    shift_fits = msg * msg - 1 < total                  # previous * msg + current
    bookkeeping = 3 * msg - 2 < total                   # degree of remainder1 + remainder2 - divisor + msg
    factor_3 = 3 * (msg - 1) + 2 < total
    flags_fit = msg + 1 < total
    return not (power_of_two and hillis_steele and difference_fits and states_fit and shift_fits and bookkeeping
                and factor_3 and flags_fit)


def test_div_refusal_over_every_set():
    from tfhe_mi355.integer import div_refusal, overflowing_sub_refusal
    from tfhe_mi355.parameters import SHORTINT_ALL

    assert len(SHORTINT_ALL) >= 40
    accepted = set()
    for name, P in SHORTINT_ALL.items():
        msg, carry = P.message_modulus, P.carry_modulus
        assert (div_refusal(msg, carry) is not None) == _rule(msg, carry), name
        if div_refusal(msg, carry) is None:
            accepted.add(name)
            assert overflowing_sub_refusal(msg, carry) is None, name
    assert {"PARAM_MESSAGE_2_CARRY_2_KS_PBS", "PARAM_MESSAGE_4_CARRY_4_KS_PBS", C.SET_3_3} <= accepted
    assert not {"PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_3_CARRY_2_KS_PBS", "PARAM_MESSAGE_2_CARRY_1_KS_PBS",
                "PARAM_MESSAGE_4_CARRY_0_KS_PBS"} & accepted
    assert "power of two" in div_refusal(3, 8) and "factor 3" not in (div_refusal(4, 4) or "")
    assert "Hillis-Steele" in div_refusal(2, 4) and "carry_modulus < message_modulus" in div_refusal(8, 4)
    assert "borrow state" in div_refusal(2, 8)
    # the sub alone packs no two messages: 3_2 serves it
    assert overflowing_sub_refusal(8, 4) is None and overflowing_sub_refusal(2, 8) is not None


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


@pytest.mark.parametrize("name", ["PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_2_CARRY_1_KS_PBS",
                                  "PARAM_MESSAGE_3_CARRY_2_KS_PBS", "PARAM_MESSAGE_1_CARRY_3_KS_PBS"])
def test_a_refused_set_raises_before_any_engine_call(name):
    P, sks = _inert_key(name)
    assert sks.div_refusal is not None
    x, y = _inert_operand(sks, P, 3), _inert_operand(sks, P, 3)
    dirty = _inert_operand(sks, P, 3, degree=2 * P.message_modulus - 2, noise=2)
    for op in DIV_METHODS:
        for a, b in ((x, y), (dirty, y), (x, dirty)):
            with pytest.raises(NotImplementedError, match=f"integer {op}: {name} .*is not supported: "):
                getattr(sks, op)(a, b)
    if sks.overflowing_sub_refusal:
        for op in SUB_METHODS:
            with pytest.raises(NotImplementedError, match=f"integer {op}: {name} .*is not supported: "):
                getattr(sks, op)(x, y)
    assert sks.pbs_count == 0 and sks.launches == 0
    assert not x.data.any() and not y.data.any() and not dirty.data.any()


def test_shapes_are_checked_before_the_first_launch():
    P, sks = _inert_key("PARAM_MESSAGE_2_CARRY_2_KS_PBS")
    assert sks.div_refusal is None and sks.overflowing_sub_refusal is None
    x, short, more = _inert_operand(sks, P, 3), _inert_operand(sks, P, 2), sks.create_trivial_zero(3, 3)
    dirty = _inert_operand(sks, P, 3, degree=6, noise=2)
    for op in DIV_METHODS + SUB_METHODS:
        for a, b in ((x, short), (short, x)):
            with pytest.raises(ValueError, match=f"{op}: .*{a.num_blocks} blocks .*{b.num_blocks}"):
                getattr(sks, op)(a, b)
        with pytest.raises(ValueError, match=f"{op}: 2 .*against 3"):
            getattr(sks, op)(x, more)
        if op.startswith("unchecked"):
            with pytest.raises(ValueError, match=f"{op}: the unchecked form takes operands with empty carries"):
                getattr(sks, op)(x, dirty)
    assert sks.pbs_count == 0 and sks.launches == 0 and not x.data.any() and not dirty.data.any()


# ---- 3 message bits ------------------------------------------------------------------------------------------------
def test_set_3_3_divides():
    """PARAM_MESSAGE_3_CARRY_3 (message modulus 8, carry modulus 8) at 2 blocks, T = 6: three in-block positions,
    two-bit trim masks (keep 1, 3; drop 6, 4), chunks of 9 blocks in compare_blocks_with_zero"""
    from tfhe_mi355 import integer
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[C.SET_3_3].with_(lwe_dimension=8)
    ck, sks = C.keys(OracleEngine(P, threads=4), parameters=P)
    assert sks.div_refusal is None and sks.bits == 3
    nb = C.BLOCKS_3_3
    M = 8 ** nb
    cks = integer.ClientKey(ck, nb)
    numerators, divisors = [M - 1, 0b101101, 0b011010], [0b000101, 0b100000, 0]
    x = cks.encrypt(np.asarray(numerators, dtype=np.uint64))
    y = cks.encrypt(np.asarray(divisors, dtype=np.uint64))
    x0, y0 = x.data.copy(), y.data.copy()
    sks.pbs_count = sks.launches = 0
    q, r = sks.div_rem_parallelized(x, y)
    assert (sks.pbs_count, sks.launches) == C.shadow_of_clean_division(nb, 3, 8, 8)
    # live width 1, 1, 1, 2, 2, 2: (2 + 2 + 2 + 3 + 3 + 3) + 2 * 6 + 1 passes
    assert sks.launches == 28
    got = list(zip((int(v) for v in cks.decrypt(q)), (int(v) for v in cks.decrypt(r))))
    assert got == [((a // b, a % b) if b else (M - 1, a)) for a, b in zip(numerators, divisors)]
    assert q.block_carries_are_empty(8) and r.block_carries_are_empty(8)
    assert np.array_equal(x.data, x0) and np.array_equal(y.data, y0)
    masks = sorted(k[1] for k in sks._luts if k[0] == "mask")
    assert masks == [1, 3, 4, 6]
    s, o = sks.unsigned_overflowing_sub_parallelized(x, y)
    assert [int(v) for v in cks.decrypt(s)] == [(a - b) % M for a, b in zip(numerators, divisors)]
    assert [int(v) for v in integer.ClientKey(ck, 1).decrypt(o)] == [int(a < b) for a, b in zip(numerators, divisors)]
