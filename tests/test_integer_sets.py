"""The radix integer layer (tfhe_mi355/integer.py) at every modulus pair it accepts, on the host path with the oracle
engine at lwe_dimension = 8: every served case of integer_sets_cases.py decrypts to the plain-integer answer, every
refused one raises NotImplementedError naming the set before anything is launched or written.  This is what
test_integer_sets_gpu.py rests on: it compares the device path with this one bit for bit.  The other CPU tests of
the layer run PARAM_MESSAGE_2_CARRY_2 and a few operations at 3_3 and 3_2.

Also pinned here: unsigned_overflowing_sub with carry_modulus < message_modulus.  The reference serves it (the prefix
sum packs its borrow states unchecked, bivariate_pbs.rs:167-182, and they never exceed 2), so the layer does, at every
block count: the bookkeeping gives a prefix-sum output the states' bound and not the degree of the LUT that made it.
"""
import numpy as np
import pytest

import integer_sets_cases as C
from conftest import OracleEngine


@pytest.fixture(scope="module")
def host_keys():
    """set -> (ClientKey, host ServerKey), built the first time a case of the set runs"""
    made = {}

    def get(s):
        if s not in made:
            made[s] = C.keys(s, OracleEngine(C.params(s), threads=4))
        return made[s]
    return get


def test_the_table_is_the_rule_of_the_reference():
    """TABLE against the conditions written out: 4 bits per block for the propagation, the comparisons and the borrow
    prefix sum; carry >= msg for whatever packs two messages; carry <= msg for the sum's extracted carries; three bits
    for the barrel shifter; the division needs all of the sub's and the shift's"""
    for s, (m, c) in C.MODULI.items():
        four_bits, packs, bounded = m * c >= 16, c >= m, c <= m
        rule = {"sub": four_bits and bounded, "mul": four_bits and bounded and packs, "bitxor": packs, "eq": packs,
                "lt": four_bits, "max": four_bits and packs, "scalar_add": four_bits and bounded, "scalar_bitand": True,
                "scalar_eq": packs, "scalar_lt": four_bits and packs, "scalar_left_shift": packs,
                "left_shift": m * c >= 8, "scalar_mul": four_bits and bounded and packs, C.SUB: four_bits,
                "div_rem": four_bits and packs}
        assert {op for op in C.OPS if rule[op]} == set(C.TABLE[s]), s


def test_case_list_is_complete():
    ids = [c.id for c in C.CASES + C.REFUSED]
    assert len(ids) == len(set(ids))
    for s, (name, nb) in C.SETS.items():
        P = C.params(s)
        assert (P.message_modulus, P.carry_modulus) == C.MODULI[s] and P.name == name and P.lwe_dimension == 8
        mine = [c for c in C.CASES if c.set == s and c.nb == nb]
        assert {c.op for c in mine} >= set(C.TABLE[s])
        assert {c.variant for c in mine} == ({"clean", "dirty", "trivial"} if s in C.FULL else {"clean"})
        assert {c.op for c in C.REFUSED if c.set == s} == set(C.OPS) - set(C.TABLE[s])
        for op in set(C.PER_ROW) & set(C.TABLE[s]):
            assert {c.form for c in mine if c.op == op} == {"int", "rows"}
        if "scalar_left_shift" in C.TABLE[s]:
            T = C.bits(s) * nb
            assert {c.scalar for c in mine if c.op == "scalar_left_shift"} == {0, 1, T - 1}
    extra = {(c.set, c.op, c.nb) for c in C.CASES}
    assert {("3_3", "eq", 9), ("3_3", "ne", 9), ("1_1", "eq", 5), ("1_1", "ne", 5)} <= extra
    assert {(s, C.SUB, nb) for s in ("3_2", "4_2") for nb in (1, 2, 3, 5)} <= extra


def test_crafted_rows():
    for case in C.CASES:
        v, m, M, nb = C.values(case), case.msg, case.M, case.nb
        lhs, rhs, clear = v["lhs"], v["rhs"], v["clear"]
        assert all(0 <= x < M for x in lhs + (rhs or []) + (clear or []))
        if case.variant == "trivial":
            assert all(x % m == 0 for x in lhs), "block 0 of the left operand is a trivial zero"
            continue
        if case.op in C.PER_ROW:
            assert (clear[0], clear[1], clear[2]) == (0, M - 1, lhs[2])
            assert clear[3] != lhs[3] and clear[3] % (M // m) == lhs[3] % (M // m)
            if m >= 8:
                assert clear[2] % (m * m) >= 16
        elif case.op == "left_shift":
            assert rhs[:4] == [0, 1, case.T - 1, M - 1]
        elif case.op == "div_rem":
            assert rhs[0] == 1 and rhs[1] == lhs[1] + 1 and rhs[2] == M - 1 and (lhs[3], rhs[3]) == (M - 1, 0)
        elif case.op not in C.ONE_INT:
            assert lhs[0] == rhs[0]
            assert lhs[1] != rhs[1] and lhs[1] // m == rhs[1] // m
            assert lhs[2] != rhs[2] and (nb == 1 or lhs[2] % (M // m) == rhs[2] % (M // m))
            assert (lhs[3], rhs[3]) == (M - 1, 0)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_case(host_keys, case):
    ck, sks = host_keys(case.set)
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in C.inputs(enc)]
    want = C.expected(case)
    for b in range(C.ROWS // C.K):
        out = [sks.to_host(r) for r in C.run(case, sks, enc, b)]
        assert C.decrypted(ck, case, out) == want[b * C.K:(b + 1) * C.K], b
        assert [r.num_blocks for r in out] == list(C.result_blocks(case)) and all(r.count == C.K for r in out)
        for r, n in zip(out, C.result_blocks(case)):
            if case.op in C.BOOLEAN or (case.op == C.SUB and r is out[1]):
                assert r.degree == [1]
            elif not (case.op == "scalar_left_shift" and case.scalar == 0):    # amount 0: the operand itself
                assert r.block_carries_are_empty(case.msg)
    assert all(np.array_equal(e.data, d) for e, d in zip(C.inputs(enc), before)), "an input batch was written"


class _NoEngine:
    def upload_bootstrap_key(self, bsk):
        pass

    def upload_keyswitch_key(self, ksk):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached on a refused parameter set")


@pytest.mark.parametrize("case", C.REFUSED, ids=lambda c: c.id)
def test_refused_case(case):
    """before the first engine call: the key's engine fails whatever is asked of it"""
    from tfhe_mi355 import integer, shortint

    P = C.params(case.set)
    ck = shortint.ClientKey(P, C.SEED)
    sks = integer.ServerKey(shortint.ServerKey(None, engine=_NoEngine(), parameters=P))
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in C.inputs(enc)]
    lhs, rhs = C.operands(case, sks, enc, 0)
    right = rhs if rhs is not None else C.clear_operand(case, 0)
    with pytest.raises(NotImplementedError, match=f"{C.method(case)}: {C.SETS[case.set][0]} .*is not supported: "):
        C.apply(case, sks, lhs, right)
    assert sks.pbs_count == 0 and sks.launches == 0
    assert np.array_equal(lhs.data, before[0][:C.K]) and (rhs is None or np.array_equal(rhs.data, before[-1][:C.K]))
    assert all(np.array_equal(e.data, d) for e, d in zip(C.inputs(enc), before))


# ---- unsigned_overflowing_sub with carry_modulus < message_modulus ------------------------------------------------
@pytest.mark.parametrize("s", ["3_2", "4_2"])
def test_overflowing_sub_is_served_with_carry_below_msg_at_every_block_count(s):
    from tfhe_mi355 import integer

    m, c = C.MODULI[s]
    assert integer.overflowing_sub_refusal(m, c) is None
    assert integer.div_refusal(m, c) is not None, "the division still refuses: its shift packs two messages"
    assert sorted(case.nb for case in C.CASES if case.set == s and case.op == C.SUB) == [1, 2, 3, 5]


def test_borrow_states_keep_their_bound_through_the_prefix_sum(host_keys):
    """5 blocks at 3_2: three Hillis-Steele steps.  The LUT of a step has degree msg - 1 = 7, and 7 * 8 + 7 does not
    fit a block of 32; the states it makes are 0, 1 or 2, and 2 * 8 + 2 does.  The borrow comes out with degree 1."""
    ck, sks = host_keys("3_2")
    case = next(c for c in C.CASES if c.id == f"3_2-{C.SUB}-clean-b5")
    assert sks.lut_prefix.degree == 7 and sks.msg * sks.carry == 32
    enc = C.encrypt(ck, case)
    diff, borrow = C.run(case, sks, enc, 0)
    assert (sks.pbs_count, sks.launches) == ((5 + 4 + 3 + 1 + 5) * C.K, 5)
    assert borrow.degree == [1] and borrow.num_blocks == 1 and diff.block_carries_are_empty(8)
    assert C.decrypted(ck, case, (diff, borrow)) == C.expected(case)[:C.K]
