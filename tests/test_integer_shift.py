"""The radix shifts and rotations by a clear and by an encrypted amount and scalar_mul (tfhe_mi355/integer.py) on the
host path, oracle engine, at lwe_dimension = 8: every row of every case of integer_shift_cases.py against plain
Python integers, pbs_count and launches against the restated loop structure of the reference, the refusals, the LUT
cache, and a set with carry_modulus < message_modulus, where the barrel shifter runs and the scalar shifts do not."""
import numpy as np
import pytest

import integer_dag_cases as D
import integer_shift_cases as C
from conftest import OracleEngine


@pytest.fixture(scope="module")
def host_key():
    return C.keys(OracleEngine(C.params(), threads=4))


def test_case_list_is_complete():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids)) == sum(len(C.SCALAR_OPS) * len(C.AMOUNTS(nb)) * 4 + len(C.ENCRYPTED_OPS) * 5 +
                                            len(C.MULTIPLIERS(nb)) * 4 for nb in C.BLOCKS)
    assert all(len(C.AMOUNTS(nb)) == 6 and len(C.MULTIPLIERS(nb)) == 9 for nb in C.BLOCKS if nb > 2)
    assert [C.total_bits(nb) for nb in C.BLOCKS] == [2, 4, 6, 10, 16]
    assert [C.control_bits(nb) for nb in C.BLOCKS] == [1, 2, 3, 4, 4]
    for nb in C.BLOCKS:
        T, s = C.total_bits(nb), C.control_bits(nb)
        assert set(C.AMOUNTS(nb)) == {0, 1, 2, 3, T - 1, T + 3}
        assert set(C.MULTIPLIERS(nb)) == {0, 1, 4, 3, 5, 10, 2 ** T - 1, 2 ** T + 3, 2 ** T}
        rows = C.amount_rows(nb, 0)
        crafted = {a for a in (0, 1, T - 1, T, 2 ** s - 1)}
        assert crafted <= set(rows[:len(crafted)]) and len(rows) - len(crafted) >= 2 and len(rows) % C.K == 0
        assert all(0 <= a < 2 ** T for a in rows)


def test_plain_semantics():
    assert C.plain("scalar_left_shift", 0b1011, 5, 2) == 0b0110          # 5 mod 4 = 1
    assert C.plain("scalar_rotate_right", 0b1011, 1, 2) == 0b1101
    assert C.plain("left_shift", 0b101101, 6, 3) == 0                    # 6 mod 8 = 6 >= T
    assert C.plain("right_shift", 0b101101, 9, 3) == 0b10110             # 9 mod 8 = 1
    assert C.plain("rotate_left", 0b100001, 7, 3) == 0b000011            # (7 mod 8) mod 6 = 1
    assert C.plain("rotate_right", 0b100001, 6, 3) == 0b100001
    assert C.plain("left_shift", 0b0110, 4, 2) == 0b0110                 # T a power of two: 4 mod 4 = 0
    assert C.plain("scalar_mul", 13, 2 ** 4 + 3, 2) == (13 * 3) % 16


# (pbs_count, launches) of K = 3 rows worked out by hand from the reference, against the restated loops.
#   scalar_left_shift b8 by 5: 2 rotations, 1 inside: the end block and 5 windows of the 6 blocks left = 6 LUTs, 1 pass
#   scalar_left_shift b8 by 4: a pure block move;  by 19 = 3 mod 16: 1 rotation, 7 LUTs
#   scalar_right_shift b5 by 3: 1 rotation: 3 windows of 4 blocks and the end block;  rotations: one LUT per block
#   encrypted, T bits, s control bits: T + s extractions joined in one pass, s passes of T muxes, nb recompositions:
#     b8: 16 + 4 + 4 * 16 + 8 = 92 in 6;  b3: 6 + 3 + 3 * 6 + 3 = 30 in 5;  b1: 2 + 1 + 2 + 1 = 6 in 3;
#     b5: 10 + 4 + 40 + 5 = 59 in 6
#   scalar_mul by 4: a left shift by 2, a pure block move.
#   scalar_mul by 5 = 0b101: both set bits at even positions, has_at_least_one_set = [true, false]
#     (scalar_mul.rs:362-367), so preshifted_lhs is the operand and a trivial zero and NO preshift pass is made
#     (the shift by 0 returns at scalar_shift.rs:578-580; it is 10 that makes exactly one pass).  Two terms, the
#     operand and its blockshift by 1: unchecked_sum_ciphertexts_vec takes its len == 2 arm (add.rs:797-801),
#     add_assign_parallelized = the single-carry propagation of add-b8 (integer_dag_cases.EXPECTED): (99, 5).
#   scalar_mul by 10 = 0b1010, the mirror: one preshift pass, the shift by 1 inside the blocks, 8 LUTs; then the
#     same two-term sum: (24 + 99, 1 + 5).
#   scalar_mul by 3 on b2: one preshift pass of 2 LUTs, two terms at block shift 0: 2 + add-b2 (15, 3) = (21, 4).
HAND = {("scalar_left_shift", 8, 5): (18, 1), ("scalar_left_shift", 8, 4): (0, 0), ("scalar_left_shift", 8, 19): (21, 1),
        ("scalar_right_shift", 5, 3): (12, 1), ("scalar_rotate_left", 3, 1): (9, 1), ("scalar_rotate_right", 1, 1): (3, 1),
        ("left_shift", 8, -1): (276, 6), ("left_shift", 3, -1): (90, 5), ("left_shift", 1, -1): (18, 3),
        ("rotate_right", 5, -1): (177, 6),
        ("scalar_mul", 8, 4): (0, 0), ("scalar_mul", 8, 5): (99, 5), ("scalar_mul", 8, 10): (123, 6),
        ("scalar_mul", 2, 3): (21, 4), ("scalar_mul", 5, 0): (0, 0), ("scalar_mul", 5, 1): (0, 0),
        ("scalar_mul", 2, 16): (0, 0)}


def test_restated_loops_give_the_hand_counts():
    """(operation, blocks, clear operand) on clean operands"""
    assert {k: C.shadow(C.Case(k[0], "clean", k[1], k[2], 0)) for k in HAND} == HAND
    assert D.EXPECTED["add-b8"] == (99, 5) and D.EXPECTED["add-b2"] == (15, 3)


def test_restated_sum_gives_the_recorded_counts_of_the_dag_cases():
    """the chunked sum as integer_shift_cases restates it, on the term shapes of integer_dag_cases' sum cases, whose
    counts that file pins: scalar_mul's counts rest on it"""
    for nb in D.BLOCKS:
        for nterms in (1, 2, 3, 2 * D.FILL + 1):
            assert C.shadow_of_dag_sum(nb, nterms) == D.EXPECTED[f"sum{nterms}-b{nb}"], (nb, nterms)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_shift_case(host_key, case):
    ck, sks = host_key
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc["lhs"] + enc["rhs"]]
    want = C.expected(case)
    for b in range(case.rows // C.K):
        res, lhs, rhs = C.run(case, sks, enc, b)
        out = sks.to_host(res)
        assert (sks.pbs_count, sks.launches) == C.shadow(case), (b, sks.pbs_count, sks.launches)
        assert C.decrypt(ck, out, case.nb) == want[b * C.K:(b + 1) * C.K], b
        assert out.num_blocks == case.nb and out.count == C.K
        assert out.block_carries_are_empty(C.MSG)
        lhs0, rhs0 = C.operands(case, sks, enc, b)    # the operands as they were handed in
        if b == 0:                                    # the returning form: a dirty operand is propagated on a clone
            assert np.array_equal(lhs.data, lhs0.data) and lhs.degree == lhs0.degree
        if rhs is not None:                           # the amount is never assigned
            assert np.array_equal(rhs.data, rhs0.data) and rhs.degree == rhs0.degree
    assert all(np.array_equal(e.data, d) for e, d in zip(enc["lhs"] + enc["rhs"], before))


def test_returning_forms_leave_the_operand_untouched(host_key):
    ck, sks = host_key
    for cid in ("scalar_rotate_left-clean-b3-by3", "left_shift-clean-b2", "scalar_mul-clean-b3-by3",
                "scalar_left_shift-clean-b3-by2"):
        case = next(c for c in C.CASES if c.id == cid)
        enc = C.encrypt(ck, case)
        lhs, rhs = C.operands(case, sks, enc, 0)
        keep = lhs.clone()
        second = rhs if rhs is not None else case.clear
        res = getattr(sks, C.method(case, False))(lhs, second)
        assert res is not lhs and res.data is not lhs.data
        assert np.array_equal(lhs.data, keep.data) and lhs.degree == keep.degree and lhs.noise == keep.noise


def test_one_dirty_operand_of_an_encrypted_shift(host_key):
    """the (true, false) and (false, true) arms of the default form (shift.rs:228-250): one full_propagate more
    than the clean case, on a clone of the amount and on the value itself in the assign form"""
    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == "right_shift-dirty-b2")
    clean = next(c for c in C.CASES if c.id == "right_shift-clean-b2")
    enc, want = C.encrypt(ck, case), C.expected(case)
    s = C.Shadow()
    C._full_propagate(s, [False] * 2)
    for dirty in (0, 1):
        x = list(C.operands(case, sks, enc, 0))
        sks.full_propagate(x[1 - dirty])
        sks.pbs_count = sks.launches = 0
        sks.right_shift_assign_parallelized(x[0], x[1])
        assert (sks.pbs_count, sks.launches) == tuple(a + b for a, b in zip((s.pbs, s.launches), C.shadow(clean)))
        assert C.decrypt(ck, sks.to_host(x[0]), 2) == want[:C.K]
        if dirty == 1:
            assert x[1].degree == [C.ADDENDS * (C.MSG - 1)] * 2, "the amount itself was propagated, not a clone"


def test_lut_cache_does_not_grow_on_a_repeated_call(host_key):
    ck, sks = host_key
    for cid in ("scalar_right_shift-clean-b3-by3", "rotate_left-clean-b2", "scalar_mul-clean-b2-by3"):
        case = next(c for c in C.CASES if c.id == cid)
        enc = C.encrypt(ck, case)
        first, _, _ = C.run(case, sks, enc, 0)
        luts = dict(sks._luts)
        again, _, _ = C.run(case, sks, enc, 0)
        assert sks._luts.keys() == luts.keys() and all(sks._luts[k] is v for k, v in luts.items())
        assert np.array_equal(first.data, again.data)
    assert ("left_shift", 1) in sks._luts and ("right_shift", 1) in sks._luts      # keyed by (operation, within)


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
    scalar, encrypted = [], []
    for op in C.ENCRYPTED_OPS:
        for unchecked in ("unchecked_", ""):
            for assign in ("_assign", ""):
                scalar.append(f"{unchecked}scalar_{op}{assign}_parallelized")
                encrypted.append(f"{unchecked}{op}{assign}_parallelized")
    mul = [f"{u}scalar_mul{a}_parallelized" for u in ("unchecked_", "") for a in ("_assign", "")]
    return scalar, encrypted, mul


def test_every_form_exists():
    from tfhe_mi355 import integer

    scalar, encrypted, mul = _all_methods()
    assert len(scalar) == len(encrypted) == 16
    for name in scalar + encrypted + mul:
        assert callable(getattr(integer.ServerKey, name)), name


def test_barrel_shifter_refusal_over_every_set():
    """shift.rs:334-337: log2(message_modulus) + log2(carry_modulus) >= 3"""
    from tfhe_mi355.integer import barrel_shifter_refusal
    from tfhe_mi355.parameters import SHORTINT_ALL

    sets = {n: P for n, P in SHORTINT_ALL.items() if n.endswith("_KS_PBS")}
    assert len(sets) >= 7
    refused = set()
    for name, P in sets.items():
        few = int(np.log2(P.message_modulus)) + int(np.log2(P.carry_modulus)) < 3
        assert (barrel_shifter_refusal(P.message_modulus, P.carry_modulus) is not None) == few, name
        if few:
            refused.add(name)
    assert "PARAM_MESSAGE_1_CARRY_1_KS_PBS" in refused and "PARAM_MESSAGE_2_CARRY_1_KS_PBS" not in refused
    assert barrel_shifter_refusal(2, 2) and barrel_shifter_refusal(2, 4) is None and barrel_shifter_refusal(4, 2) is None


def test_clear_operands_and_block_counts_are_checked_before_the_first_launch():
    P, sks = _inert_key("PARAM_MESSAGE_2_CARRY_2_KS_PBS")
    x, y, short = _inert_operand(sks, P, 3), _inert_operand(sks, P, 3), _inert_operand(sks, P, 2)
    dirty = _inert_operand(sks, P, 3, degree=6, noise=2)
    scalar, encrypted, mul = _all_methods()
    for name in scalar + mul:
        with pytest.raises(ValueError, match=f"{name}: the clear operand must not be negative"):
            getattr(sks, name)(x, -1)
        with pytest.raises(ValueError, match="must not be negative"):
            getattr(sks, name)(dirty, -3)
        with pytest.raises(TypeError, match="one Python int for the whole batch"):
            getattr(sks, name)(x, [1, 2])
    for name in encrypted:
        for a, b in ((x, short), (short, x), (dirty, short)):
            with pytest.raises(ValueError, match=f"{name}: the value has {a.num_blocks} blocks and the amount {b.num_blocks}"):
                getattr(sks, name)(a, b)
    assert sks.pbs_count == 0 and sks.launches == 0
    assert not x.data.any() and not y.data.any() and not dirty.data.any() and not short.data.any()


# set -> (propagation, bivariate layers, barrel shifter) refused
RULE = {
    "PARAM_MESSAGE_2_CARRY_2_KS_PBS": (False, False, False),
    "PARAM_MESSAGE_1_CARRY_1_KS_PBS": (True, False, True),
    "PARAM_MESSAGE_2_CARRY_1_KS_PBS": (True, True, False),
    "PARAM_MESSAGE_2_CARRY_3_KS_PBS": (True, False, False),
    "PARAM_MESSAGE_3_CARRY_1_KS_PBS": (True, True, False),
    "PARAM_MESSAGE_3_CARRY_2_KS_PBS": (False, True, False),
    "PARAM_MESSAGE_4_CARRY_4_KS_PBS": (False, False, False),
}


@pytest.mark.parametrize("name", list(RULE))
def test_every_form_refuses_by_the_rule_before_the_first_launch(name):
    P, sks = _inert_key(name)
    refused = RULE[name]
    assert (sks.propagation_refusal is not None, sks.bivariate_refusal is not None,
            sks.barrel_shifter_refusal is not None) == refused
    x, y = _inert_operand(sks, P, 3), _inert_operand(sks, P, 3)
    dirty = _inert_operand(sks, P, 3, degree=2 * P.message_modulus - 2, noise=2)
    scalar, encrypted, mul = _all_methods()
    for op in scalar:
        if refused[1]:
            for v in (x, dirty):
                with pytest.raises(NotImplementedError, match=f"{op}: {name} .*carry_modulus < message_modulus"):
                    getattr(sks, op)(v, 1)
        elif refused[0] and not op.startswith("unchecked"):
            with pytest.raises(NotImplementedError, match=f"full_propagate: {name} .*is not supported: "):
                getattr(sks, op)(dirty, 1)
    for op in encrypted:
        if refused[2]:
            for v in (x, dirty):
                with pytest.raises(NotImplementedError, match=f"{op}: {name} .*fewer than 3 bits"):
                    getattr(sks, op)(v, y)
        elif refused[0] and not op.startswith("unchecked"):
            for a, b in ((dirty, y), (x, dirty)):
                with pytest.raises(NotImplementedError, match=f"full_propagate: {name} .*is not supported: "):
                    getattr(sks, op)(a, b)
    for op in mul:
        for v in (x, dirty):
            if refused[1]:
                for scalar_value in (4, 3):
                    with pytest.raises(NotImplementedError, match=f"{op}: {name} .*carry_modulus < message_modulus"):
                        getattr(sks, op)(v, scalar_value)
            elif refused[0]:
                with pytest.raises(NotImplementedError, match=f"{name} .*is not supported: "):
                    getattr(sks, op)(v, 3)
    assert sks.pbs_count == 0 and sks.launches == 0
    assert not x.data.any() and not y.data.any() and not dirty.data.any()


# ---- carry_modulus < message_modulus: the barrel shifter runs, the scalar shifts are refused ------------------------
def test_set_3_2_runs_the_encrypted_shifts_and_refuses_the_scalar_ones():
    """PARAM_MESSAGE_3_CARRY_2 (message modulus 8, carry modulus 4, 3 bits per block): the barrel shifter needs 3
    bits of a block and packs nothing wider (shift.rs:334-337), so it runs; the scalar shifts pack two messages
    for their bivariate LUT, which does not fit.  As in the reference."""
    from tfhe_mi355 import integer
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[C.SET_3_2].with_(lwe_dimension=8)
    ck, sks = C.keys(OracleEngine(P, threads=4), parameters=P)
    nb, bits = C.BLOCKS_3_2, 3
    T, s = bits * nb, 3
    M = 2 ** T
    cks = integer.ClientKey(ck, nb)
    values = [M - 1, 0b100001, 0b010110]
    amounts = [1, T - 1, 2 ** s - 1]
    x = cks.encrypt(np.asarray(values, dtype=np.uint64))
    y = cks.encrypt(np.asarray(amounts, dtype=np.uint64))
    x0, y0 = x.data.copy(), y.data.copy()
    want = {"left_shift": [(v << a) % M for v, a in zip(values, amounts)],
            "rotate_right": [((v >> a % T) | (v << (T - a % T))) % M for v, a in zip(values, amounts)]}
    for op in ("left_shift", "rotate_right"):
        sks.pbs_count = sks.launches = 0
        out = getattr(sks, f"{op}_parallelized")(x, y)
        assert (sks.pbs_count, sks.launches) == ((T + s + s * T + nb) * C.K, s + 2) == (29 * C.K, 5)
        assert [int(v) for v in cks.decrypt(out)] == want[op]
        assert out.block_carries_are_empty(P.message_modulus)
    assert np.array_equal(x.data, x0) and np.array_equal(y.data, y0)
    count = sks.pbs_count
    for call in (lambda: sks.scalar_left_shift_parallelized(x, 1), lambda: sks.unchecked_scalar_rotate_right_parallelized(x, 4),
                 lambda: sks.scalar_mul_parallelized(x, 4), lambda: sks.scalar_mul_parallelized(x, 3)):
        with pytest.raises(NotImplementedError, match="carry_modulus < message_modulus"):
            call()
    assert sks.pbs_count == count
