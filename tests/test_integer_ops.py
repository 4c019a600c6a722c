"""The radix integer operations beyond the multiply DAG (tfhe_mi355/integer.py: neg, sub, bitwise ops, eq / ne,
order, if_then_else, min / max) on the host path, oracle engine, at lwe_dimension = 8: every row of every case of
integer_ops_cases.py against plain Python integers, pbs_count and launches against the restated loop structure of
the reference, the refusals, the block layer's numpy formula, and a set with carry_modulus < message_modulus."""
import numpy as np
import pytest

import integer_ops_cases as C
from conftest import OracleEngine

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def host_key():
    return C.keys(OracleEngine(C.params(), threads=4))


def test_case_list_is_complete():
    ids = [c.id for c in C.CASES]
    assert len(ids) == len(set(ids)) == len(C.BLOCKS) * (len(C.OPS) * len(C.VARIANTS) - 1)
    assert {c.nb for c in C.CASES} == set(C.BLOCKS) and {c.op for c in C.CASES} == set(C.OPS)
    for nb in C.BLOCKS:
        assert all(0 <= j < nb for j in C.TRIVIAL(nb)) and nb - 1 in C.TRIVIAL(nb)


def test_crafted_rows():
    for case in C.CASES:
        if case.variant == "trivial" or case.op != "lt":
            continue
        v, M = C.values(case), C.MSG ** case.nb
        lhs, rhs = v["lhs"], v["rhs"]
        assert lhs[0] == rhs[0]
        assert lhs[1] != rhs[1] and lhs[1] // C.MSG == rhs[1] // C.MSG
        assert lhs[2] != rhs[2] and lhs[2] % (M // C.MSG) == rhs[2] % (M // C.MSG)
        assert (lhs[3], rhs[3]) == (M - 1, 0)


# (pbs_count, launches) of K = 3 rows worked out by hand from the reference, against the restated loops:
#   lt, 8 blocks: 4 packed chunks, tree 2 + 1, map 1 = 8 LUTs in 1 + 2 + 1 passes (comparator.rs:421-463, 257-280)
#   lt, 5 blocks: 3 chunks (the last unpaired), tree 1 + 1, map 1 = 6 LUTs in 4 passes
#   eq, 8 blocks: 8 bivariate LUTs, one sum of 8 <= 15 blocks = 9 LUTs in 2 passes (comparison.rs:10-33)
#   eq, 1 block: the block comparison is the result
#   if_then_else, 5 blocks: 5 + 5 zero_out LUTs in one pass, 5 message extractions (cmux.rs:194-248)
#   max, 2 blocks: 1 chunk (no tree, no map), then the cmux: 1 + 4 + 2 LUTs in 3 passes (comparator.rs:849-875)
#   sub, 8 blocks: the single-carry propagation of add-b8 (integer_dag_cases.EXPECTED): 8 + (7 + 6 + 4) + 8
#   bitand: one LUT per block
HAND = {"lt-clean-b8": (24, 4), "lt-clean-b5": (18, 4), "eq-clean-b8": (27, 2), "eq-clean-b1": (3, 1),
        "if_then_else-clean-b5": (45, 2), "max-clean-b2": (21, 3), "sub-clean-b8": (99, 5), "bitand-clean-b3": (9, 1),
        "lt-unchecked-b1": (6, 2), "neg-clean-b1": (6, 2)}


def test_restated_loops_give_the_hand_counts():
    by_id = {c.id: c for c in C.CASES}
    assert {cid: C.shadow(by_id[cid]) for cid in HAND} == HAND


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_ops_case(host_key, case):
    ck, sks = host_key
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc["lhs"] + enc["rhs"] + [enc["cond"]]]
    want, nblocks = C.expected(case)
    for b in range(C.ROWS // C.K):
        out = sks.to_host(C.run(case, sks, enc, b))
        assert (sks.pbs_count, sks.launches) == C.shadow(case), (b, sks.pbs_count, sks.launches)
        assert C.decrypt(ck, out, nblocks) == want[b * C.K:(b + 1) * C.K], b
        assert out.num_blocks == nblocks and out.count == C.K
        if case.op in C.BOOLEAN:
            assert out.degree == [1]
        else:
            assert out.block_carries_are_empty(C.MSG)
    assert all(np.array_equal(e.data, d) for e, d in zip(enc["lhs"] + enc["rhs"] + [enc["cond"]], before))


def test_one_dirty_operand(host_key):
    """the (true, false) and (false, true) arms of the default forms' preamble"""
    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == "le-dirty-b3")
    enc = C.encrypt(ck, case)
    want, _ = C.expected(case)
    clean = C.Case("le", "clean", 3, 0)
    for dirty in ("lhs", "rhs"):
        x = {}
        for name in ("lhs", "rhs"):
            parts = [sks.to_device(C.batch_rows(e, 0)) for e in enc[name]]
            for t in parts[1:]:
                sks.unchecked_add_assign(parts[0], t)
            if name != dirty:
                sks.full_propagate(parts[0])
            x[name] = parts[0]
        sks.pbs_count = sks.launches = 0
        out = sks.le_parallelized(x["lhs"], x["rhs"])
        s = C.Shadow()
        C._full_propagate(s, [False] * 3)
        assert (sks.pbs_count, sks.launches) == tuple(a + b for a, b in zip((s.pbs, s.launches), C.shadow(clean)))
        assert C.decrypt(ck, sks.to_host(out), 1) == want[:C.K]
        assert x[dirty].degree == [4 * (C.MSG - 1)] * 3, "the operand itself was propagated, not a clone"


def test_condition_of_degree_zero_decides_on_the_spot(host_key):
    """zero_out_if (cmux.rs:292-299): a condition that can only be 0 zeroes the true operand trivially and leaves the
    false one alone: no PBS before the message extraction"""
    ck, sks = host_key
    case = next(c for c in C.CASES if c.id == "if_then_else-clean-b3")
    enc = C.encrypt(ck, case)
    t, f = (sks.to_device(C.batch_rows(enc[n][0], 0)) for n in ("lhs", "rhs"))
    cond = sks.create_trivial_zero(C.K, 1)
    sks.pbs_count = sks.launches = 0
    out = sks.if_then_else_parallelized(cond, t, f)
    assert (sks.pbs_count, sks.launches) == (3 * C.K, 1)
    assert C.decrypt(ck, sks.to_host(out), 3) == C.values(case)["rhs"][:C.K]


def test_equality_over_more_blocks_than_one_chunk_sums(host_key):
    """17 blocks: the block comparisons are summed in chunks of 15 and 2 (scalar_comparison.rs:164-185), then the
    two chunk results in a second pass: 17 + 2 + 1 LUTs in 3 passes"""
    from tfhe_mi355 import integer

    ck, sks = host_key
    nb = 17
    cks, one = integer.ClientKey(ck, nb), integer.ClientKey(ck, 1)
    lhs = np.array([C.MSG ** nb - 1, 123456789, 3 * C.MSG ** 16 + 5], dtype=np.uint64)
    rhs = np.array([C.MSG ** nb - 1, 123456788, 2 * C.MSG ** 16 + 5], dtype=np.uint64)   # equal, block 0, top block
    x, y = cks.encrypt(lhs), cks.encrypt(rhs)
    for name, want in (("eq", [1, 0, 0]), ("ne", [0, 1, 1])):
        sks.pbs_count = sks.launches = 0
        out = getattr(sks, f"{name}_parallelized")(x, y)
        assert (sks.pbs_count, sks.launches) == ((17 + 2 + 1) * C.K, 3)
        assert [int(v) for v in one.decrypt(out)] == want
        assert out.degree == [1] and out.num_blocks == 1


# ---- the block layer's formula -----------------------------------------------------------------------------------
def test_host_block_layer_is_the_formula():
    from tfhe_mi355.integer import _HostOps

    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 64, (3, 4, 9), dtype=np.uint64)
    y = rng.integers(0, 1 << 64, (3, 5, 9), dtype=np.uint64)
    a0, y0 = a.copy(), y.copy()
    r = [int(x) for x in rng.integers(0, 1 << 64, 4, dtype=np.uint64)]
    _HostOps(None).block_layer([
        (y[:, 0, :], r[0], []),
        (y[:, 1, :], r[1], [(a[:, 0, :], -1)]),
        (y[:, 2, :], 0, [(a[:, 1, :], 4), (a[:, 0, :], 1), (a[:, 3, :], -4), (a[:, 2, :], U64)]),
        (y[:, 3, :], r[2], [(y[:, 3, :], 3), (a[:, 2, :], r[3])]),
        (y[:, 4, :], 0, [(a[:, k % 4, :], 1) for k in range(7)]),
    ])
    assert np.array_equal(a, a0)
    for row in range(3):
        for w in range(9):
            body = w == 8
            A = [int(a0[row, j, w]) for j in range(4)]
            want = [r[0] * body, -A[0] + r[1] * body, 4 * A[1] + A[0] - 4 * A[3] - A[2],
                    3 * int(y0[row, 3, w]) + r[3] * A[2] + r[2] * body, 2 * (A[0] + A[1] + A[2]) + A[3]]
            assert [int(v) for v in y[row, :, w]] == [v & U64 for v in want], (row, w)


# ---- refusals ------------------------------------------------------------------------------------------------------
class _NoEngine:
    def upload_bootstrap_key(self, bsk):
        pass

    def upload_keyswitch_key(self, ksk):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached on a refused parameter set")


# set -> (propagation, bivariate layers, comparisons) refused; the rule: propagation_refusal of integer.py (pinned in
# test_integer_dag.py), carry_modulus < message_modulus, message_modulus * carry_modulus < 16
RULE = {
    "PARAM_MESSAGE_2_CARRY_2_KS_PBS": (False, False, False),
    "PARAM_MESSAGE_1_CARRY_1_KS_PBS": (True, False, True),
    "PARAM_MESSAGE_2_CARRY_1_KS_PBS": (True, True, True),
    "PARAM_MESSAGE_2_CARRY_3_KS_PBS": (True, False, False),
    "PARAM_MESSAGE_3_CARRY_1_KS_PBS": (True, True, False),
    "PARAM_MESSAGE_3_CARRY_2_KS_PBS": (False, True, False),
    "PARAM_MESSAGE_4_CARRY_4_KS_PBS": (False, False, False),
}
# operation -> which of the three it needs on operands with empty carries
NEEDS = {"neg_parallelized": (0,), "sub_parallelized": (0,), "sub_assign_parallelized": (0,),
         "bitand_parallelized": (1,), "bitor_parallelized": (1,), "bitxor_parallelized": (1,),
         "unchecked_bitand_assign_parallelized": (1,), "unchecked_bitor_assign_parallelized": (1,),
         "unchecked_bitxor_assign_parallelized": (1,),
         "eq_parallelized": (1,), "ne_parallelized": (1,), "unchecked_eq_parallelized": (1,),
         "unchecked_ne_parallelized": (1,), "if_then_else_parallelized": (1,),
         "unchecked_if_then_else_parallelized": (1,),
         "gt_parallelized": (2,), "ge_parallelized": (2,), "lt_parallelized": (2,), "le_parallelized": (2,),
         "unchecked_gt_parallelized": (2,), "unchecked_ge_parallelized": (2,), "unchecked_lt_parallelized": (2,),
         "unchecked_le_parallelized": (2,),
         "max_parallelized": (1, 2), "min_parallelized": (1, 2), "unchecked_max_parallelized": (1, 2),
         "unchecked_min_parallelized": (1, 2)}


@pytest.mark.parametrize("name", list(RULE))
def test_every_operation_refuses_by_the_rule_before_the_first_launch(name):
    from tfhe_mi355 import integer, shortint
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[name]
    sks = integer.ServerKey(shortint.ServerKey(None, engine=_NoEngine(), parameters=P))
    refused = RULE[name]
    assert (sks.propagation_refusal is not None, sks.bivariate_refusal is not None,
            sks.comparison_refusal is not None) == refused
    sks.lwe_size = 3
    x, y, cond = sks.create_trivial_zero(2, 3), sks.create_trivial_zero(2, 3), sks.create_trivial_zero(2, 1)
    x.degree = y.degree = [P.message_modulus - 1] * 3
    x.noise = y.noise = [1] * 3
    cond.degree, cond.noise = [1], [1]
    dirty = sks.create_trivial_zero(2, 3)
    dirty.degree, dirty.noise = [2 * P.message_modulus - 2] * 3, [2] * 3
    for op, needs in NEEDS.items():
        args = (cond, x, y) if "if_then_else" in op else (x,) if op == "neg_parallelized" else (x, y)
        if any(refused[i] for i in needs):
            with pytest.raises(NotImplementedError, match=f"{op}: {name} .*is not supported: "):
                getattr(sks, op)(*args)
        elif refused[0] and not op.startswith("unchecked"):    # served on clean operands, but it cannot propagate
            args = tuple(dirty if a is x else a for a in args)
            with pytest.raises(NotImplementedError, match=f"full_propagate: {name} .*is not supported: "):
                getattr(sks, op)(*args)
    assert sks.pbs_count == 0 and sks.launches == 0
    assert not x.data.any() and not y.data.any() and not dirty.data.any()


# ---- carry_modulus < message_modulus: the comparison block by block -----------------------------------------------
def test_set_3_2_compares_block_by_block_and_refuses_the_bivariate_layers():
    """PARAM_MESSAGE_3_CARRY_2 (message modulus 8, carry modulus 4): Comparator::unchecked_compare_parallelized
    takes its unpacked branch (comparator.rs:399-419) and sub propagates; the cmux's zero_out_if, like the bitwise
    ops, packs block * message_modulus + condition, which does not fit: refused, as for the multiply."""
    from tfhe_mi355 import integer
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[C.SET_3_2].with_(lwe_dimension=8)
    ck, sks = C.keys(OracleEngine(P, threads=4), parameters=P)
    nb, m = C.BLOCKS_3_2, P.message_modulus
    M = m ** nb
    cks = integer.ClientKey(ck, nb)
    rng = np.random.default_rng(3)
    lhs = [int(v) for v in rng.integers(0, M, C.K)] + [M - 1, 5 * m + 2, 77]
    rhs = [lhs[0], lhs[1] ^ 1, lhs[2] ^ (m // 2 * m ** (nb - 1)), 0, 5 * m + 3, 76]
    for b in range(2):
        rows = slice(b * C.K, (b + 1) * C.K)
        x = cks.encrypt(np.asarray(lhs[rows], dtype=np.uint64))
        y = cks.encrypt(np.asarray(rhs[rows], dtype=np.uint64))
        x0, y0 = x.data.copy(), y.data.copy()
        sks.pbs_count = sks.launches = 0
        out = sks.lt_parallelized(x, y)
        assert (sks.pbs_count, sks.launches) == C.shadow_3_2_lt(nb) == (6 * C.K, 4)
        assert [int(v) for v in integer.ClientKey(ck, 1).decrypt(out)] == [int(a < c) for a, c in zip(lhs[rows], rhs[rows])]
        diff = sks.sub_parallelized(x, y)
        assert [int(v) for v in cks.decrypt(diff)] == [(a - c) % M for a, c in zip(lhs[rows], rhs[rows])]
        assert np.array_equal(x.data, x0) and np.array_equal(y.data, y0)
        count = sks.pbs_count
        for call in (lambda: sks.if_then_else_parallelized(out, x, y), lambda: sks.bitand_parallelized(x, y),
                     lambda: sks.max_parallelized(x, y), lambda: sks.eq_parallelized(x, y)):
            with pytest.raises(NotImplementedError, match="carry_modulus < message_modulus"):
                call()
        assert sks.pbs_count == count
