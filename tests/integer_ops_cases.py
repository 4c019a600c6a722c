"""Case list of the radix integer operations beyond the multiply DAG (neg, sub, bitwise ops, eq / ne, order,
if_then_else, min / max), shared by test_integer_ops.py (host path, oracle engine) and test_integer_ops_gpu.py
(device path against the host path).

Conventions of integer_dag_cases.py: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8, batches of K = 3
operand rows, blocks (1, 2, 3, 5, 8): odd counts leave the last chunk of a packed comparison unpaired, 8 blocks
give 4 chunks and, with the final map, a three-level sign tree.  A case has ROWS = 6 operand rows, run as two
batches of K: rows 0 .. 3 are crafted (equal operands; operands differing only in block 0; only in the top block;
all-ones against zero), rows 4 and 5 are random.

A case is (operation, variant, blocks):
  unchecked  clean operands through the unchecked_* form (neg and sub: followed by full_propagate, so the result
             decrypts digit by digit);
  clean      clean operands through the default form;
  dirty      every radix operand is the sum of four encryptions (three unchecked adds first, degree 12): the
             default form propagates both before it starts;
  trivial    blocks TRIVIAL(nb) of both radix operands are trivial ciphertexts (the top chunk entirely, one block
             of a lower chunk; one of them of degree 0): requests whose sources are all trivial take the trivial
             PBS and are not counted.

Expected pbs_count and launches come from `shadow` below, which restates the loop structure of the reference
functions on one flag per block (trivial or not): how many LUT applications each parallel pass makes, and which
of them meet only trivial inputs.  Nothing here is recorded from the code under test.
"""
from dataclasses import dataclass

import numpy as np

from integer_dag_cases import K, MSG, SEED, keys, params  # noqa: F401  (the same key conventions)

BLOCKS = (1, 2, 3, 5, 8)
ROWS = 2 * K
CARRY = 4
MAX_VALUE = MSG * CARRY - 1      # blocks summed per chunk by eq / ne (scalar_comparison.rs:155-158)

BITOPS = {"bitand": lambda a, b: a & b, "bitor": lambda a, b: a | b, "bitxor": lambda a, b: a ^ b}
ORDER = {"gt": lambda a, b: a > b, "ge": lambda a, b: a >= b, "lt": lambda a, b: a < b, "le": lambda a, b: a <= b}
OPS = ("neg", "sub", "bitand", "bitor", "bitxor", "bitnot", "eq", "ne", "gt", "ge", "lt", "le", "max", "min",
       "if_then_else")
UNARY = ("neg", "bitnot")
BOOLEAN = ("eq", "ne", "gt", "ge", "lt", "le")
VARIANTS = ("unchecked", "clean", "dirty", "trivial")
ADDENDS = 4                      # a dirty operand: three unchecked adds, degree 4 * (MSG - 1) = 12


@dataclass(frozen=True)
class Case:
    op: str
    variant: str
    nb: int
    seed: int

    @property
    def id(self):
        return f"{self.op}-{self.variant}-b{self.nb}"


def _cases():
    out, seed = [], 500
    for nb in BLOCKS:
        for op in OPS:
            for variant in VARIANTS:
                if op == "bitnot" and variant == "unchecked":
                    continue                 # the reference has no unchecked bitnot
                out.append(Case(op, variant, nb, seed))
                seed += 1
    return out


CASES = _cases()


# ---- plaintext side ---------------------------------------------------------------------------------------------
def TRIVIAL(nb):
    """blocks made trivial in both operands: the whole top chunk of the packed comparison, and block nb // 4 (a
    lower chunk's, where there is one)"""
    return sorted(set(range(2 * ((nb - 1) // 2), nb)) | {nb // 4})


def trivial_digit(nb, j, operand):
    """the digit a trivial block holds, the same in every row: 0 (degree 0) at block nb // 4 of the left operand"""
    if operand == 0:
        return 0 if j == nb // 4 else 1 + j % 3
    return 1 + (j + 1) % 3


def _set_digit(v, j, d):
    return v - ((v // MSG ** j) % MSG) * MSG ** j + d * MSG ** j


def values(case):
    """{"lhs": [ROWS], "rhs": [ROWS], "cond": [ROWS]} as Python ints, the trivial digits already in place"""
    nb, M = case.nb, MSG ** case.nb
    rng = np.random.default_rng(case.seed)
    lhs = [int(x) for x in rng.integers(0, M, ROWS)]
    rhs = [int(x) for x in rng.integers(0, M, ROWS)]
    rhs[0] = lhs[0]                                                         # equal
    rhs[1] = _set_digit(lhs[1], 0, (lhs[1] % MSG + 1) % MSG)                # differ only in block 0
    top = (lhs[2] // MSG ** (nb - 1)) % MSG
    rhs[2] = _set_digit(lhs[2], nb - 1, (top + 2) % MSG)                    # differ only in the top block
    lhs[3], rhs[3] = M - 1, 0                                               # all-ones against zero
    if case.variant == "trivial":
        for j in TRIVIAL(nb):
            lhs = [_set_digit(v, j, trivial_digit(nb, j, 0)) for v in lhs]
            rhs = [_set_digit(v, j, trivial_digit(nb, j, 1)) for v in rhs]
    return {"lhs": lhs, "rhs": rhs, "cond": [1, 0, 0, 1, 1, 0]}


def expected(case):
    """([ROWS] Python ints, blocks of the result)"""
    v, M, op = values(case), MSG ** case.nb, case.op
    out = []
    for a, b, c in zip(v["lhs"], v["rhs"], v["cond"]):
        if op == "neg":
            e = -a % M
        elif op == "sub":
            e = (a - b) % M
        elif op in BITOPS:
            e = BITOPS[op](a, b)
        elif op == "bitnot":
            e = M - 1 - a
        elif op == "eq":
            e = int(a == b)
        elif op == "ne":
            e = int(a != b)
        elif op in ORDER:
            e = int(ORDER[op](a, b))
        elif op == "max":
            e = max(a, b)
        elif op == "min":
            e = min(a, b)
        else:
            e = a if c else b
        out.append(e)
    return out, (1 if op in BOOLEAN else case.nb)


# ---- ciphertext side --------------------------------------------------------------------------------------------
def encrypt(ck, case):
    """Host batches of ROWS rows: {"lhs": [batches to add up], "rhs": [...], "cond": batch}; a clean operand is
    one batch, a dirty one ADDENDS batches whose plaintexts add up to the operand modulo MSG ** nb.  The
    encryption randomness depends on the case alone."""
    from tfhe_mi355 import integer

    ck._enc_counter = case.seed << 8
    cks, M = integer.ClientKey(ck, case.nb), MSG ** case.nb
    v = values(case)
    rng = np.random.default_rng(case.seed + 7)
    enc = {}
    for name in ("lhs", "rhs"):
        parts = [np.asarray(v[name], dtype=np.uint64)]
        if case.variant == "dirty":
            extra = rng.integers(0, M, (ADDENDS - 1, ROWS), dtype=np.uint64)
            parts = [(parts[0] + np.uint64(ADDENDS - 1) * np.uint64(M) - extra.sum(axis=0)) % np.uint64(M)] + list(extra)
        enc[name] = [cks.encrypt(p) for p in parts]
    cond = integer.ClientKey(ck, 1).encrypt(np.asarray(v["cond"], dtype=np.uint64))
    cond.degree = [1]                       # a BooleanBlock: the block holds 0 or 1
    enc["cond"] = cond
    return enc


def batch_rows(rb, b):
    """rows [b K, (b + 1) K) of a host batch, as a batch of its own"""
    from tfhe_mi355.integer import RadixBatch

    return RadixBatch(rb.data[b * K:(b + 1) * K].copy(), list(rb.degree), list(rb.noise))


def decrypt(ck, rb, nblocks):
    from tfhe_mi355 import integer

    return [int(x) for x in integer.ClientKey(ck, nblocks).decrypt(rb)]


def run(case, sks, enc, b):
    """The case on rows [b K, (b + 1) K) on `sks` (host or device path); the host batches of `enc` stay
    untouched.  Returns the result in the key's residency; sks.pbs_count and sks.launches count the case alone."""
    def operand(name, index):
        x = [sks.to_device(batch_rows(e, b)) for e in enc[name]]
        for t in x[1:]:
            sks.unchecked_add_assign(x[0], t)
        if case.variant == "trivial":
            for j in TRIVIAL(case.nb):
                sks._set_trivial(x[0], j, trivial_digit(case.nb, j, index))
        return x[0]

    lhs, rhs = operand("lhs", 0), operand("rhs", 1)
    cond = sks.to_device(batch_rows(enc["cond"], b))
    sks.pbs_count = sks.launches = 0
    op, unchecked = case.op, case.variant == "unchecked"
    if op == "neg":
        if unchecked:
            res = sks.unchecked_neg(lhs)
            sks.full_propagate(res)
            return res
        return sks.neg_parallelized(lhs)
    if op == "sub":
        if unchecked:
            sks.unchecked_sub_assign(lhs, rhs)
            sks.full_propagate(lhs)
            return lhs
        return sks.sub_parallelized(lhs, rhs)
    if op == "bitnot":
        return sks.bitnot_parallelized(lhs)
    if op in BITOPS and unchecked:
        getattr(sks, f"unchecked_{op}_assign_parallelized")(lhs, rhs)
        return lhs
    if op == "if_then_else":
        f = sks.unchecked_if_then_else_parallelized if unchecked else sks.if_then_else_parallelized
        return f(cond, lhs, rhs)
    return getattr(sks, f"unchecked_{op}_parallelized" if unchecked else f"{op}_parallelized")(lhs, rhs)


# ---- the expected counts: the reference's loops on one flag per block ---------------------------------------------
class Shadow:
    """pbs_count and launches of K rows.  A block is True where it is a trivial ciphertext; a LUT application
    whose inputs are all trivial is a trivial PBS (shortint/server_key/mod.rs:763-781), not a bootstrap."""

    def __init__(self):
        self.pbs = self.launches = 0

    def layer(self, requests):
        """one parallel pass of LUT applications (a par_iter / rayon::join of the reference): one batched launch
        over the requests that are not trivial"""
        n = sum(1 for trivial in requests if not trivial)
        if n:
            self.pbs += n * K
            self.launches += 1


def _single_carry(s, ct):
    """propagate_single_carry_parallelized_low_latency (add.rs:518-603)"""
    nb = len(ct)
    gp = list(ct)
    s.layer(gp)                                       # generate_init_carry_array: every block
    space = 1
    for _ in range((nb - 1).bit_length() if nb > 1 else 0):   # compute_prefix_sum_hillis_steele
        new = list(gp)
        for b in range(space, nb):
            new[b] = gp[b] and gp[b - space]
        s.layer(new[space:])
        gp, space = new, space * 2
    carries = [True] + gp[:-1]                        # the last carry swapped for a trivial zero, rotate_right(1)
    out = [a and c for a, c in zip(ct, carries)]
    s.layer(out)                                      # message extraction of every block
    return out


def _full_propagate(s, ct):
    """full_propagate_parallelized (radix_parallel/mod.rs:88-155)"""
    s.layer(ct + ct[:-1])                             # messages of all blocks, carries of all but the last
    carries = [True] + ct[:-1]
    return _single_carry(s, [a and c for a, c in zip(ct, carries)])


def _compare(s, lhs, rhs, packed=True):
    """Comparator::unchecked_compare_parallelized (comparator.rs:389-463): with carry >= msg chunks of two blocks
    are packed (:421-441), else every block is a chunk (:399-419); one sign per chunk, then
    reduce_signs_parallelized (:257-280) pairs them until one is left"""
    both = [a and b for a, b in zip(lhs, rhs)]
    signs = [all(both[j:j + 2]) for j in range(0, len(both), 2)] if packed else both
    s.layer(signs)
    while len(signs) != 1:
        pairs = [signs[2 * c] and signs[2 * c + 1] for c in range(len(signs) // 2)]
        s.layer(pairs)
        signs = pairs + (signs[-1:] if len(signs) % 2 else [])
    return signs[0]


def _cmux(s, cond, t, f, t_zero, f_zero):
    """unchecked_programmable_if_then_else_parallelized (cmux.rs:194-248): both zero_out_if (:281-316, blocks of
    degree 0 skipped) joined in one pass, then add + message_extract of every block"""
    s.layer([x and cond for x, z in zip(t, t_zero) if not z] + [x and cond for x, z in zip(f, f_zero) if not z])
    t = [x if z else x and cond for x, z in zip(t, t_zero)]
    f = [x if z else x and cond for x, z in zip(f, f_zero)]
    s.layer([a and b for a, b in zip(t, f)])


def shadow(case):
    """(pbs_count, launches) of one batch of K rows"""
    nb, op, s = case.nb, case.op, Shadow()
    flags = [case.variant == "trivial" and j in TRIVIAL(nb) for j in range(nb)]
    lhs, rhs = list(flags), list(flags)
    lhs_zero = [case.variant == "trivial" and j == nb // 4 for j in range(nb)]   # trivial_digit(.., 0) == 0
    rhs_zero = [False] * nb
    if case.variant == "dirty":                       # the default forms' preamble: both operands have carries
        lhs = _full_propagate(s, lhs)
        if op not in UNARY:
            rhs = _full_propagate(s, rhs)
    both = [a and b for a, b in zip(lhs, rhs)]
    if op == "neg":                                   # neg.rs:77-100; unchecked: neg.rs:39-73, no PBS
        (_full_propagate if case.variant == "unchecked" else _single_carry)(s, lhs)
    elif op == "sub":                                 # sub.rs:206-243; unchecked: radix/sub.rs:80-86, no PBS
        (_full_propagate if case.variant == "unchecked" else _single_carry)(s, both)
    elif op in BITOPS:                                # bitwise_op.rs:15-26: one bivariate PBS per block
        s.layer(both)
    elif op == "bitnot":                              # bitwise_op.rs:549-562
        s.layer(lhs)
    elif op in ("eq", "ne"):                          # comparison.rs:10-83, scalar_comparison.rs:147-191
        blocks = both
        s.layer(blocks)
        while len(blocks) > 1:
            blocks = [all(blocks[c:c + MAX_VALUE]) for c in range(0, len(blocks), MAX_VALUE)]
            s.layer(blocks)
    elif op in ORDER:                                 # comparator.rs:976-990: the sign, then map_sign_result
        s.layer([_compare(s, lhs, rhs)])
    elif op in ("max", "min"):                        # comparator.rs:849-875
        _cmux(s, _compare(s, lhs, rhs), lhs, rhs, lhs_zero, rhs_zero)
    else:                                             # cmux.rs:7-25: the condition is encrypted
        _cmux(s, False, lhs, rhs, lhs_zero, rhs_zero)
    return s.pbs, s.launches


# ---- a set with carry_modulus < message_modulus: the comparison block by block -----------------------------------
SET_3_2 = "PARAM_MESSAGE_3_CARRY_2_KS_PBS"
BLOCKS_3_2 = 3


def shadow_3_2_lt(nb):
    """one sign per block, the tree, the map"""
    s = Shadow()
    s.layer([_compare(s, [False] * nb, [False] * nb, packed=False)])
    return s.pbs, s.launches
