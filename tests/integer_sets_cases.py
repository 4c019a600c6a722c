"""Case list of the radix integer layer at every modulus pair it accepts, shared by test_integer_sets.py (host path,
oracle engine) and test_integer_sets_gpu.py (device path against the host path).  The other integer_*_cases.py fix
PARAM_MESSAGE_2_CARRY_2_KS_PBS; everything here is generic in the set: its message modulus, its bits per block, its
block count, its delta.

A set is taken from SHORTINT_ALL with lwe_dimension = 8 (tiny keys, lower noise: decryption still holds) and runs
batches of K = 3 operand rows at the block count of SETS.  TABLE says, set by set, which operations the layer serves
and which it refuses by name; it is written out from the refusal rules of the reference's own arithmetic (4 bits per
block for the Hillis-Steele propagation and the comparisons, two messages in a block for a bivariate PBS, three bits
for the barrel shifter's mux) and not computed from the code under test.

A case is (set, operation, variant, blocks, form):
  clean     clean operands through the default form: every set;
  dirty     every encrypted operand is the sum of message_modulus encryptions (degree msg * (msg - 1)), so the
            default form propagates it first: 3_3 and 4_4;
  trivial   block 0 of both encrypted operands is a trivial ciphertext (the left one's of degree 0), and with three
            blocks or more the top block as well, so the trivial PBS runs at the set's delta and box: 3_3 and 4_4.
form: "" two encrypted operands; "int" one clear Python int for the whole batch (per-row operations: the clear
operand of the batch's first row; scalar_left_shift and scalar_mul: the case's own scalar); "rows" one clear operand
per row.

A case has ROWS = 6 operand rows, two batches of K.  Rows 0 .. 3 are crafted, rows 4 and 5 random:
  two encrypted operands   equal; differing only in block 0; only in the top block; all-ones against zero
  division                 divisor 1; divisor numerator + 1; divisor msg^blocks - 1; all-ones by zero
  encrypted shift          amounts 0, 1, T - 1, 2^T - 1
  clear operand per row    0; msg^blocks - 1; the encrypted operand itself, its low packed digit (two blocks) forced
                           to msg^2 - 2, which is 16 or more from 3 message bits on: the LUT index leaves the range
                           PARAM_MESSAGE_2_CARRY_2 has; the encrypted operand with another top digit
  scalar_left_shift        one case per amount 0, 1, T - 1
The trivial variant overwrites the digits of its trivial blocks in every row.

Expected values are plain Python integers modulo msg^blocks.  Nothing here is recorded from the code under test.
"""
from dataclasses import dataclass

import numpy as np

SEED = 11          # ClientKey seed: the GPU key and the oracle-engine key of a set are built from the same one
K = 3
ROWS = 2 * K

# set -> (name in SHORTINT_ALL, blocks)
SETS = {
    "3_3": ("PARAM_MESSAGE_3_CARRY_3_KS_PBS", 3),
    "4_4": ("PARAM_MESSAGE_4_CARRY_4_KS_PBS", 2),
    "2_3": ("PARAM_MESSAGE_2_CARRY_3_KS_PBS", 3),
    "3_2": ("PARAM_MESSAGE_3_CARRY_2_KS_PBS", 3),
    "4_2": ("PARAM_MESSAGE_4_CARRY_2_KS_PBS", 2),
    "1_1": ("PARAM_MESSAGE_1_CARRY_1_KS_PBS", 5),
}
# (message modulus, carry modulus), written out: the cases must not take them from the code under test
MODULI = {"3_3": (8, 8), "4_4": (16, 16), "2_3": (4, 8), "3_2": (8, 4), "4_2": (16, 4), "1_1": (2, 2)}

SUB = "unsigned_overflowing_sub"
BINARY = ("sub", "mul", "bitxor", "eq", "ne", "lt", "max", SUB, "div_rem")
PER_ROW = ("scalar_add", "scalar_bitand", "scalar_eq", "scalar_lt")      # one clear operand per batch or per row
ONE_INT = ("scalar_left_shift", "scalar_mul")                            # one clear operand per batch
OPS = ("sub", "mul", "bitxor", "eq", "lt", "max") + PER_ROW + ("scalar_left_shift", "left_shift", "scalar_mul", SUB,
                                                               "div_rem")
BOOLEAN = ("eq", "ne", "lt", "scalar_eq", "scalar_lt")

_ALL = OPS
_NO_PROPAGATION = ("bitxor", "eq", "lt", "max", "scalar_bitand", "scalar_eq", "scalar_lt", "scalar_left_shift",
                   "left_shift", SUB, "div_rem")
_NO_BIVARIATE = ("sub", "lt", "scalar_add", "scalar_bitand", "left_shift", SUB)
_TWO_BITS = ("bitxor", "eq", "scalar_bitand", "scalar_eq", "scalar_left_shift")
# set -> the operations served; every other one of OPS is refused by name
TABLE = {"3_3": _ALL, "4_4": _ALL, "2_3": _NO_PROPAGATION, "3_2": _NO_BIVARIATE, "4_2": _NO_BIVARIATE, "1_1": _TWO_BITS}
FULL = ("3_3", "4_4")               # the sets that also run the dirty and the trivial variant


def params(s):
    from tfhe_mi355.parameters import SHORTINT_ALL

    return SHORTINT_ALL[SETS[s][0]].with_(lwe_dimension=8)


def keys(s, engine=None):
    """(shortint ClientKey, integer ServerKey) of set `s` on `engine` (None: the GPU engine on device 0)"""
    from tfhe_mi355 import integer, shortint

    ck = shortint.ClientKey(params(s), SEED)
    return ck, integer.ServerKey(shortint.ServerKey(ck, engine=engine))


def msg(s):
    return MODULI[s][0]


def bits(s):
    return MODULI[s][0].bit_length() - 1


def multiplier(s):
    """scalar_mul's clear operand: not a power of two, so the chunked sum runs"""
    return msg(s) + 1


@dataclass(frozen=True)
class Case:
    set: str
    op: str
    variant: str
    nb: int
    form: str       # "", "int" or "rows"
    scalar: int     # scalar_left_shift's amount, scalar_mul's multiplier; -1 otherwise
    seed: int

    @property
    def id(self):
        tail = f"-{self.form}" if self.op in PER_ROW else f"-by{self.scalar}" if self.op in ONE_INT else ""
        return f"{self.set}-{self.op}{tail}-{self.variant}-b{self.nb}"

    @property
    def msg(self):
        return msg(self.set)

    @property
    def M(self):
        return msg(self.set) ** self.nb

    @property
    def T(self):
        return bits(self.set) * self.nb


def _forms(s, op, nb):
    """(form, scalar) of the cases of one operation"""
    if op in PER_ROW:
        return [("int", -1), ("rows", -1)]
    if op == "scalar_left_shift":
        T = bits(s) * nb
        return [("int", a) for a in sorted({0, 1, T - 1})]
    if op == "scalar_mul":
        return [("int", multiplier(s))]
    return [("", -1)]


def _cases():
    served, refused, seed = [], [], 3000
    for s, (_, nb) in SETS.items():
        for op in OPS:
            for form, scalar in _forms(s, op, nb):
                if op not in TABLE[s]:
                    refused.append(Case(s, op, "clean", nb, form, scalar, seed))
                    seed += 1
                    continue
                for variant in ("clean", "dirty", "trivial") if s in FULL else ("clean",):
                    served.append(Case(s, op, variant, nb, form, scalar, seed))
                    seed += 1
    # eq / ne over one sum of 9 terms (three block-layer calls on the device) and over chunks of 3 and 2 blocks with a
    # second reduction level; the borrow prefix sum with carry < msg at 1, 2, 3 and 5 blocks (no step, one, two, three)
    extra = [("3_3", "eq", 9), ("3_3", "ne", 9), ("1_1", "ne", 5)]
    extra += [(s, SUB, nb) for s in ("3_2", "4_2") for nb in (1, 2, 3, 5) if nb != SETS[s][1]]
    for s, op, nb in extra:
        served.append(Case(s, op, "clean", nb, "", -1, seed))
        seed += 1
    return served, refused


CASES, REFUSED = _cases()


# ---- plaintext side ---------------------------------------------------------------------------------------------
def trivial_blocks(nb):
    return [0] if nb < 3 else [0, nb - 1]


def trivial_digit(case, j, operand):
    """the digit a trivial block holds, the same in every row: 0 (degree 0) at block 0 of the left operand"""
    if operand == 0:
        return 0 if j == 0 else case.msg - 3
    return case.msg - 1 if j == 0 else 2


def _set_digit(v, j, d, m):
    return v - ((v // m ** j) % m) * m ** j + d * m ** j


def _trivial(case, values, operand):
    if case.variant != "trivial":
        return values
    for j in trivial_blocks(case.nb):
        values = [_set_digit(v, j, trivial_digit(case, j, operand), case.msg) for v in values]
    return values


def values(case):
    """{"lhs": [ROWS], "rhs": [ROWS] or None, "clear": [ROWS] or None} as Python ints, the trivial digits in place"""
    m, nb, M, T = case.msg, case.nb, case.M, case.T
    rng = np.random.default_rng(case.seed)
    lhs = [int(x) for x in rng.integers(0, M, ROWS)]
    other = [int(x) for x in rng.integers(0, M, ROWS)]
    top = m ** (nb - 1)
    if case.op in PER_ROW:
        if nb > 1:
            lhs[2] = lhs[2] - lhs[2] % (m * m) + m * m - 2          # the low packed digit
        lhs = _trivial(case, lhs, 0)
        other[0], other[1], other[2] = 0, M - 1, lhs[2]
        other[3] = _set_digit(lhs[3], nb - 1, (lhs[3] // top + 1) % m, m)
        return {"lhs": lhs, "rhs": None, "clear": other}
    if case.op in ONE_INT:
        lhs[3] = M - 1
        return {"lhs": _trivial(case, lhs, 0), "rhs": None, "clear": None}
    if case.op == "left_shift":
        lhs[3] = M - 1
        other[:4] = [0, 1 % M, T - 1, M - 1]
    elif case.op == "div_rem":
        lhs[1] = lhs[1] % (M - 1)                                   # numerator + 1 fits
        other[:4] = [1, lhs[1] + 1, M - 1, 0]
        lhs[3] = M - 1
    else:
        other[0] = lhs[0]                                                          # equal
        other[1] = _set_digit(lhs[1], 0, (lhs[1] % m + 1) % m, m)                  # differ only in block 0
        other[2] = _set_digit(lhs[2], nb - 1, (lhs[2] // top + m // 2) % m, m)     # differ only in the top block
        lhs[3], other[3] = M - 1, 0                                                # all-ones against zero
    return {"lhs": _trivial(case, lhs, 0), "rhs": _trivial(case, other, 1), "clear": None}


def control_bits(T):
    """the bits of an encrypted amount the barrel shifter reads (shift.rs:345-353)"""
    return T.bit_length() - 1 + (1 if T & (T - 1) else 0)


def plain(case, a, b):
    """the tuple of plain results of one row; b: the right operand, encrypted or clear"""
    op, M, T = case.op, case.M, case.T
    if op in ("sub", "scalar_sub"):
        return ((a - b) % M,)
    if op == "scalar_add":
        return ((a + b) % M,)
    if op in ("mul", "scalar_mul"):
        return ((a * b) % M,)
    if op == "bitxor":
        return (a ^ b,)
    if op == "scalar_bitand":
        return (a & b,)
    if op in ("eq", "scalar_eq"):
        return (int(a == b),)
    if op == "ne":
        return (int(a != b),)
    if op in ("lt", "scalar_lt"):
        return (int(a < b),)
    if op == "max":
        return (max(a, b),)
    if op == "scalar_left_shift":
        return ((a << (b % T)) % M,)
    if op == "left_shift":
        return ((a << (b % 2 ** control_bits(T))) % M,)
    if op == SUB:
        return (a - b) % M, int(a < b)
    assert op == "div_rem"
    return (a // b, a % b) if b else (M - 1, a)     # what the long-division loop yields for a zero divisor


def clear_rows(case, b):
    """the clear operands of batch b as Python ints: one per row; forms "int": K times the batch's one"""
    v = values(case)
    if case.op in ONE_INT:
        return [case.scalar] * K
    rows = v["clear"][b * K:(b + 1) * K]
    return [rows[0]] * K if case.form == "int" else rows


def expected(case):
    """[ROWS] tuples of Python ints"""
    v = values(case)
    if v["rhs"] is not None:
        right = v["rhs"]
    else:
        right = clear_rows(case, 0) + clear_rows(case, 1)
    return [plain(case, a, b) for a, b in zip(v["lhs"], right)]


def result_blocks(case):
    """the block count of each result"""
    if case.op == SUB:
        return case.nb, 1
    if case.op == "div_rem":
        return case.nb, case.nb
    return (1,) if case.op in BOOLEAN else (case.nb,)


# ---- ciphertext side --------------------------------------------------------------------------------------------
def encrypt(ck, case):
    """Host batches of ROWS rows: {"lhs": [batches to add up], "rhs": [...] or None}; a clean operand is one batch, a
    dirty one msg batches whose plaintexts add up to the operand modulo msg ** nb.  The encryption randomness
    depends on the case alone."""
    from tfhe_mi355 import integer

    ck._enc_counter = case.seed << 10
    cks, M, addends = integer.ClientKey(ck, case.nb), case.M, case.msg
    v = values(case)
    rng = np.random.default_rng(case.seed + 7)
    enc = {"rhs": None}
    for name in ("lhs", "rhs"):
        if v[name] is None:
            continue
        parts = [np.asarray(v[name], dtype=np.uint64)]
        if case.variant == "dirty":
            extra = rng.integers(0, M, (addends - 1, ROWS), dtype=np.uint64)
            parts = [(parts[0] + np.uint64(addends - 1) * np.uint64(M) - extra.sum(axis=0)) % np.uint64(M)] + list(extra)
        enc[name] = [cks.encrypt(p) for p in parts]
    return enc


def inputs(enc):
    """every host batch of `enc`"""
    return enc["lhs"] + (enc["rhs"] or [])


def batch_rows(rb, b):
    """rows [b K, (b + 1) K) of a host batch, as a batch of its own"""
    from tfhe_mi355.integer import RadixBatch

    return RadixBatch(rb.data[b * K:(b + 1) * K].copy(), list(rb.degree), list(rb.noise))


def operands(case, sks, enc, b):
    """(left, right or None) of rows [b K, (b + 1) K) in the residency of `sks`, as the case hands them to the
    operation; the host batches of `enc` stay untouched"""
    def operand(name, index):
        if enc[name] is None:
            return None
        x = [sks.to_device(batch_rows(e, b)) for e in enc[name]]
        for t in x[1:]:
            sks.unchecked_add_assign(x[0], t)
        if case.variant == "trivial":
            for j in trivial_blocks(case.nb):
                sks._set_trivial(x[0], j, trivial_digit(case, j, index))
        return x[0]

    return operand("lhs", 0), operand("rhs", 1)


def clear_operand(case, b):
    """the clear operand of batch b as the host forms hand it over: a Python int, or a numpy uint64 array of K"""
    rows = clear_rows(case, b)
    return np.asarray(rows, dtype=np.uint64) if case.form == "rows" else rows[0]


def method(case):
    return f"{case.op}_parallelized"


def apply(case, sks, lhs, right):
    """The case's operation on operands in the residency of `sks`; right: the encrypted or the clear operand.
    Returns the tuple of its results; sks.pbs_count and sks.launches count the call alone."""
    sks.pbs_count = sks.launches = 0
    res = getattr(sks, method(case))(lhs, right)
    return tuple(res) if case.op in (SUB, "div_rem") else (res,)


def run(case, sks, enc, b):
    """The case on rows [b K, (b + 1) K) on `sks` (host or device path), a clear operand in its host form"""
    lhs, rhs = operands(case, sks, enc, b)
    return apply(case, sks, lhs, rhs if rhs is not None else clear_operand(case, b))


def decrypted(ck, case, results):
    """[K] tuples, as `expected` gives them"""
    from tfhe_mi355 import integer

    cols = [[int(x) for x in integer.ClientKey(ck, n).decrypt(rb)] for rb, n in zip(results, result_blocks(case))]
    return [tuple(col[r] for col in cols) for r in range(K)]
