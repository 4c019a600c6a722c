"""Case list of the unsigned radix division (div_rem, div, rem) and of unsigned_overflowing_sub, shared by
test_integer_div.py (host path, oracle engine) and test_integer_div_gpu.py (device path against the host path).

Conventions of integer_ops_cases.py and integer_shift_cases.py: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8,
batches of K = 3 operand rows, blocks (1, 2, 3, 5, 8).  One block has no upper divisor blocks at its last bit and no
Hillis-Steele step; three and five blocks are not powers of two; eight blocks give up to seven upper blocks, hence two
chunks in compare_blocks_with_zero and a reduction pass.

A case is (operation, variant, blocks):
  unchecked         clean operands through the unchecked_* form;
  clean             clean operands through the default form;
  dirty             both operands are the sum of four encryptions: the default form propagates them first;
  trivial           blocks TRIVIAL(nb) of both operands are trivial ciphertexts (one of the numerator's of degree 0);
  trivial_divisor   the whole divisor (the right operand of the sub) is trivial, TRIVIAL_DIVISOR(nb) in every row.
Batch 0 of a case goes through the form that returns its result, every other batch through the _assign form where
the operation has one (div and rem).

A case has ROWS = 12 operand rows, four batches of K: ten crafted (numerator, divisor) pairs -- (any, 0), (any, 1),
(n, n), (n, n + 1), (max, max), (0, d), (max, 1), a divisor with its top bit set, a power-of-two divisor on a block
boundary, one inside a block -- and two random ones.  The trivial variants overwrite digits of every row.

Expected plaintexts: (n // d, n % d), and (2^T - 1, n) for d = 0, which is what the long-division loop yields; for
the sub ((a - b) mod 2^T, a < b).  Expected pbs_count and launches come from `shadow` below, which restates the loops
of div_mod.rs, sub.rs and scalar_comparison.rs on two flags per block (a trivial ciphertext or not; of degree 0 or
not).  Branches the reference runs in one rayon::join or par_iter share their passes: pass k of every branch is one
batched launch.  Nothing here is recorded from the code under test.
"""
from dataclasses import dataclass

import numpy as np

from integer_dag_cases import K, MSG, SEED, keys, params  # noqa: F401  (the same key conventions)
from integer_ops_cases import (ADDENDS, BLOCKS, CARRY, TRIVIAL, Shadow, _full_propagate, _set_digit,  # noqa: F401
                               batch_rows, decrypt, trivial_digit)
from integer_shift_cases import FRESH, ZERO, _and, _lut

BITS = 2                         # log2(MSG)
DIV_OPS = ("div_rem", "div", "rem")
SUB = "unsigned_overflowing_sub"
OPS = DIV_OPS + (SUB,)
VARIANTS = ("unchecked", "clean", "dirty", "trivial", "trivial_divisor")
ROWS = 4 * K
CRAFTED = 10


def TRIVIAL_DIVISOR(nb):
    """6 = 0b0110: bits in two blocks where there are two, upper blocks trivial zeros of degree 0"""
    return 6 % MSG ** nb


@dataclass(frozen=True)
class Case:
    op: str
    variant: str
    nb: int
    seed: int

    @property
    def id(self):
        return f"{self.op}-{self.variant}-b{self.nb}"

    @property
    def results(self):
        return 2 if self.op in ("div_rem", SUB) else 1


def _cases():
    out, seed = [], 1500
    for nb in BLOCKS:
        for op in OPS:
            for variant in VARIANTS:
                out.append(Case(op, variant, nb, seed))
                seed += 1
    return out


CASES = _cases()


# ---- plaintext side ---------------------------------------------------------------------------------------------
def values(case):
    """{"lhs": [ROWS] numerators, "rhs": [ROWS] divisors} as Python ints, the trivial digits in place"""
    nb, M = case.nb, MSG ** case.nb
    rng = np.random.default_rng(case.seed)
    lhs = [int(x) for x in rng.integers(0, M, ROWS)]
    rhs = [int(x) for x in rng.integers(0, M, ROWS)]
    n = 1 + int(rng.integers(0, M - 2)) if M > 2 else 1      # 1 .. M - 2: n and n + 1 both fit, n is not zero
    rhs[0] = 0
    rhs[1] = 1
    lhs[2], rhs[2] = n, n
    lhs[3], rhs[3] = n, n + 1
    lhs[4], rhs[4] = M - 1, M - 1
    lhs[5], rhs[5] = 0, max(rhs[5], 1)
    lhs[6], rhs[6] = M - 1, 1
    rhs[7] = M // 2 + rhs[7] % (M // 2)                       # the top bit set
    rhs[8] = MSG ** (nb // 2)                                 # a power of two on a block boundary
    rhs[9] = 2 * MSG ** (nb // 2)                             # a power of two inside a block
    if case.variant == "trivial":
        for j in TRIVIAL(nb):
            lhs = [_set_digit(v, j, trivial_digit(nb, j, 0)) for v in lhs]
            rhs = [_set_digit(v, j, trivial_digit(nb, j, 1)) for v in rhs]
    if case.variant == "trivial_divisor":
        rhs = [TRIVIAL_DIVISOR(nb)] * ROWS
    return {"lhs": lhs, "rhs": rhs}


def plain(op, a, b, nb):
    """the tuple of plain results of one row"""
    M = MSG ** nb
    if op == SUB:
        return (a - b) % M, int(a < b)
    q, r = (a // b, a % b) if b else (M - 1, a)
    return {"div_rem": (q, r), "div": (q,), "rem": (r,)}[op]


def expected(case):
    v = values(case)
    return [plain(case.op, a, b, case.nb) for a, b in zip(v["lhs"], v["rhs"])]


def result_blocks(case):
    """the block count of each result"""
    return (case.nb, 1) if case.op == SUB else (case.nb,) * case.results


# ---- ciphertext side --------------------------------------------------------------------------------------------
def encrypt(ck, case):
    """Host batches of ROWS rows: {"lhs": [batches to add up], "rhs": [...]}; a clean operand is one batch, a dirty
    one ADDENDS batches whose plaintexts add up to the operand modulo MSG ** nb.  The encryption randomness depends
    on the case alone."""
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
    return enc


def operands(case, sks, enc, b):
    """(numerator, divisor) of rows [b K, (b + 1) K) in the residency of `sks`, as the case hands them to the
    operation; the host batches of `enc` stay untouched"""
    def operand(name, index):
        x = [sks.to_device(batch_rows(e, b)) for e in enc[name]]
        for t in x[1:]:
            sks.unchecked_add_assign(x[0], t)
        if case.variant == "trivial":
            for j in TRIVIAL(case.nb):
                sks._set_trivial(x[0], j, trivial_digit(case.nb, j, index))
        if index == 1 and case.variant == "trivial_divisor":
            for j in range(case.nb):
                sks._set_trivial(x[0], j, (TRIVIAL_DIVISOR(case.nb) // MSG ** j) % MSG)
        return x[0]

    return operand("lhs", 0), operand("rhs", 1)


def assigns(case, b):
    return b != 0 and case.op in ("div", "rem")


def method(case, assign):
    return ("unchecked_" if case.variant == "unchecked" else "") + case.op + ("_assign" if assign else "") + "_parallelized"


def apply(case, sks, lhs, rhs, b):
    """The case's operation on operands in the residency of `sks`; returns the tuple of its results.  sks.pbs_count
    and sks.launches count the call alone."""
    sks.pbs_count = sks.launches = 0
    if assigns(case, b):
        assert getattr(sks, method(case, True))(lhs, rhs) is None
        return (lhs,)
    res = getattr(sks, method(case, False))(lhs, rhs)
    return tuple(res) if case.results == 2 else (res,)


def run(case, sks, enc, b):
    """The case on rows [b K, (b + 1) K) on `sks` (host or device path).  Returns (results, numerator, divisor) in
    the key's residency."""
    lhs, rhs = operands(case, sks, enc, b)
    return apply(case, sks, lhs, rhs, b), lhs, rhs


def decrypted(ck, case, results):
    """[K] tuples, as `expected` gives them"""
    cols = [decrypt(ck, rb, n) for rb, n in zip(results, result_blocks(case))]
    return [tuple(col[r] for col in cols) for r in range(K)]


# ---- the expected counts: the reference's loops on two flags per block ---------------------------------------------
# A block is (trivial, zero) as in integer_shift_cases.  A branch of a rayon::join is (passes, result): the LUT
# applications of each of its passes, as the trivial flags Shadow.layer takes.
def _join(s, *branches):
    """pass k of every branch in one batched launch"""
    for k in range(max(len(passes) for passes, _ in branches)):
        s.layer([t for passes, _ in branches if k < len(passes) for t in passes[k]])
    return [result for _, result in branches]


def _shift_left_by_one(requests, blocks):
    """unchecked_scalar_left_shift_assign_parallelized by 1 (scalar_shift.rs:553-647): no block rotation, the first
    block alone and one window per pair of neighbours, joined"""
    first = _lut(requests, blocks[0])
    return [first] + [_lut(requests, a, b) for a, b in zip(blocks, blocks[1:])]


def _overflowing_sub(lhs, rhs):
    """unchecked_unsigned_overflowing_sub_parallelized (sub.rs:355-421): shortint unchecked_sub per block (no PBS),
    generate_init_borrow_array on every block, ceil(log2(blocks)) Hillis-Steele steps over blocks space .., the input
    borrow (a trivial zero for block 0) subtracted and message_extract on every block; the last state is the output
    borrow"""
    nb, passes = len(lhs), []
    difference = [_and(a, b)[0] for a, b in zip(lhs, rhs)]
    states = list(difference)
    passes.append(list(states))
    space = 1
    for _ in range((nb - 1).bit_length()):
        step = list(states)
        for b in range(space, nb):
            step[b] = states[b] and states[b - space]
        passes.append(step[space:])
        states, space = step, space * 2
    borrows = [True] + states[:-1]
    out = [d and c for d, c in zip(difference, borrows)]
    passes.append(out)
    return passes, ([(t, False) for t in out], (states[-1], False))


def _compare_blocks_with_zero(blocks, msg=MSG, carry=CARRY):
    """scalar_comparison.rs:254-296: one LUT per chunk of (msg * carry - 1) / (msg - 1) blocks"""
    fill = (msg * carry - 1) // (msg - 1)
    requests = []
    out = [_lut(requests, *blocks[c:c + fill]) for c in range(0, len(blocks), fill)]
    return ([requests] if blocks else []), out


def _at_least_one(blocks, msg=MSG, carry=CARRY):
    """is_at_least_one_comparisons_block_true (scalar_comparison.rs:200-233) on a non-empty list: chunks of
    msg * carry - 1 until one block is left; one block is returned as it is"""
    passes, max_value = [], msg * carry - 1
    while len(blocks) > 1:
        requests = []
        blocks = [_lut(requests, *blocks[c:c + max_value]) for c in range(0, len(blocks), max_value)]
        passes.append(requests)
    return passes, blocks[0]


def _div_rem(s, numerator, divisor, bits=BITS, msg=MSG, carry=CARRY):
    """unsigned_unchecked_div_rem_parallelized (div_mod.rs:92-492)"""
    nb = len(numerator)
    total_bits = bits * nb
    quotient, remainder1, remainder2 = [ZERO] * nb, [ZERO] * nb, [ZERO] * nb
    numerator_block_stack = list(numerator)
    for i in reversed(range(total_bits)):
        block_of_bit, pos_in_block = divmod(i, bits)
        msb_bit_set = total_bits - 1 - i
        last_non_trivial_block = msb_bit_set // bits
        first_trivial_block = last_non_trivial_block + 1
        interesting_remainder1 = remainder1[:first_trivial_block]
        interesting_remainder2 = remainder2[:first_trivial_block]
        interesting_divisor = divisor[:first_trivial_block]
        divisor_ms_blocks = divisor[(msb_bit_set + 1) // bits:]
        requests = []                                            # the four tasks of :310-316
        if (msb_bit_set + 1) % bits:
            interesting_divisor[-1] = _lut(requests, interesting_divisor[-1])
        if divisor_ms_blocks and (msb_bit_set + 1) % bits:
            divisor_ms_blocks[0] = _lut(requests, divisor_ms_blocks[0])
        interesting_remainder1 = _shift_left_by_one(requests, [numerator_block_stack.pop()] + interesting_remainder1)
        numerator_block = interesting_remainder1.pop(0)          # rotate_left(1), pop
        if pos_in_block != 0:
            numerator_block_stack.append(numerator_block)
        interesting_remainder2 = _shift_left_by_one(requests, interesting_remainder2)
        s.layer(requests)
        merged = [_and(a, b) for a, b in zip(interesting_remainder1, interesting_remainder2)]

        def check_divisor_upper_blocks():
            if not divisor_ms_blocks:
                return [], ZERO
            first, tmp = _compare_blocks_with_zero(divisor_ms_blocks, msg, carry)
            more, out = _at_least_one(tmp, msg, carry)
            return first + more, out

        clean = []
        cleaned = [_lut(clean, b) for b in merged]
        (new_remainder, overflowed), upper_non_zero, _ = _join(
            s, _overflowing_sub(merged, interesting_divisor), check_divisor_upper_blocks(), ([clean], None))
        requests = []                                            # the three tasks of :442-447
        remainder1[:first_trivial_block] = [_lut(requests, b, overflowed, upper_non_zero) for b in cleaned]
        remainder2[:first_trivial_block] = [_lut(requests, b, overflowed, upper_non_zero) for b in new_remainder]
        did_not_overflow = _lut(requests, overflowed, upper_non_zero)
        quotient[block_of_bit] = _and(quotient[block_of_bit], did_not_overflow)
        s.layer(requests)
    requests = []                                                # :473-489, joined
    remainder = [_lut(requests, a, b) for a, b in zip(remainder1, remainder2)]
    quotient = [_lut(requests, b) for b in quotient]
    s.layer(requests)
    return quotient, remainder


def operand_flags(case):
    """(numerator, divisor) as the operation meets them, before a default form's preamble"""
    nb = case.nb
    lhs, rhs = [FRESH] * nb, [FRESH] * nb
    if case.variant == "trivial":
        lhs = [(j in TRIVIAL(nb), j in TRIVIAL(nb) and trivial_digit(nb, j, 0) == 0) for j in range(nb)]
        rhs = [(j in TRIVIAL(nb), False) for j in range(nb)]
    if case.variant == "trivial_divisor":
        rhs = [(True, (TRIVIAL_DIVISOR(nb) // MSG ** j) % MSG == 0) for j in range(nb)]
    return lhs, rhs


def shadow(case):
    """(pbs_count, launches) of one batch of K rows"""
    s = Shadow()
    lhs, rhs = operand_flags(case)
    if case.variant == "dirty":                       # the default forms' preamble: both operands have carries
        _full_propagate(s, [False] * case.nb)
        _full_propagate(s, [False] * case.nb)
    if case.op == SUB:
        _join(s, _overflowing_sub(lhs, rhs))
    else:
        _div_rem(s, lhs, rhs)
    return s.pbs, s.launches


def shadow_of_clean_division(nb, bits=BITS, msg=MSG, carry=CARRY):
    s = Shadow()
    _div_rem(s, [FRESH] * nb, [FRESH] * nb, bits, msg, carry)
    return s.pbs, s.launches


# ---- a set with 3 message bits ---------------------------------------------------------------------------------------
SET_3_3 = "PARAM_MESSAGE_3_CARRY_3_KS_PBS"   # message modulus 8, carry modulus 8: div_refusal accepts it
BLOCKS_3_3 = 2                                # T = 6: three in-block positions, two-bit trim masks, chunks of 9 and 63
