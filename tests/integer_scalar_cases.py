"""Case list of the radix operations with a clear operand (scalar_add, scalar_sub, the scalar bitwise ops, the
scalar comparisons, scalar_max / scalar_min), one clear operand per batch or one per row, shared by
test_integer_scalar.py (host path, oracle engine) and test_integer_scalar_gpu.py (device path against the host path).

Conventions of integer_ops_cases.py / integer_shift_cases.py: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8,
batches of K = 3 rows, blocks (1, 2, 3, 5, 8), so T = 2, 4, 6, 10, 16 bits, and the variants
  unchecked  clean operands through the unchecked_* form;
  clean      clean operands through the default form;
  dirty      the encrypted operand is the sum of four encryptions: the default form propagates it first;
  trivial    blocks TRIVIAL(nb) of the encrypted operand are trivial ciphertexts (one of them of degree 0).
Batch 0 of a case goes through the form that returns a new batch, every other batch through the _assign form where
the reference has one (add, sub, the bitwise ops).

A case is (operation, variant, blocks, form):
  int    one Python int for the whole batch; batch b of the case takes SCALARS(op, nb)[b]: 0, 1, msg - 1, msg,
         2^T - 1, 2^T, 2^T + 3, a value whose top digit is 0 with the digit below set, and -1 for the comparisons;
  rows   one value per row, a numpy uint64 array; three batches, see clear_rows: batch 0 holds 2^T - 1, a value with
         only the top digit set and a random one with a non-zero top digit (every row has a non-zero top digit: the
         batch is bit-identical to the one-int form row by row); batch 1 holds 0, the encrypted value itself and that
         value + 1; batch 2 that value - 1, a value whose top digit is 0, and a random one.

Expected pbs_count and launches come from `shadow` below, which restates the loop structure of the reference
functions on two flags per block (a trivial ciphertext or not; of degree 0 or not).  For the per-row form it runs
with the scalar 2^T - 1, whose digits cover every block, and counts a request with a LUT per row as a bootstrap
even where its blocks are trivial: the batched PBS serves it, the trivial PBS takes one LUT for all rows.  Nothing
here is recorded from the code under test.
"""
from dataclasses import dataclass

import numpy as np

from integer_dag_cases import FILL, K, MSG, SEED, keys, params  # noqa: F401  (the same key conventions)
from integer_ops_cases import (ADDENDS, BITOPS, BLOCKS, CARRY, MAX_VALUE, ORDER, TRIVIAL, Shadow, _cmux,  # noqa: F401
                               _full_propagate, _set_digit, _single_carry, batch_rows, trivial_digit)

BITS = 2                         # log2(MSG)
ARITHMETIC = ("scalar_add", "scalar_sub")
BITWISE = tuple(f"scalar_{op}" for op in BITOPS)
EQUALITY = ("scalar_eq", "scalar_ne")
ORDERED = tuple(f"scalar_{op}" for op in ORDER)
SELECT = ("scalar_max", "scalar_min")
BOOLEAN = EQUALITY + ORDERED
COMPARISONS = BOOLEAN + SELECT
OPS = ARITHMETIC + BITWISE + COMPARISONS
VARIANTS = ("unchecked", "clean", "dirty", "trivial")
FORMS = ("int", "rows")
IS_INFERIOR, IS_EQUAL, IS_SUPERIOR = 0, 1, 2


def _distinct(values):
    return tuple(dict.fromkeys(values))


def top_zero(nb):
    """a value whose top digit is 0 with the digit below set (one block: 0)"""
    return 2 * MSG ** (nb - 2) + (1 if nb > 2 else 0) if nb > 1 else 0


def SCALARS(op, nb):
    M = MSG ** nb
    return _distinct((0, 1, MSG - 1, MSG, M - 1, M, M + 3, top_zero(nb)) + ((-1,) if op in COMPARISONS else ()))


@dataclass(frozen=True)
class Case:
    op: str
    variant: str
    nb: int
    form: str
    seed: int

    @property
    def id(self):
        return f"{self.op}-{self.variant}-b{self.nb}-{self.form}"

    @property
    def batches(self):
        return len(SCALARS(self.op, self.nb)) if self.form == "int" else 3

    @property
    def rows(self):
        return self.batches * K


def _cases():
    out, seed = [], 2000
    for nb in BLOCKS:
        for op in OPS:
            for variant in VARIANTS:
                for form in FORMS:
                    out.append(Case(op, variant, nb, form, seed))
                    seed += 1
    return out


CASES = _cases()


# ---- plaintext side ---------------------------------------------------------------------------------------------
def values(case):
    """the encrypted operand row by row, as Python ints, the trivial digits in place.  Without them every value is
    in [1, 2^T - 2], so that value - 1 and value + 1 exist."""
    nb, M = case.nb, MSG ** case.nb
    rng = np.random.default_rng(case.seed)
    lhs = [1 + int(x) for x in rng.integers(0, M - 2, case.rows)]
    if case.variant == "trivial":
        for j in TRIVIAL(nb):
            lhs = [_set_digit(v, j, trivial_digit(nb, j, 0)) for v in lhs]
    return lhs


def clear_rows(case):
    """the clear operand row by row, as Python ints"""
    nb, M = case.nb, MSG ** case.nb
    if case.form == "int":
        return [s for s in SCALARS(case.op, nb) for _ in range(K)]
    v = values(case)
    rng = np.random.default_rng(case.seed + 13)
    top = MSG ** (nb - 1)
    r = [int(x) for x in rng.integers(0, M, 3)]
    return [M - 1, (MSG - 1) * top, r[0] % top + (1 + r[0] % (MSG - 1)) * top,                 # top digits 3, 3, 1 or 2
            0, v[4], v[5] + 1 if v[5] + 1 < M else r[1],
            v[6] - 1 if v[6] > 0 else r[1], r[2] % top, r[1]]


def full_width(case, b):
    """whether every clear operand of batch b has a non-zero top message digit and fits the ciphertext: the one-int
    DAG of each is then the full-width one"""
    top = MSG ** (case.nb - 1)
    return all(top <= c < MSG * top for c in clear_rows(case)[b * K:(b + 1) * K])


def plain(op, v, c, nb):
    """the plain semantics of an unsigned operand of T bits against a clear operand of any size or sign: add, sub
    and the bitwise ops work modulo 2^T, the comparisons on the integers, and max / min give the clear operand
    modulo 2^T where it wins (create_trivial_radix)"""
    M = MSG ** nb
    kind = op[len("scalar_"):]
    if kind == "add":
        return (v + c) % M
    if kind == "sub":
        return (v - c) % M
    if kind in BITOPS:
        return BITOPS[kind](v, c % M)
    if kind == "eq":
        return int(v == c)
    if kind == "ne":
        return int(v != c)
    if kind in ORDER:
        return int(ORDER[kind](v, c))
    return v if (v > c if kind == "max" else v < c) else c % M


def expected(case):
    return [plain(case.op, v, c, case.nb) for v, c in zip(values(case), clear_rows(case))]


def result_blocks(case):
    return 1 if case.op in BOOLEAN else case.nb


# ---- ciphertext side --------------------------------------------------------------------------------------------
def encrypt(ck, case):
    """Host batches of case.rows rows to add up: a clean operand is one batch, a dirty one ADDENDS batches whose
    plaintexts add up to the operand modulo MSG ** nb.  The encryption randomness depends on the case alone."""
    from tfhe_mi355 import integer

    ck._enc_counter = case.seed << 8
    cks, M = integer.ClientKey(ck, case.nb), MSG ** case.nb
    rng = np.random.default_rng(case.seed + 7)
    parts = [np.asarray(values(case), dtype=np.uint64)]
    if case.variant == "dirty":
        extra = rng.integers(0, M, (ADDENDS - 1, case.rows), dtype=np.uint64)
        parts = [(parts[0] + np.uint64(ADDENDS - 1) * np.uint64(M) - extra.sum(axis=0)) % np.uint64(M)] + list(extra)
    return [cks.encrypt(p) for p in parts]


def decrypt(ck, rb, nblocks):
    """the value of every row, carries included: sum of block * MSG^j modulo MSG^nblocks (an unchecked add leaves
    carries in the blocks)"""
    from tfhe_mi355 import client

    p = ck.parameters
    out = [0] * rb.count
    for j in range(nblocks):
        raw = client.lwe_decrypt(ck.large_lwe_secret_key, np.ascontiguousarray(rb.data[:, j, :]))
        d = client.decode(raw, p.delta) % np.uint64(MSG * CARRY)
        out = [(o + int(x) * MSG ** j) % MSG ** nblocks for o, x in zip(out, d)]
    return out


def operand(case, sks, enc, b):
    """rows [b K, (b + 1) K) of the encrypted operand in the residency of `sks`, as the case hands them to the
    operation; the host batches of `enc` stay untouched"""
    x = [sks.to_device(batch_rows(e, b)) for e in enc]
    for t in x[1:]:
        sks.unchecked_add_assign(x[0], t)
    if case.variant == "trivial":
        for j in TRIVIAL(case.nb):
            sks._set_trivial(x[0], j, trivial_digit(case.nb, j, 0))
    return x[0]


def clear_operand(case, b):
    """the clear operand of batch b as the case hands it over: a Python int, or a numpy uint64 array of K values"""
    c = clear_rows(case)[b * K:(b + 1) * K]
    return c[0] if case.form == "int" else np.asarray(c, dtype=np.uint64)


def has_assign(op):
    return op in ARITHMETIC + BITWISE


def method(op, unchecked, assign=False):
    tail = "_assign" if assign else ""
    if op in ARITHMETIC:
        return f"unchecked_{op}{tail}" if unchecked else f"{op}{tail}_parallelized"
    return ("unchecked_" if unchecked else "") + op + tail + "_parallelized"


def apply(case, sks, lhs, clear, b):
    """The case's operation on an operand in the residency of `sks`.  sks.pbs_count and sks.launches count the call
    alone."""
    sks.pbs_count = sks.launches = 0
    unchecked = case.variant == "unchecked"
    if b == 0 or not has_assign(case.op):
        return getattr(sks, method(case.op, unchecked))(lhs, clear)
    assert getattr(sks, method(case.op, unchecked, True))(lhs, clear) is None
    return lhs


def run(case, sks, enc, b, clear=None):
    """The case on rows [b K, (b + 1) K) on `sks` (host or device path), with the case's clear operand or the one
    given.  Returns (result, operand) in the key's residency."""
    lhs = operand(case, sks, enc, b)
    return apply(case, sks, lhs, clear_operand(case, b) if clear is None else clear, b), lhs


# ---- the expected counts: the reference's loops on two flags per block ---------------------------------------------
def _digits(value, bits):
    """BlockDecomposer::with_early_stop_at_zero"""
    out = []
    while value:
        out.append(value & ((1 << bits) - 1))
        value >>= bits
    return out


def _pairs(flags):
    """pack_block_chunk over par_chunks(2): a packed block is trivial where both blocks are"""
    return [all(flags[j:j + 2]) for j in range(0, len(flags), 2)]


def _zero_chunks(flags):
    """compare_blocks_with_zero (scalar_comparison.rs:254-296): one LUT per chunk of FILL blocks"""
    return [all(flags[c:c + FILL]) for c in range(0, len(flags), FILL)]


def _block_true_passes(blocks):
    """are_all_ / is_at_least_one_comparisons_block_true (scalar_comparison.rs:147-233): the passes, and the block
    left; one block comes back as it is"""
    passes = []
    while len(blocks) > 1:
        blocks = [all(blocks[c:c + MAX_VALUE]) for c in range(0, len(blocks), MAX_VALUE)]
        passes.append(blocks)
    return passes, blocks[0]


def _sign_tree_passes(signs):
    """reduce_signs_parallelized (comparator.rs:257-280)"""
    passes = []
    while len(signs) != 1:
        pairs = [signs[2 * c] and signs[2 * c + 1] for c in range(len(signs) // 2)]
        passes.append(pairs)
        signs = pairs + (signs[-1:] if len(signs) % 2 else [])
    return passes, signs[0]


def _joined(s, *branches):
    """rayon::join over branches of several passes each: pass k of every branch is one batched launch"""
    for k in range(max((len(b) for b in branches), default=0)):
        s.layer([r for b in branches if k < len(b) for r in b[k]])


def _equality(s, flags, clear, per_row):
    """unchecked_scalar_{eq,ne}_parallelized (scalar_comparison.rs:366-558)"""
    nb = len(flags)
    halved = (nb + 1) // 2
    if per_row:
        blocks = [False] * halved                     # a LUT per row: the batched PBS whatever the blocks are
    else:
        if clear < 0:
            return
        digits = _digits(clear, 2 * BITS)
        if any(digits[halved:]):
            return
        digits = digits[:halved]
        split = min(nb, 2 * len(digits))
        blocks = _pairs(flags[:split]) + _zero_chunks(flags[split:])      # joined: one pass
    s.layer(blocks)
    for p in _block_true_passes(blocks)[0]:
        s.layer(p)


def _sign(s, flags, clear):
    """unsigned_unchecked_scalar_compare_blocks_parallelized (comparator.rs:677-783): (the sign block is trivial,
    it is of degree 0)"""
    nb = len(flags)
    if clear < 0:
        return True, False                            # a trivial IS_SUPERIOR
    digits = _digits(clear, BITS)
    if any(digits[nb:]):
        return True, True                             # a trivial IS_INFERIOR: the value 0, degree 0
    covered = min(len(digits), nb)
    branches, signs = [], []
    if covered:
        first = _pairs(flags[:covered])
        passes, sign = _sign_tree_passes(first)
        branches.append([first] + passes)
        signs.append(sign)
    if covered < nb:
        zero = _zero_chunks(flags[covered:])
        passes, one = _block_true_passes(zero)
        branches.append([zero] + passes + [[one]])    # and the LUT 1 -> IS_EQUAL, else IS_SUPERIOR
        signs.append(one)
    _joined(s, *branches)
    if len(signs) == 2:
        s.layer([all(signs)])                         # reduce_two_sign_blocks_assign
    return all(signs), False


def _select(s, op, sign, lhs, lhs_zero, rhs_zero):
    """unchecked_scalar_min_or_max_parallelized (comparator.rs:877-912): the cmux of lhs and the trivial radix of
    the scalar on the sign; a sign of degree 0 (the scalar is out of range above: IS_INFERIOR) decides on the spot
    (zero_out_if, cmux.rs:292-299), and only the message extraction is left"""
    trivial, zero = sign
    rhs = [True] * len(lhs)
    if not zero:
        return _cmux(s, trivial, lhs, rhs, lhs_zero, rhs_zero)
    s.layer(rhs if op == "scalar_max" else lhs)       # max: lhs zeroed, the trivial rhs kept; min: lhs kept


def shadow(case, b):
    """(pbs_count, launches) of batch b of K rows"""
    nb, op, s = case.nb, case.op, Shadow()
    M = MSG ** nb
    per_row = case.form == "rows"
    clear = M - 1 if per_row else clear_rows(case)[b * K]
    trivial = case.variant == "trivial"
    lhs = [trivial and j in TRIVIAL(nb) for j in range(nb)]
    lhs_zero = [trivial and j == nb // 4 for j in range(nb)]                  # trivial_digit(.., 0) == 0
    if case.variant == "dirty":                       # the default forms' preamble
        lhs = _full_propagate(s, lhs)
    if op in ARITHMETIC:                              # radix/scalar_add.rs:53-65: no PBS; then the single carries
        if case.variant != "unchecked":
            _single_carry(s, lhs)
    elif op in BITWISE:                               # scalar_bitwise_op.rs:17-45: one PBS per digit of the scalar
        s.layer([False] * nb if per_row else lhs[:len(_digits(clear, BITS))])
    elif op in EQUALITY:
        _equality(s, lhs, clear, per_row)
    else:
        sign = _sign(s, lhs, clear)
        if op in ORDERED:
            s.layer([sign[0]])                        # map_sign_result (comparator.rs:957-971)
        else:
            rhs_zero = [not per_row and (clear % M >> (BITS * j)) % MSG == 0 for j in range(nb)]
            _select(s, op, sign, lhs, lhs_zero, rhs_zero)
    return s.pbs, s.launches
