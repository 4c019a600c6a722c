"""Case list of the radix shifts and rotations by a clear amount, by an encrypted amount, and of scalar_mul, shared
by test_integer_shift.py (host path, oracle engine) and test_integer_shift_gpu.py (device path against the host
path).

Conventions of integer_ops_cases.py: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8, batches of K = 3 operand
rows, blocks (1, 2, 3, 5, 8), so T = bits * blocks = 2, 4, 6, 10, 16 bits in all and s = 1, 2, 3, 4, 4 control bits
of the barrel shifter: totals that are a power of two and totals that are not, and one block, where the giver and
the receiver of a rotation are the same block.

A case is (operation, variant, blocks, clear operand):
  scalar_{left_shift,right_shift,rotate_left,rotate_right}   one clear amount per case, AMOUNTS(nb)
  {left_shift,right_shift,rotate_left,rotate_right}          encrypted amounts, one per row: amount_rows(nb)
  scalar_mul                                                 one clear multiplier per case, MULTIPLIERS(nb)
with the variants of integer_ops_cases.py:
  unchecked  clean operands through the unchecked_* form;
  clean      clean operands through the default form;
  dirty      every encrypted operand, the amount included, is the sum of four encryptions: the default form
             propagates them before it starts;
  trivial    blocks TRIVIAL(nb) of the value are trivial ciphertexts (one of them of degree 0);
  trivial_amount   (encrypted amounts only) the same, and the whole amount operand is trivial: every row shifts by
             TRIVIAL_AMOUNT(nb).
Batch 0 of a case goes through the form that returns a new batch, batch 1 through the _assign form.

A case has ROWS = 6 operand rows, two batches of K.  The crafted encrypted amounts are 0, 1, T - 1, T and 2^s - 1;
two further rows are random.  Where T is a power of two 2^s - 1 is T - 1 again and six rows hold them; where it is
not (3 and 5 blocks) there are five distinct crafted amounts, and the case takes a third batch (9 rows, four of
them random) so that none is left out.  With one block T - 1 = 2^s - 1 = 1, and three rows are random.

Expected pbs_count and launches come from `shadow` below, which restates the loop structure of the reference
functions on two flags per block (a trivial ciphertext or not; of degree 0 or not, which the chunked sum's
first_add / last_add windows look at).  Nothing here is recorded from the code under test.
"""
from dataclasses import dataclass

import numpy as np

from integer_dag_cases import FILL, K, MSG, SEED, keys, params  # noqa: F401  (the same key conventions)
from integer_ops_cases import (ADDENDS, BLOCKS, TRIVIAL, Shadow, _full_propagate, _set_digit, _single_carry,  # noqa: F401
                               batch_rows, decrypt, trivial_digit)

BITS = 2                         # log2(MSG)
SCALAR_OPS = ("scalar_left_shift", "scalar_right_shift", "scalar_rotate_left", "scalar_rotate_right")
ENCRYPTED_OPS = ("left_shift", "right_shift", "rotate_left", "rotate_right")
OPS = SCALAR_OPS + ENCRYPTED_OPS + ("scalar_mul",)
VARIANTS = ("unchecked", "clean", "dirty", "trivial")


def total_bits(nb):
    return BITS * nb


def control_bits(nb):
    """shift.rs:345-353: ilog2(T), one more when T is not a power of two"""
    T = total_bits(nb)
    return T.bit_length() - 1 + (1 if T & (T - 1) else 0)


def _distinct(values):
    """without the repeats that one and two blocks give (T - 1 = 1, 2^T = 4, ...)"""
    return tuple(dict.fromkeys(values))


def AMOUNTS(nb):
    T = total_bits(nb)
    return _distinct((0, 1, BITS, BITS + 1, T - 1, T + 3))       # BITS: a pure block move; T + 3 wraps


def MULTIPLIERS(nb):
    """4: a power of two.  5: set bits at even positions only, so the shift by 1 inside the blocks must not be
    computed; 10 the mirror case.  2^T + 3: bits beyond T are dropped.  2^T: trivial zero here (the product modulo
    2^T), where the reference shifts by T mod T."""
    T = total_bits(nb)
    return _distinct((0, 1, 4, 3, 5, 10, 2 ** T - 1, 2 ** T + 3, 2 ** T))


def TRIVIAL_AMOUNT(nb):
    return total_bits(nb) - 1


@dataclass(frozen=True)
class Case:
    op: str
    variant: str
    nb: int
    clear: int          # the clear amount or multiplier; -1: the amount is encrypted
    seed: int

    @property
    def id(self):
        return f"{self.op}-{self.variant}-b{self.nb}" + ("" if self.clear < 0 else f"-by{self.clear}")

    @property
    def rows(self):
        return len(amount_rows(self.nb, self.seed)) if self.op in ENCRYPTED_OPS else 2 * K


def amount_rows(nb, seed):
    """the encrypted amounts of a case, row by row: the distinct crafted ones, then random ones (two at least) up to
    a whole number of batches"""
    T, s = total_bits(nb), control_bits(nb)
    crafted = []
    for a in (0, 1, T - 1, T, 2 ** s - 1):
        if a not in crafted and a < 2 ** T:           # it fits in the operand
            crafted.append(a)
    n = -(-(len(crafted) + 2) // K) * K
    rng = np.random.default_rng(seed + 13)
    return crafted + [int(x) for x in rng.integers(0, 2 ** T, n - len(crafted))]


def _cases():
    out, seed = [], 900
    for nb in BLOCKS:
        for op in SCALAR_OPS:
            for clear in AMOUNTS(nb):
                for variant in VARIANTS:
                    out.append(Case(op, variant, nb, clear, seed))
                    seed += 1
        for op in ENCRYPTED_OPS:
            for variant in VARIANTS + ("trivial_amount",):
                out.append(Case(op, variant, nb, -1, seed))
                seed += 1
        for clear in MULTIPLIERS(nb):
            for variant in VARIANTS:
                out.append(Case("scalar_mul", variant, nb, clear, seed))
                seed += 1
    return out


CASES = _cases()


# ---- plaintext side ---------------------------------------------------------------------------------------------
def _trivial(case):
    return case.variant in ("trivial", "trivial_amount")


def values(case):
    """{"lhs": [rows] values, "rhs": [rows] amounts (encrypted ones only)} as Python ints, the trivial digits in
    place.  Rows 0 .. 2 of the value: all ones, one, the top and the bottom bit; the rest random."""
    nb, M = case.nb, MSG ** case.nb
    rng = np.random.default_rng(case.seed)
    lhs = [int(x) for x in rng.integers(0, M, case.rows)]
    lhs[0], lhs[1], lhs[2] = M - 1, 1, M // 2 + 1
    if _trivial(case):
        for j in TRIVIAL(nb):
            lhs = [_set_digit(v, j, trivial_digit(nb, j, 0)) for v in lhs]
    rhs = []
    if case.op in ENCRYPTED_OPS:
        rhs = [TRIVIAL_AMOUNT(nb)] * case.rows if case.variant == "trivial_amount" else amount_rows(nb, case.seed)
    return {"lhs": lhs, "rhs": rhs}


def _rotl(v, a, T):
    a %= T
    return ((v << a) | (v >> (T - a))) & (2 ** T - 1)


def plain(op, v, a, nb):
    """the plain semantics.  Clear amounts: a mod T.  Encrypted amounts: a mod 2^s, so a shift gives 0 once that
    is T or more, and a rotation goes by (a mod 2^s) mod T."""
    T = total_bits(nb)
    M = 2 ** T
    if op == "scalar_mul":
        return (v * a) % M
    a = a % T if op in SCALAR_OPS else a % 2 ** control_bits(nb)
    kind = op[len("scalar_"):] if op in SCALAR_OPS else op
    if kind == "left_shift":
        return (v << a) % M
    if kind == "right_shift":
        return v >> a
    return _rotl(v, a if kind == "rotate_left" else T - a % T, T)


def expected(case):
    v = values(case)
    amounts = v["rhs"] or [case.clear] * case.rows
    return [plain(case.op, x, a, case.nb) for x, a in zip(v["lhs"], amounts)]


# ---- ciphertext side --------------------------------------------------------------------------------------------
def encrypt(ck, case):
    """Host batches of case.rows rows: {"lhs": [batches to add up], "rhs": [...] or []}; a clean operand is one
    batch, a dirty one ADDENDS batches whose plaintexts add up to the operand modulo MSG ** nb.  The encryption
    randomness depends on the case alone."""
    from tfhe_mi355 import integer

    ck._enc_counter = case.seed << 8
    cks, M = integer.ClientKey(ck, case.nb), MSG ** case.nb
    v = values(case)
    rng = np.random.default_rng(case.seed + 7)
    enc = {}
    for name in ("lhs", "rhs"):
        if not v[name]:
            enc[name] = []
            continue
        parts = [np.asarray(v[name], dtype=np.uint64)]
        if case.variant == "dirty":
            extra = rng.integers(0, M, (ADDENDS - 1, case.rows), dtype=np.uint64)
            parts = [(parts[0] + np.uint64(ADDENDS - 1) * np.uint64(M) - extra.sum(axis=0)) % np.uint64(M)] + list(extra)
        enc[name] = [cks.encrypt(p) for p in parts]
    return enc


def operands(case, sks, enc, b):
    """(value, amount or None) of rows [b K, (b + 1) K) in the residency of `sks`, as the case hands them to the
    operation; the host batches of `enc` stay untouched"""
    def operand(name, index):
        if not enc[name]:
            return None
        x = [sks.to_device(batch_rows(e, b)) for e in enc[name]]
        for t in x[1:]:
            sks.unchecked_add_assign(x[0], t)
        if index == 0 and _trivial(case):
            for j in TRIVIAL(case.nb):
                sks._set_trivial(x[0], j, trivial_digit(case.nb, j, 0))
        if index == 1 and case.variant == "trivial_amount":
            for j in range(case.nb):
                sks._set_trivial(x[0], j, (TRIVIAL_AMOUNT(case.nb) // MSG ** j) % MSG)
        return x[0]

    return operand("lhs", 0), operand("rhs", 1)


def method(case, assign):
    return ("unchecked_" if case.variant == "unchecked" else "") + case.op + ("_assign" if assign else "") + "_parallelized"


def apply(case, sks, lhs, rhs, b):
    """The case's operation on operands in the residency of `sks`: batch 0 through the form that returns the result,
    every other batch through the _assign form.  sks.pbs_count and sks.launches count the call alone."""
    sks.pbs_count = sks.launches = 0
    second = rhs if case.op in ENCRYPTED_OPS else case.clear
    if b == 0:
        return getattr(sks, method(case, False))(lhs, second)
    assert getattr(sks, method(case, True))(lhs, second) is None
    return lhs


def run(case, sks, enc, b):
    """The case on rows [b K, (b + 1) K) on `sks` (host or device path).  Returns (result, value operand, amount
    operand) in the key's residency."""
    lhs, rhs = operands(case, sks, enc, b)
    return apply(case, sks, lhs, rhs, b), lhs, rhs


# ---- the expected counts: the reference's loops on two flags per block ---------------------------------------------
# a block is (trivial, zero): a trivial ciphertext or not, of degree 0 or not
ZERO = (True, True)              # a trivial zero
FRESH = (False, False)


def _and(*blocks):
    return all(t for t, _ in blocks), all(z for _, z in blocks)


def _lut(s_requests, *sources):
    """a LUT application on the sum of `sources`, queued on the pass: the result block (no LUT here has degree 0)"""
    t = all(t for t, _ in sources)
    s_requests.append(t)
    return t, False


def _rotate_right(blocks, n):
    n %= len(blocks)
    return blocks[len(blocks) - n:] + blocks[:len(blocks) - n]


def _rotate_left(blocks, n):
    n %= len(blocks)
    return blocks[n:] + blocks[:n]


def _scalar_shift(requests, ct, kind, amount):
    """unchecked_scalar_{left,right}_shift_assign_parallelized (scalar_shift.rs:553-647, 246-368) and
    unchecked_scalar_rotate_{left,right}_assign_parallelized (scalar_rotate.rs:611-681, 272-350): rotate the blocks,
    trivial zeros where a shift wrapped, then one pass over windows of two blocks, the end block of a shift apart in
    the same rayon::join.  The LUT applications go on `requests`."""
    nb = len(ct)
    amount %= BITS * nb
    if amount == 0:
        return list(ct)
    rotations, within = divmod(amount, BITS)
    if kind == "left_shift":
        blocks = _rotate_right(ct, rotations)
        blocks[:rotations] = [ZERO] * rotations
        if within == 0:
            return blocks
        last = _lut(requests, blocks[rotations])
        partial = [_lut(requests, w0, w1) for w0, w1 in zip(blocks[rotations:], blocks[rotations + 1:])]
        return blocks[:rotations] + [last] + partial
    if kind == "right_shift":
        blocks = _rotate_left(ct, rotations)
        blocks[nb - rotations:] = [ZERO] * rotations
        if within == 0:
            return blocks
        inner = blocks[:nb - rotations]
        partial = [_lut(requests, w0, w1) for w0, w1 in zip(inner, inner[1:])]
        last = _lut(requests, blocks[nb - rotations - 1])
        return partial + [last] + blocks[nb - rotations:]
    blocks = _rotate_right(ct, rotations) if kind == "rotate_left" else _rotate_left(ct, rotations)
    if within == 0:
        return blocks
    giver = (lambda i: nb - 1 if i == 0 else i - 1) if kind == "rotate_left" else (lambda i: (i + 1) % nb)
    return [_lut(requests, blocks[i], blocks[giver(i)]) for i in range(nb)]


def _barrel(s, ct, shift, kind):
    """barrel_shifter (shift.rs:321-473)"""
    nb = len(ct)
    T, n = BITS * nb, control_bits(nb)
    requests = []
    bits = [_lut(requests, ct[j]) for j in range(nb) for _ in range(BITS)]          # extract_all_bits
    shift_bits = [_lut(requests, shift[i // BITS]) for i in range(n)]             # extract_n_bits, joined
    s.layer(requests)
    a = bits
    for d, shift_bit in enumerate(shift_bits):
        b = list(a)
        if kind in ("left_shift", "rotate_left"):
            b = _rotate_right(b, 1 << d)
            if kind == "left_shift":
                b[:1 << d] = [ZERO] * (1 << d)
        else:
            b = _rotate_left(b, 1 << d)
            if kind == "right_shift":
                b[T - (1 << d):] = [ZERO] * (1 << d)
        requests = []
        a = [_lut(requests, b[i], a[i], shift_bit) for i in range(T)]
        s.layer(requests)
    requests = []
    out = [_lut(requests, *a[j * BITS:(j + 1) * BITS]) for j in range(nb)]           # recomposition, message_extract
    s.layer(requests)
    return out


def _blockshift(ct, shift):
    """radix/scalar_mul.rs:345-355"""
    out = _rotate_right(ct, shift)
    out[:min(shift, len(ct))] = [ZERO] * min(shift, len(ct))
    return out


def _trivial_flags(ct):
    return [t for t, _ in ct]


def _add_clean(s, lhs, rhs):
    """add_assign_parallelized (add.rs:206-242) on operands with empty carries"""
    out = _single_carry(s, [a and b for a, b in zip(_trivial_flags(lhs), _trivial_flags(rhs))])
    return [(t, False) for t in out]


def _sum(s, terms):
    """unchecked_sum_ciphertexts_vec_parallelized (add.rs:783-960): chunks of FILL terms are added up over the
    window of blocks where a term's degree is not 0, the messages of the window and its carries (all but the top
    block's) are extracted in one pass over all chunks, and (message, carry rotated up one block) go back on the
    list; the last FILL or fewer terms are added up, split once more and added with carry propagation"""
    if not terms:
        return None
    if len(terms) == 1:
        return terms[0]
    if len(terms) == 2:
        return _add_clean(s, terms[0], terms[1])
    nb = len(terms[0])
    terms = [list(t) for t in terms]
    while len(terms) > FILL:
        nchunks = len(terms) // FILL
        rest = terms[nchunks * FILL:]
        requests, new = [], []
        for c in range(nchunks):
            chunk = terms[c * FILL:(c + 1) * FILL]
            total = list(chunk[0])
            first_where, last_where = nb - 1, 0
            for a in chunk[1:]:
                nz = [j for j in range(nb) if not a[j][1]]
                first_add, last_add = (nz[0], nz[-1]) if nz else (nb, nb - 1)
                first_where, last_where = min(first_where, first_add), max(last_where, last_add)
                for j in range(first_add, last_add + 1):
                    total[j] = _and(total[j], a[j])
            message, carry = list(total), [ZERO] * nb
            for j in range(first_where, last_where + 1):
                message[j] = _lut(requests, total[j])
            end = last_where - 1 if last_where == nb - 1 else last_where
            for j in range(first_where, end + 1):
                carry[j] = _lut(requests, total[j])
            new += [message, _rotate_right(carry, 1)]
        s.layer(requests)
        terms = new + rest
    total = [_and(*(t[j] for t in terms)) for j in range(nb)]
    requests = []
    message = [_lut(requests, x) for x in total]
    carry = [ZERO] + [_lut(requests, x) for x in total[:-1]]
    s.layer(requests)
    return _add_clean(s, message, carry)


def _scalar_mul(s, ct, scalar):
    """unchecked_scalar_mul_assign_parallelized (scalar_mul.rs:330-397); 2^e with e >= T: trivial zero here"""
    nb = len(ct)
    T = BITS * nb
    if scalar == 0:
        return [ZERO] * nb
    if scalar == 1:
        return ct
    if scalar & (scalar - 1) == 0:
        e = scalar.bit_length() - 1
        if e >= T:
            return [ZERO] * nb
        requests = []
        out = _scalar_shift(requests, ct, "left_shift", e)
        s.layer(requests)
        return out
    scalar_bits = [int(c) for c in reversed(bin(scalar)[2:])]
    has_at_least_one_set = [any(scalar_bits[w::BITS]) for w in range(BITS)]
    requests = []                # the par_iter over the shifts: one pass
    preshifted = [_scalar_shift(requests, ct, "left_shift", w) if has_at_least_one_set[w] else [ZERO] * nb
                  for w in range(BITS)]
    s.layer(requests)
    out = _sum(s, [_blockshift(preshifted[i % BITS], i // BITS) for i, bit in enumerate(scalar_bits[:T]) if bit])
    return out if out is not None else [ZERO] * nb


def value_flags(case):
    """the value operand as the operation meets it, before a default form's preamble"""
    nb = case.nb
    if _trivial(case):
        return [(j in TRIVIAL(nb), trivial_digit(nb, j, 0) == 0 and j in TRIVIAL(nb)) for j in range(nb)]
    return [FRESH] * nb


def shadow(case):
    """(pbs_count, launches) of one batch of K rows"""
    nb, op, s = case.nb, case.op, Shadow()
    ct = value_flags(case)
    shift = [(case.variant == "trivial_amount", False)] * nb
    if case.variant == "dirty":                       # the default forms' preamble
        _full_propagate(s, [False] * nb)
        if op in ENCRYPTED_OPS:
            _full_propagate(s, [False] * nb)
    if op in SCALAR_OPS:
        requests = []
        _scalar_shift(requests, ct, op[len("scalar_"):], case.clear)
        s.layer(requests)
    elif op in ENCRYPTED_OPS:
        _barrel(s, ct, shift, op)
    else:
        _scalar_mul(s, ct, case.clear)
    return s.pbs, s.launches


# ---- the sum's restated loops against the recorded counts of integer_dag_cases -------------------------------------
def shadow_of_dag_sum(nb, nterms):
    """the `sum` case of integer_dag_cases (run: term i block-shifted by _term_shape, its top block cleared to a
    trivial zero for every fourth) through _sum above"""
    from integer_dag_cases import Case as DagCase, _term_shape

    case, s, terms = DagCase("sum", nb, 0, nterms), Shadow(), []
    for i in range(nterms):
        shift, clear = _term_shape(case, i)
        t = _blockshift([FRESH] * nb, shift) if shift else [FRESH] * nb
        if clear:
            t[nb - 1] = ZERO
        terms.append(t)
    _sum(s, terms)
    return s.pbs, s.launches


# ---- a set with carry_modulus < message_modulus ---------------------------------------------------------------------
SET_3_2 = "PARAM_MESSAGE_3_CARRY_2_KS_PBS"
BLOCKS_3_2 = 2                   # 3 bits per block: T = 6, s = 3; 6 + 3 + 3 * 6 + 2 = 29 LUTs per row in 5 passes
