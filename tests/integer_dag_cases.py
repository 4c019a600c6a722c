"""Case list of the radix integer DAG tests, shared by test_integer_dag.py (host path, oracle engine)
and test_integer_dag_gpu.py (device path against the host path).

Every case runs PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8 (tiny keys, lower noise: decryption
still holds) on K = 3 operand rows.  A case fixes its seed, block count, values and the DAG's expected
pbs_count and launches; those two were recorded once from the host run and depend only on the degrees and
noise levels of the operands, never on the data or on the engine.
"""
from dataclasses import dataclass

import numpy as np

SEED = 11          # ClientKey seed: the GPU key and the oracle-engine key are built from the same one
K = 3
BLOCKS = (1, 2, 3, 5, 8)
MSG = 4
FILL = 5           # (16 - 1) // (4 - 1) terms fill a 2_2 block


def params():
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    return P.with_(lwe_dimension=8)


def keys(engine=None, seed=SEED, parameters=None):
    """(shortint ClientKey, integer ServerKey) on `engine` (None: the GPU engine on device 0)."""
    from tfhe_mi355 import integer, shortint

    ck = shortint.ClientKey(parameters or params(), seed)
    return ck, integer.ServerKey(shortint.ServerKey(ck, engine=engine))


@dataclass(frozen=True)
class Case:
    kind: str
    nb: int
    seed: int
    nterms: int = 0

    @property
    def id(self):
        return f"{self.kind}{self.nterms or ''}-b{self.nb}"

    @property
    def inputs(self):
        return {"mul": 2, "add": 2, "dirty_add": 7, "dirty_mul": 7, "propagate": 3, "trivial_mul": 2,
                "sum": self.nterms, "trivial_sum": FILL + 1}[self.kind]


def _cases():
    out, seed = [], 100
    for nb in BLOCKS:
        for kind in ("mul", "add", "dirty_add", "dirty_mul", "propagate", "trivial_mul", "trivial_sum"):
            out.append(Case(kind, nb, seed))
            seed += 1
        for nterms in (1, 2, 3, 2 * FILL + 1):
            out.append(Case("sum", nb, seed, nterms))
            seed += 1
    return out


CASES = _cases()

# case id -> (pbs_count, launches) of the whole case on K = 3 rows, from the host run
EXPECTED = {
    "mul-b1": (9, 3), "add-b1": (6, 2), "dirty_add-b1": (24, 8), "dirty_mul-b1": (27, 9),
    "propagate-b1": (9, 3), "trivial_mul-b1": (9, 3), "trivial_sum-b1": (12, 4),
    "sum1-b1": (0, 0), "sum2-b1": (6, 2), "sum3-b1": (9, 3), "sum11-b1": (15, 4),
    "mul-b2": (36, 5), "add-b2": (15, 3), "dirty_add-b2": (63, 11), "dirty_mul-b2": (84, 13),
    "propagate-b2": (24, 4), "trivial_mul-b2": (57, 9), "trivial_sum-b2": (33, 5),
    "sum1-b2": (0, 0), "sum2-b2": (15, 3), "sum3-b2": (24, 4), "sum11-b2": (42, 5),
    "mul-b3": (78, 7), "add-b3": (27, 4), "dirty_add-b3": (111, 14), "dirty_mul-b3": (162, 17),
    "propagate-b3": (42, 5), "trivial_mul-b3": (93, 12), "trivial_sum-b3": (57, 6),
    "sum1-b3": (0, 0), "sum2-b3": (27, 4), "sum3-b3": (42, 5), "sum11-b3": (72, 6),
    "mul-b5": (192, 8), "add-b5": (54, 5), "dirty_add-b5": (216, 17), "dirty_mul-b5": (354, 20),
    "propagate-b5": (81, 6), "trivial_mul-b5": (255, 14), "trivial_sum-b5": (108, 7),
    "sum1-b5": (0, 0), "sum2-b5": (54, 5), "sum3-b5": (81, 6), "sum11-b5": (135, 7),
    "mul-b8": (474, 9), "add-b8": (99, 5), "dirty_add-b8": (387, 17), "dirty_mul-b8": (762, 21),
    "propagate-b8": (144, 6), "trivial_mul-b8": (600, 15), "trivial_sum-b8": (189, 7),
    "sum1-b8": (0, 0), "sum2-b8": (99, 5), "sum3-b8": (144, 6), "sum11-b8": (234, 7),
}


def values(case):
    """[inputs][K] plaintext operands.  Rows of input 0: all digits message_modulus - 1, zero, and a value
    whose middle digits are zero; the all-ones row is kept in every input, and row 2 of input 1 is the
    complement of input 0's (their sum generates a carry in block 0 that every other block propagates: the
    longest chain of the prefix sum).  The rest is random."""
    M = MSG ** case.nb
    v = np.random.default_rng(case.seed).integers(0, M, (case.inputs, K), dtype=np.uint64)
    v[:, 0] = M - 1
    v[0, 1] = 0
    v[0, 2] = (3 * MSG ** (case.nb - 1) + 1) % M if case.nb > 1 else 2
    if case.inputs > 1:
        v[1, 2] = M - v[0, 2]
    return v


def encrypt(ck, case):
    """Host RadixBatch per input; the encryption randomness depends on the case alone."""
    from tfhe_mi355 import integer

    ck._enc_counter = case.seed << 8
    cks = integer.ClientKey(ck, case.nb)
    return [cks.encrypt(v) for v in values(case)]


def decrypt(ck, case, rb):
    from tfhe_mi355 import integer

    return integer.ClientKey(ck, case.nb).decrypt(rb)


def _term_shape(case, i):
    """(blockshift, clear the top block) of term i of a sum: odd terms get leading trivial zeros, every
    fourth a trailing one, so the first_add / last_add windows differ between the terms of a chunk."""
    shift = i % case.nb if i % 2 else 0
    return shift, (i % 4 == 2 and case.nb > 1)


TRIVIAL_MID, TRIVIAL_LOW = 5, 2   # trivial block values of trivial_mul: one with a carry, one without


def _trivial_blocks(case):
    blocks = {case.nb // 2: TRIVIAL_MID}
    if case.nb >= 3:
        blocks[0] = TRIVIAL_LOW
    return blocks


def expected(case):
    """The K plaintext results, modulo message_modulus ** blocks."""
    v = [[int(x) for x in row] for row in values(case)]
    M = MSG ** case.nb
    res = []
    for r in range(K):
        col = [row[r] for row in v]
        if case.kind == "mul":
            e = col[0] * col[1]
        elif case.kind == "add":
            e = col[0] + col[1]
        elif case.kind == "dirty_add":
            e = sum(col)
        elif case.kind == "dirty_mul":
            e = (sum(col[:4]) % M) * (sum(col[4:]) % M)
        elif case.kind == "propagate":
            e = sum(col)
        elif case.kind == "trivial_mul":
            a = col[0]
            for j, t in _trivial_blocks(case).items():
                a += (t - (a // MSG ** j) % MSG) * MSG ** j
            e = a * col[1]
        elif case.kind == "trivial_sum":
            e = sum(col)
        else:
            e = 0
            for i, x in enumerate(col):
                shift, clear = _term_shape(case, i)
                x = (x * MSG ** shift) % M
                e += x % (M // MSG) if clear else x
        res.append(e % M)
    return np.asarray(res, dtype=np.uint64)


def run(case, sks, enc):
    """The case's DAG on `sks` (host or device path) from the host batches `enc`, which stay untouched;
    returns the result in the key's residency.  sks.pbs_count and sks.launches count the case alone."""
    x = [sks.to_device(e.clone()) for e in enc]
    sks.pbs_count = sks.launches = 0
    kind = case.kind
    if kind == "mul":
        return sks.mul_parallelized(x[0], x[1])
    if kind == "add":
        sks.add_assign_parallelized(x[0], x[1])
        return x[0]
    if kind in ("dirty_add", "dirty_mul"):
        for t in x[1:4]:                                  # three adds: degree 12
            sks.unchecked_add_assign(x[0], t)
        for t in x[5:7]:                                  # two adds: degree 9
            sks.unchecked_add_assign(x[4], t)
        if kind == "dirty_mul":
            return sks.mul_parallelized(x[0], x[4])
        sks.add_assign_parallelized(x[0], x[4])           # both operands take full_propagate
        return x[0]
    if kind == "propagate":
        sks.unchecked_add_assign(x[0], x[1])
        sks.unchecked_add_assign(x[0], x[2])
        sks.full_propagate(x[0])
        return x[0]
    if kind == "trivial_mul":
        for j, t in _trivial_blocks(case).items():
            sks._set_trivial(x[0], j, t)
        return sks.mul_parallelized(x[0], x[1])
    if kind == "trivial_sum":                             # one chunk of trivial-zero operands among the terms
        zeros = [sks.create_trivial_zero(K, case.nb) for _ in range(FILL)]
        return sks.unchecked_sum_ciphertexts_vec(zeros + x)
    terms = []
    for i, t in enumerate(x):
        shift, clear = _term_shape(case, i)
        if shift:
            t = sks.blockshift(t, shift)
        if clear:
            sks._set_trivial(t, case.nb - 1, 0)
        terms.append(t)
    return sks.unchecked_sum_ciphertexts_vec(terms)


# ---- parameter-set sweep (one set per child process: see test_integer_dag.py) --------------------------
SWEEP_BLOCKS = 3
SWEEP_OPS = ("mul_parallelized", "add_assign_parallelized", "dirty_add")


def sweep_set(name):
    """mul_parallelized, add_assign_parallelized and an add of operands with carries on the set `name` at
    lwe_dimension = 8, 3 blocks, 3 ciphertexts, host path, oracle engine.  Per operation: "ok" (decrypts to
    the integer answer), "wrong", or the message of the NotImplementedError; and the seconds it took."""
    import time

    from oracle.oracle import OracleEngine
    from tfhe_mi355 import integer
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[name].with_(lwe_dimension=8)
    ck, sks = keys(OracleEngine(P, threads=4), parameters=P)
    cks = integer.ClientKey(ck, SWEEP_BLOCKS)
    m = P.message_modulus
    M = m ** SWEEP_BLOCKS
    v = np.random.default_rng(7).integers(0, M, (4, K), dtype=np.uint64)
    v[:, 0] = M - 1
    v[0, 2] = (m - 1) * m ** (SWEEP_BLOCKS - 1) + 1      # zero digit in the middle
    v[1, 2] = M - v[0, 2]                                # carry generated in block 0, propagated by the rest
    out = {}
    for op in SWEEP_OPS:
        e = [cks.encrypt(x) for x in v]
        t = time.perf_counter()
        try:
            if op == "mul_parallelized":
                res, exp = sks.mul_parallelized(e[0], e[1]), (v[0] * v[1]) % np.uint64(M)
            elif op == "add_assign_parallelized":
                sks.add_assign_parallelized(e[0], e[1])
                res, exp = e[0], (v[0] + v[1]) % np.uint64(M)
            else:
                sks.unchecked_add_assign(e[0], e[2])
                sks.unchecked_add_assign(e[1], e[3])
                sks.add_assign_parallelized(e[0], e[1])
                res, exp = e[0], v.sum(axis=0) % np.uint64(M)
            verdict = "ok" if np.array_equal(cks.decrypt(res), exp) else "wrong"
        except NotImplementedError as ex:
            verdict = f"NotImplementedError: {ex}"
        out[op] = {"verdict": verdict, "seconds": time.perf_counter() - t, "pbs_count": sks.pbs_count}
    return out


if __name__ == "__main__":
    import json
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tfhe-rs-odd_amd")]
    print(json.dumps(sweep_set(sys.argv[1])))
