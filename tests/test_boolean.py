"""boolean module on the CPU: parameter sets, the RefEngine32 restatement pinned to the oracle, the gate
semantics and the plain / trivial shortcuts (no GPU: ServerKey over RefEngine32)."""
import dataclasses

import numpy as np
import pytest

from boolean_cases import gate_inputs, run_gate_batch
from boolean_reference import (F, RefEngine32, T, conversion_edge_fractions, conversion_expected, decompose32,
                               from_fraction, widen)
from pbs_edge_inputs32 import crafted_case32
from tfhe_mi355 import boolean as B

SHAPES = [(512, 2, 3, 6), (1024, 2, 2, 10), (1024, 1, 4, 5), (1024, 1, 3, 7)]  # N, k, L, reference base_log


# ---- 1. parameters -------------------------------------------------------------------------------
def test_parameter_sets_equal_the_references():
    # boolean/parameters/mod.rs:123-192: (n, k, N, lwe std, glwe std, pbs B, pbs L, ks B, ks L, key choice)
    ref = {
        "DEFAULT_PARAMETERS": (722, 2, 512, 0.000013071021089943935, 0.00000004990272175010415, 6, 3, 3, 4, "Small"),
        "DEFAULT_PARAMETERS_KS_PBS": (664, 2, 512, 0.00003808282923459771, 0.00000004990272175010415, 6, 3, 3, 4,
                                      "Big"),
        "PARAMETERS_ERROR_PROB_2_POW_MINUS_165": (767, 2, 1024, 0.000005104350373791501,
                                                  0.0000000009313225746154785, 10, 2, 3, 5, "Small"),
        "PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS": (700, 1, 1024, 0.0000196095987892077,
                                                         0.00000004990272175010415, 5, 4, 2, 7, "Big"),
        "TFHE_LIB_PARAMETERS": (630, 1, 1024, 0.000030517578125, 0.00000002980232238769531, 7, 3, 2, 8, "Small"),
    }
    assert len(B.PARAMETER_SETS) == 5
    for name, v in ref.items():
        p = getattr(B, name)
        assert p.name == name
        assert (p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.lwe_modular_std_dev, p.glwe_modular_std_dev,
                p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.encryption_key_choice) == v
        assert p.pbs_order == (1 if v[-1] == "Small" else 0)
        assert p.ciphertext_words == (p.lwe_dimension if p.pbs_order else p.big_lwe_dimension) + 1
    assert (B.PLAINTEXT_TRUE, B.PLAINTEXT_FALSE) == (1 << 29, 7 << 29) == (T, F)


# ---- 2. reference keyswitch = the oracle's on words shifted left by 32 ---------------------------
@pytest.mark.parametrize("base_log,level", [(3, 4), (3, 5), (2, 7), (2, 8)])
def test_reference_keyswitch_equals_oracle(orc, base_log, level):
    rng = np.random.default_rng(base_log * 10 + level)
    in_dim, out_dim, count = 37, 29, 5
    ksk = rng.integers(0, 1 << 32, (in_dim * level, out_dim + 1), dtype=np.uint32)
    x = rng.integers(0, 1 << 32, (count, in_dim + 1), dtype=np.uint32)
    x[0, :8] = [0, 1 << 31, 0xFFFFFFFF, 1 << (31 - base_log * level), (1 << (32 - base_log * level)) - 1,
                0x80000000 >> base_log, 0x7FFFFFFF, 1]
    got = RefEngine32(B.DEFAULT_PARAMETERS).keyswitch_u32(x, ksk, in_dim, out_dim, base_log, level)
    exp = orc.keyswitch(widen(ksk).ravel(), in_dim, out_dim, base_log, level, widen(x))
    assert not (exp & np.uint64(0xFFFFFFFF)).any()  # digits identical, the sum linear: low halves stay zero
    assert np.array_equal(got, (exp >> np.uint64(32)).astype(np.uint32))


def test_reference_digits_equal_the_u64_decomposer(orc):
    rng = np.random.default_rng(1)
    for base_log, level in [(6, 3), (10, 2), (5, 4), (7, 3), (3, 4), (2, 8), (15, 2)]:
        w = rng.integers(0, 1 << 32, 64, dtype=np.uint32)
        w[:4] = [0, 1 << 31, 0xFFFFFFFF, (1 << 31) - 1]
        d = decompose32(w, base_log, level)
        for i, x in enumerate(w):
            e = [v - (1 << 64) if v >> 63 else v for v in orc.decompose(int(x) << 32, base_log, level)]
            assert [int(v) for v in d[i]] == e, (base_log, level, hex(int(x)))


# ---- 3. reference CMUX pinned to the oracle ---------------------------------------------------------
@pytest.mark.parametrize("N,k,L,base_log", SHAPES)
def test_reference_cmux_within_one_of_the_oracle(orc, N, k, L, base_log):
    """One external-product step (one-element key, rotation by X^N: ct1 = -2 acc) from a random u32
    accumulator under a random GGSW.  With the low halves zero the digits and spectra of the u64 oracle
    coincide with the u32 computation, X64 / 2^32 = fr 2^32 +- 2^-33, so any rounding of it is within 1
    of rint(fr 2^32): every coefficient within 1 mod 2^32, none exempt."""
    rng = np.random.default_rng(N + 7 * k + L)
    p = dataclasses.replace(B.DEFAULT_PARAMETERS, lwe_dimension=1, glwe_dimension=k, polynomial_size=N,
                            pbs_base_log=base_log, pbs_level=L)
    ggsw = rng.integers(0, 1 << 32, L * (k + 1) * (k + 1) * N, dtype=np.uint32)
    acc = rng.integers(0, 1 << 32, (k + 1) * N, dtype=np.uint32)
    ref = RefEngine32(p)
    ref.upload_bootstrap_key_u32(ggsw)
    got = ref.blind_rotate_u32(np.array([[1 << 31, 0]], dtype=np.uint32), acc)[0]
    f64 = orc.FourierBsk(widen(ggsw), 1, k, N, base_log, L)
    exp64 = f64.blind_rotate(np.array([[1 << 63, 0]], dtype=np.uint64), widen(acc))[0]
    exp = ((exp64 + np.uint64(1 << 31)) >> np.uint64(32)).astype(np.uint32)
    diff = (got.astype(np.int64) - exp.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
    assert np.abs(diff).max() <= 1, np.abs(diff).max()
    assert not np.array_equal(got, acc)  # the step did something
    # the same step through the stand-alone external product entry
    step = ref.external_product(f64.fourier(), acc, (np.uint32(0) - acc * np.uint32(2)).astype(np.uint32))
    assert np.array_equal(step, got)


def test_reference_crafted_first_cmux_digits(orc):
    """The crafted n = 1 case decomposes the worst-case words: its u32 digits are the u64 decomposer's for
    word << 32 (ties, carries, the +2^(B-1) digit, the rounding overflow)."""
    for N, k, L, base_log in SHAPES:
        cts, lut, D = crafted_case32(base_log, L, N, k, seed=3)
        d = decompose32(D, base_log, L)
        half = 1 << (base_log - 1)
        assert d.max() == half and d.min() <= -(half - 1)
        for x, row in zip(D.ravel()[:64], d.reshape(-1, L)[:64]):
            e = [v - (1 << 64) if v >> 63 else v for v in orc.decompose(int(x) << 32, base_log, L)]
            assert [int(v) for v in row] == e


# ---- 4. conversion edges ----------------------------------------------------------------------------
def test_reference_conversion_edges():
    fr = conversion_edge_fractions()
    got = from_fraction(fr)
    assert got[0] == got[1] == 0x80000000  # +-1/2 wrap to the same word
    assert got[2] == 0x80000000 and got[3] == 0x80000000  # 2^31 -+ 2^-21 rounds to 2^31
    assert got[4] == 0
    assert np.array_equal(got, conversion_expected(fr))
    # ties (j + 1/2) 2^-32 round half-even
    assert list(got[5:9]) == [0, 2, 2, 4]
    assert got[11] == 0 and got[12] == 0xFFFFFFFE  # -1/2 -> -0 = 0, -3/2 -> -2


# ---- 5. gate semantics on RefEngine32 with full keys ------------------------------------------------
@pytest.fixture(scope="module", params=["DEFAULT_PARAMETERS", "DEFAULT_PARAMETERS_KS_PBS"])
def ref_keys(request):
    p = getattr(B, request.param)
    cks, sk = B.gen_keys(p, seed=11, device=RefEngine32(p))
    return p, cks, sk


def test_gate_semantics_on_the_reference_engine(ref_keys):
    p, cks, sk = ref_keys
    assert sk.pbs_order == (1 if p.encryption_key_choice == "Small" else 0)
    x = gate_inputs(cks)
    for name, (ct, exp) in run_gate_batch(sk, x).items():
        assert not ct.is_trivial and ct.data.shape == (len(exp), p.ciphertext_words), name
        # failure probability <= 2^-40 per gate: no failure allowed
        assert np.array_equal(cks.decrypt(ct), exp), name


# ---- 6. plain and trivial shortcuts -------------------------------------------------------------------
def kind(out, ct):
    if out.is_trivial:
        return ("trivial", out.value)
    if np.array_equal(out.data, ct.data):
        assert out.data is not ct.data  # a clone, not an alias
        return "clone"
    if np.array_equal(out.data, (np.uint32(0) - ct.data).astype(np.uint32)):
        return "negation"
    return "other"


class NoBootstrapEngine:
    """An engine whose bootstrapping paths must not be reached by a shortcut."""

    def boolean_not(self, ct):
        return (np.uint32(0) - np.asarray(ct, dtype=np.uint32)).astype(np.uint32)

    def boolean_gates(self, *a):
        raise AssertionError("a shortcut ran a bootstrap")

    boolean_mux = boolean_gates


# gate(ct, plain b) -> kind, boolean/engine/mod.rs:969-1039
PLAIN = {
    ("and", True): "clone", ("and", False): ("trivial", False),
    ("nand", True): "negation", ("nand", False): ("trivial", True),
    ("nor", True): ("trivial", False), ("nor", False): "negation",
    ("or", True): ("trivial", True), ("or", False): "clone",
    ("xor", True): "negation", ("xor", False): "clone",
    ("xnor", True): "clone", ("xnor", False): "negation",
}


def test_plain_and_trivial_shortcuts():
    p = B.DEFAULT_PARAMETERS
    sk = B.ServerKey(NoBootstrapEngine(), p)
    rng = np.random.default_rng(5)
    ct = B.BoolBatch(rng.integers(0, 1 << 32, (3, p.ciphertext_words), dtype=np.uint32))
    for (name, b), exp in PLAIN.items():
        fn = getattr(sk, name + "_" if name in ("and", "or") else name)
        # plain bool on either side, and a trivial batch on either side (mod.rs:618-623, 1041-1065)
        for out in (fn(ct, b), fn(b, ct), fn(ct, B.BoolBatch.trivial(b, 3)), fn(B.BoolBatch.trivial(b, 3), ct)):
            assert kind(out, ct) == exp, (name, b)
        # two trivials: the plain truth table (mod.rs:614-617)
        for a in (False, True):
            out = fn(B.BoolBatch.trivial(a, 3), B.BoolBatch.trivial(b, 3))
            want = {"and": a and b, "nand": not (a and b), "nor": not (a or b), "or": a or b, "xor": a != b,
                    "xnor": a == b}[name]
            assert kind(out, ct) == ("trivial", want), (name, a, b)
            # a trivial ciphertext with a plain bool follows the plain rule on the trivial value
            out = fn(B.BoolBatch.trivial(a, 3), b)
            assert out.is_trivial and out.value == want, (name, a, b)
    # NOT (mod.rs:377-389)
    assert kind(sk.not_(ct), ct) == "negation"
    assert kind(sk.not_(B.BoolBatch.trivial(True, 3)), ct) == ("trivial", False)
    # MUX with a trivial condition returns a clone of the chosen operand (mod.rs:472-478)
    th, el = B.BoolBatch(ct.data ^ np.uint32(5)), B.BoolBatch(ct.data ^ np.uint32(9))
    assert kind(sk.mux(B.BoolBatch.trivial(True, 3), th, el), th) == "clone"
    assert kind(sk.mux(False, th, el), el) == "clone"
    assert kind(sk.mux(True, B.BoolBatch.trivial(True, 3), el), ct) == ("trivial", True)


class RecordingEngine(NoBootstrapEngine):
    def __init__(self):
        self.calls = []

    def boolean_gates(self, ops, lhs, rhs, pbs_order):
        self.calls.append((list(ops), np.array(lhs), np.array(rhs)))
        return np.array(lhs)

    def boolean_mux(self, c, t, e, pbs_order):
        self.calls.append(("mux", np.array(c), np.array(t), np.array(e)))
        return np.array(c)


def test_mux_shortcuts_with_trivial_then_or_else():
    """mod.rs:483-500: trivial then -> or(cond, else) / and(not cond, else); trivial else ->
    or(then, not cond) / and(cond, then); each one bootstrap of the cited gate on the cited operands."""
    p = B.DEFAULT_PARAMETERS_KS_PBS
    rng = np.random.default_rng(6)
    w = p.ciphertext_words
    c, t, e = (B.BoolBatch(rng.integers(0, 1 << 32, (2, w), dtype=np.uint32)) for _ in range(3))
    neg = (np.uint32(0) - c.data).astype(np.uint32)
    cases = [
        (lambda sk: sk.mux(c, True, e), B.OR, c.data, e.data),
        (lambda sk: sk.mux(c, B.BoolBatch.trivial(False, 2), e), B.AND, neg, e.data),
        (lambda sk: sk.mux(c, t, True), B.OR, t.data, neg),
        (lambda sk: sk.mux(c, t, B.BoolBatch.trivial(False, 2)), B.AND, c.data, t.data),
    ]
    for run, op, lhs, rhs in cases:
        eng = RecordingEngine()
        run(B.ServerKey(eng, p))
        assert len(eng.calls) == 1
        ops, a, b = eng.calls[0]
        assert ops == [op, op] and np.array_equal(a, lhs) and np.array_equal(b, rhs)
    # both trivial: then decides first, and the trivial else folds into the plain rule (no bootstrap)
    eng = RecordingEngine()
    out = B.ServerKey(eng, p).mux(c, True, False)  # or(cond, false) = cond
    assert eng.calls == [] and kind(out, c) == "clone"
    # all encrypted: one mux call on the three operands
    eng = RecordingEngine()
    B.ServerKey(eng, p).mux(c, t, e)
    assert len(eng.calls) == 1 and eng.calls[0][0] == "mux"
    # convert_into_lwe_ciphertext_32 (mod.rs:573-605): zero mask, body T / F, the order's input size
    for prm in (B.DEFAULT_PARAMETERS, B.DEFAULT_PARAMETERS_KS_PBS):
        sk = B.ServerKey(NoBootstrapEngine(), prm)
        for v, body in ((True, T), (False, F)):
            rows = sk.to_lwe(B.BoolBatch.trivial(v, 2)).data
            assert rows.shape == (2, prm.ciphertext_words)
            assert not rows[:, :-1].any() and (rows[:, -1] == body).all()
        assert sk.to_lwe(c) is c
