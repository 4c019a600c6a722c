"""The gate batch shared by test_boolean.py (on RefEngine32) and test_boolean_gpu.py (on the GPU and,
for bit-exact parity, on RefEngine32 through the same ServerKey code): every binary gate on all four
inputs, NOT on two, MUX on eight, and gates() with all six opcodes in one batch."""
import numpy as np

from tfhe_mi355 import boolean as B

A4 = np.array([0, 0, 1, 1], dtype=bool)
B4 = np.array([0, 1, 0, 1], dtype=bool)
C8 = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=bool)
T8 = np.array([0, 0, 1, 1, 0, 0, 1, 1], dtype=bool)
E8 = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=bool)
MIX_OPS = np.array([B.AND, B.NAND, B.NOR, B.OR, B.XOR, B.XNOR], dtype=np.uint8)
MIX_A = np.array([1, 1, 0, 0, 1, 0], dtype=bool)
MIX_B = np.array([1, 0, 0, 1, 0, 0], dtype=bool)

TRUTH = {
    "and": lambda a, b: a & b, "nand": lambda a, b: ~(a & b), "nor": lambda a, b: ~(a | b),
    "or": lambda a, b: a | b, "xor": lambda a, b: a ^ b, "xnor": lambda a, b: ~(a ^ b),
}


def gate_inputs(cks):
    """Encrypted operands (one encryption each, so every engine sees the same ciphertext words)."""
    return {"a4": cks.encrypt(A4), "b4": cks.encrypt(B4), "n2": cks.encrypt([False, True]),
            "c8": cks.encrypt(C8), "t8": cks.encrypt(T8), "e8": cks.encrypt(E8),
            "ma": cks.encrypt(MIX_A), "mb": cks.encrypt(MIX_B)}


def run_gate_batch(sk, x):
    """{name: (BoolBatch, expected bools)} of the whole batch under ServerKey `sk`."""
    out = {}
    for name in B.GATE_NAMES:
        fn = getattr(sk, name + "_" if name in ("and", "or") else name)
        out[name] = (fn(x["a4"], x["b4"]), TRUTH[name](A4, B4))
    out["not"] = (sk.not_(x["n2"]), np.array([True, False]))
    out["mux"] = (sk.mux(x["c8"], x["t8"], x["e8"]), np.where(C8, T8, E8))
    exp = np.array([TRUTH[B.GATE_NAMES[o]](np.bool_(a), np.bool_(b)) for o, a, b in zip(MIX_OPS, MIX_A, MIX_B)])
    out["gates"] = (sk.gates(MIX_OPS, x["ma"], x["mb"]), exp)
    return out
