#!/usr/bin/env python3
"""What the radix operations with a clear operand of DESIGN.md 5.6e cost on the GPU: scalar_add, scalar_bitand,
scalar_eq, scalar_lt and scalar_max on FheUint32 operands (16 blocks of PARAM_MESSAGE_2_CARRY_2_KS_PBS, the real key)
at K = 256 and K = 1 rows per call, in one process, by the method of integer_ops_perf.py: the same windows (wall time
around REPS calls ending in a device synchronise), the median of 7 rounds, every arm taken in turn within each round.

Arms, per operation:
  int_full    one Python int for the batch, a full-width scalar (0xDEADBEEF: no digit is 0, every block takes part)
  int_small   one Python int for the batch, a small scalar (5): the reference's shortcut DAG
  rows        one clear operand per row, a torch tensor on the device (nothing is copied)
  encrypted   the counterpart with two encrypted operands: add, bitand, eq, lt, max

Per arm: ms per call, operations/s, PBS per operation, launches, effective PBS/s and its fraction of the isolated
KS+PBS rate on the rows of the arm's average layer.  Per operation the ratios rows / int_full (the
same PBS counts) and both against encrypted (whose first layer has twice the rows of a packed comparison, or as many
for a bitwise op), each with the spread of its windows (min and max of the per-round ratios): a ratio whose spread
holds 1 is "not measurably different".

usage: integer_scalar_perf.py [--out result.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import integer_ops_perf as base  # noqa: E402
from tfhe_mi355 import integer, shortint  # noqa: E402
from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P  # noqa: E402

BLOCKS = 16
OPS = ("add", "bitand", "eq", "lt", "max")
ARMS = ("int_full", "int_small", "rows", "encrypted")
FULL, SMALL = 0xDEADBEEF, 5      # 0xDEADBEEF: the top digit is 3, every block takes part


def calls_of(sks, K, rng, cks):
    M = 1 << 32
    a = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    b = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    clear = rng.integers(M // 2, M, K, dtype=np.uint64)          # the top digit is not 0: the full-width DAG
    rows = torch.from_numpy(clear.view(np.int64)).to(sks.ops.device)
    calls = {}
    for op in OPS:
        scalar = getattr(sks, f"scalar_{op}_parallelized")
        encrypted = getattr(sks, "add_parallelized" if op == "add" else f"{op}_parallelized")
        calls[op] = {
            "int_full": lambda f=scalar: f(a, FULL),
            "int_small": lambda f=scalar: f(a, SMALL),
            "rows": lambda f=scalar: f(a, rows),
            "encrypted": lambda f=encrypted: f(a, b),
        }
    return calls


def add_parallelized(sks):
    """add_parallelized as the other default forms: on a clone"""
    def f(lhs, rhs):
        res = lhs.clone()
        sks.add_assign_parallelized(res, rhs)
        return res
    return f


def measure(sks, cks, K, reps, rng, rounds):
    calls = calls_of(sks, K, rng, cks)
    res = {"K": K, "reps_per_window": reps, "rounds": rounds, "ops": {}}
    counts, samples = {}, {}
    for op in OPS:                   # warm-up: LUTs, layer tables, scratch; and the counters
        for arm, f in calls[op].items():
            sks.pbs_count = sks.launches = 0
            f()
            counts[op, arm] = (sks.pbs_count, sks.launches)
            samples[op, arm] = []
    for _ in range(rounds):
        for op in OPS:
            for arm, f in calls[op].items():
                samples[op, arm].append(base.timed(f, reps))
    rates = {}
    for op in OPS:
        arms = {}
        for arm in ARMS:
            pbs, launches = counts[op, arm]
            med = statistics.median(samples[op, arm])
            rows = max(pbs // max(launches, 1), 1)
            if rows not in rates:
                rates[rows] = base.isolated_rate(sks, rows, max(reps, 3))
            arms[arm] = {
                "ms_per_call": 1e3 * med, "min_ms": 1e3 * min(samples[op, arm]), "max_ms": 1e3 * max(samples[op, arm]),
                "operations_per_s": K / med, "pbs_per_operation": pbs / K, "launches": launches,
                "effective_pbs_per_s": pbs / med, "mean_rows_per_layer": rows, "isolated_ks_pbs_per_s": rates[rows],
                "fraction_of_isolated": pbs / med / rates[rows],
            }
        ratios = {}
        for name, (num, den) in {"rows_over_int_full": ("rows", "int_full"), "rows_over_encrypted": ("rows", "encrypted"),
                                 "int_full_over_encrypted": ("int_full", "encrypted"),
                                 "int_small_over_int_full": ("int_small", "int_full")}.items():
            per_round = [x / y for x, y in zip(samples[op, num], samples[op, den])]
            lo, hi = min(per_round), max(per_round)
            ratios[name] = {"ratio_of_medians": arms[num]["ms_per_call"] / arms[den]["ms_per_call"],
                            "min_over_rounds": lo, "max_over_rounds": hi,
                            "verdict": "not measurably different" if lo <= 1.0 <= hi else
                                       ("faster" if hi < 1.0 else "slower")}
        res["ops"][op] = {"arms": arms, "time_ratios": ratios}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integer_scalar_perf_2_2.json"))
    ap.add_argument("--quick", action="store_true", help="one short window per arm: a rehearsal, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU fall-back"
    rounds = 1 if args.quick else base.ROUNDS
    base.ROUNDS = rounds

    def say(text):
        print(text, file=sys.stderr, flush=True)

    say("generating the 2_2 keys ...")
    ck = shortint.ClientKey(P, 11)
    sks = integer.ServerKey(shortint.ServerKey(ck))
    sks.add_parallelized = add_parallelized(sks)
    say("keys on the device")
    cks = integer.ClientKey(ck, BLOCKS)
    rng = np.random.default_rng(7)
    # correctness of what is timed: every scalar operation on two rows, per row and with one int, decrypts
    M = 1 << 32
    v = np.array([5, FULL], dtype=np.uint64)
    c = np.array([FULL, FULL - 1], dtype=np.uint64)
    x = sks.to_device(cks.encrypt(v))
    rows = torch.from_numpy(c.view(np.int64)).to(sks.ops.device)
    plain = {"add": lambda a, b: (a + b) % M, "bitand": lambda a, b: a & b, "eq": lambda a, b: int(a == b),
             "lt": lambda a, b: int(a < b), "max": max}
    for op in OPS:
        dec = integer.ClientKey(ck, 1 if op in ("eq", "lt") else BLOCKS)
        f = getattr(sks, f"scalar_{op}_parallelized")
        assert [int(t) for t in dec.decrypt(sks.to_host(f(x, rows)))] == [plain[op](int(a), int(b)) for a, b in zip(v, c)], op
        for s in (FULL, SMALL):
            assert [int(t) for t in dec.decrypt(sks.to_host(f(x, s)))] == [plain[op](int(a), s) for a in v], (op, s)
    say("the scalar operations decrypt; measuring")
    runs = []
    for K, reps in ((256, 3), (1, 20)):
        runs.append(measure(sks, cks, K, 1 if args.quick else reps, rng, rounds))
        say(f"K = {K} done")
    result = {"family": "scalar", "device": torch.cuda.get_device_name(0), "parameters": P.name, "blocks": BLOCKS,
              "full_width_scalar": FULL, "small_scalar": SMALL, "runs": runs}
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
