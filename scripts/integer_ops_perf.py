#!/usr/bin/env python3
"""What the radix integer operations of DESIGN.md 5.6b cost on the GPU: sub, lt, eq, bitand, max and if_then_else on
FheUint32 operands (16 blocks of PARAM_MESSAGE_2_CARRY_2_KS_PBS, the real key) at K = 256 and K = 1 operand pairs
per call, in one process.

Per operation and K: operations/s (K operations per call; wall time around REPS calls ending in a device
synchronise, the median of ROUNDS such windows, the operations taken in turn within each round), PBS per operation and
launches per call (the key's own counters), and the effective PBS/s as a fraction of the isolated KS+PBS rate --
the same engine call on the same number of rows as the operation's average layer, measured in the same process (the
metric DESIGN.md 5.6 quotes for the multiply).

The kernel's own share: `lt` once more with _DeviceOps.block_layer replaced by per-block
tfhe_mi355_lwe_scalar_mul_add_async calls (a copy of the first term, a scale, then one call per further term, a
plaintext add on the body through torch), alternating with the fused arm in every round; both arms' outputs are
compared first.  This unfused arm lives in this script only.

--family shift measures the operations of DESIGN.md 5.6c instead, by the same method and without the unfused arm:
scalar_left_shift and scalar_rotate_right by 5, left_shift and rotate_left by an encrypted amount, scalar_mul by 5
and by 0xDEADBEEF (profiles/integer_shift_perf_2_2.json).

--family div measures the operations of DESIGN.md 5.6d, again by the same method: div_rem and
unsigned_overflowing_sub (profiles/integer_div_perf_2_2.json).  A division is a couple of hundred dependent layers, so
its windows are a sixth as many calls; at K = 1 its time per call is put next to launches x the single-layer time of
a one-launch operation measured in the same process (scalar_left_shift by 5, the 2.6 ms of the shift family).

usage: integer_ops_perf.py [--family ops|shift|div] [--out result.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
from tfhe_mi355 import integer, shortint  # noqa: E402
from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P  # noqa: E402

BLOCKS = 16
OPS = ("sub", "lt", "eq", "bitand", "max", "if_then_else")
SHIFT_OPS = ("scalar_left_shift_5", "scalar_rotate_right_5", "left_shift", "rotate_left", "scalar_mul_5",
             "scalar_mul_0xDEADBEEF")
DIV_OPS = ("div_rem", "unsigned_overflowing_sub")
ROUNDS = 7


def timed(f, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def unfused_block_layer(ops_obj):
    """_DeviceOps.block_layer as the launches it replaces, block by block, the way the reference's shortint calls
    go: a group of terms (first * scalar + the others) is a copy of its first block followed by one
    lwe_scalar_mul_add call per further block (pack_block_chunk, the bivariate packing, the sums); the terms with
    negative scalars form a second group that is subtracted with one more call (compare_block_assign's LWE
    subtraction); a plaintext on the body is one torch add."""
    eng = ops_obj.eng

    def mul_add(y, x, scalar):
        eng.lwe_scalar_mul_add_async(y.data_ptr(), None if x is None else x.data_ptr(), scalar, y.shape[0], y.shape[1],
                                     y.stride(0), 0 if x is None else x.stride(0))
    return block_layer_from(mul_add)


def block_layer_from(mul_add):
    """the block layer out of mul_add(y, x, scalar): y = y * scalar + (x or 0) on [rows, words] views"""
    half = 1 << 63

    def build(buf, group):
        """buf = first * scalar + the others (every other scalar is 1 in the layers of integer.py)"""
        (first, scalar), rest = group[0], group[1:]
        assert all(s == 1 for _, s in rest)
        if first.data_ptr() != buf.data_ptr():
            buf.copy_(first)
        if not rest and scalar != 1:
            mul_add(buf, None, scalar)
        for i, (src, _) in enumerate(rest):
            mul_add(buf, src, scalar if i == 0 else 1)

    def block_layer(ops):
        for dst, body_add, terms in ops:
            terms = [(src, s % (1 << 64)) for src, s in terms]
            pos = [(src, s) for src, s in terms if s < half]
            neg = [(src, (1 << 64) - s) for src, s in terms if s >= half]
            if not terms:
                dst.zero_()
            elif not neg:
                build(dst, pos)
            else:
                build(dst, neg)
                if pos:
                    tmp = torch.empty_like(dst)
                    build(tmp, pos)
                    mul_add(dst, tmp, -1)          # dst = tmp - dst
                else:
                    mul_add(dst, None, -1)
            if body_add % (1 << 64):
                dst[:, -1] += int(np.uint64(body_add % (1 << 64)).view(np.int64))
    return block_layer


def calls_of(sks, K, rng, cks):
    M = 1 << 32
    a = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    b = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    cond = sks.lt_parallelized(a, b)
    calls = {
        "sub": lambda: sks.sub_parallelized(a, b),
        "lt": lambda: sks.lt_parallelized(a, b),
        "eq": lambda: sks.eq_parallelized(a, b),
        "bitand": lambda: sks.bitand_parallelized(a, b),
        "max": lambda: sks.max_parallelized(a, b),
        "if_then_else": lambda: sks.if_then_else_parallelized(cond, a, b),
    }
    return calls, (a, b)


def shift_calls_of(sks, K, rng, cks):
    M = 1 << 32
    a = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    amount = sks.to_device(cks.encrypt(rng.integers(0, 32, K, dtype=np.uint64)))
    calls = {
        "scalar_left_shift_5": lambda: sks.scalar_left_shift_parallelized(a, 5),
        "scalar_rotate_right_5": lambda: sks.scalar_rotate_right_parallelized(a, 5),
        "left_shift": lambda: sks.left_shift_parallelized(a, amount),
        "rotate_left": lambda: sks.rotate_left_parallelized(a, amount),
        "scalar_mul_5": lambda: sks.scalar_mul_parallelized(a, 5),
        "scalar_mul_0xDEADBEEF": lambda: sks.scalar_mul_parallelized(a, 0xDEADBEEF),
    }
    assert tuple(calls) == SHIFT_OPS
    return calls, (a, amount)


def div_calls_of(sks, K, rng, cks):
    M = 1 << 32
    a = sks.to_device(cks.encrypt(rng.integers(0, M, K, dtype=np.uint64)))
    b = sks.to_device(cks.encrypt(rng.integers(1, 1 << 16, K, dtype=np.uint64)))
    calls = {
        "div_rem": lambda: sks.div_rem_parallelized(a, b),
        "unsigned_overflowing_sub": lambda: sks.unsigned_overflowing_sub_parallelized(a, b),
    }
    assert tuple(calls) == DIV_OPS
    return calls, (a, b)


def isolated_rate(sks, rows, reps):
    """KS+PBS/s of one engine call on `rows` rows (one LUT), the same entry point the layers use"""
    eng, ops = sks.ops.eng, sks.ops
    x = torch.zeros((rows, sks.lwe_size), dtype=torch.int64, device=ops.device)
    out = torch.empty_like(x)
    lut = ops.from_host(sks.lut_message.acc[None])
    scratch = torch.empty(max(eng.ks_pbs_scratch_bytes(rows), 1), dtype=torch.uint8, device=ops.device)
    f = lambda: eng.keyswitch_programmable_bootstrap_async(x, out, lut, 1, rows, scratch)   # noqa: E731
    f()
    return rows / statistics.median(timed(f, reps) for _ in range(ROUNDS))


def measure(sks, cks, K, reps, rng, family="ops"):
    calls, (a, b) = {"ops": calls_of, "shift": shift_calls_of, "div": div_calls_of}[family](sks, K, rng, cks)
    window = {name: max(1, reps // 6) if name == "div_rem" else reps for name in calls}
    res = {"K": K, "reps_per_window": reps, "rounds": ROUNDS, "ops": {}}
    counts = {}
    for name, f in calls.items():   # warm-up: LUTs, layer tables, scratch; and the counters
        sks.pbs_count = sks.launches = 0
        f()
        counts[name] = (sks.pbs_count, sks.launches)
    fused = sks.ops.block_layer
    unfused = unfused_block_layer(sks.ops)
    if "lt" in calls:
        want = sks.to_host(calls["lt"]())
        sks.ops.block_layer = unfused
        same = bool(np.array_equal(sks.to_host(calls["lt"]()).data, want.data))
        sks.ops.block_layer = fused
    samples = {name: [] for name in list(calls) + ["lt_unfused"]}
    for _ in range(ROUNDS):
        for name, f in calls.items():
            samples[name].append(timed(f, window[name]))
            if name == "lt":
                sks.ops.block_layer = unfused
                samples["lt_unfused"].append(timed(f, reps))
                sks.ops.block_layer = fused
    rates = {}
    for name in calls:
        pbs, launches = counts[name]
        med = statistics.median(samples[name])
        rows = max(pbs // max(launches, 1), 1)
        if rows not in rates:
            rates[rows] = isolated_rate(sks, rows, max(reps, 3))
        res["ops"][name] = {
            "ms_per_call": 1e3 * med, "min_ms": 1e3 * min(samples[name]), "max_ms": 1e3 * max(samples[name]),
            "operations_per_s": K / med, "pbs_per_operation": pbs / K, "launches": launches,
            "effective_pbs_per_s": pbs / med, "mean_rows_per_layer": rows, "isolated_ks_pbs_per_s": rates[rows],
            "fraction_of_isolated": pbs / med / rates[rows], "calls_per_window": window[name],
        }
    if family == "div" and K == 1:
        shift = lambda: sks.scalar_left_shift_parallelized(a, 5)   # noqa: E731  (one fused layer of 14 rows)
        shift()
        layer = statistics.median(timed(shift, reps) for _ in range(ROUNDS))
        res["single_layer_ms"] = 1e3 * layer
        for name in calls:
            op = res["ops"][name]
            op["launches_x_single_layer_ms"] = op["launches"] * 1e3 * layer
            op["ratio_to_launches_x_single_layer"] = op["ms_per_call"] / op["launches_x_single_layer_ms"]
    if "lt" not in calls:
        return res
    u = statistics.median(samples["lt_unfused"])
    f_ = statistics.median(samples["lt"])
    res["lt_unfused"] = {"outputs_equal_fused": same, "ms_per_call": 1e3 * u, "min_ms": 1e3 * min(samples["lt_unfused"]),
                         "max_ms": 1e3 * max(samples["lt_unfused"]), "fused_ms_per_call": 1e3 * f_,
                         "fused_speedup": u / f_}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=("ops", "shift", "div"), default="ops")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one short window per arm: a rehearsal, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU fall-back"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"integer_{args.family}_perf_2_2.json")
    if args.quick:
        ROUNDS = 1
    def say(text):
        print(text, file=sys.stderr, flush=True)

    say("generating the 2_2 keys ...")
    ck = shortint.ClientKey(P, 11)
    sks = integer.ServerKey(shortint.ServerKey(ck))
    say("keys on the device")
    cks = integer.ClientKey(ck, BLOCKS)
    rng = np.random.default_rng(7)
    # correctness of what is timed: one lt and one sub on two rows decrypt
    v = np.array([[5, 1 << 31], [7, 3]], dtype=np.uint64)
    x, y = sks.to_device(cks.encrypt(v[0])), sks.to_device(cks.encrypt(v[1]))
    assert [int(t) for t in integer.ClientKey(ck, 1).decrypt(sks.to_host(sks.lt_parallelized(x, y)))] == [1, 0]
    assert [int(t) for t in cks.decrypt(sks.to_host(sks.sub_parallelized(x, y)))] == [(5 - 7) % (1 << 32), (1 << 31) - 3]
    if args.family == "shift":   # and of the new family: a shift by an encrypted amount and a scalar_mul decrypt
        amount = sks.to_device(cks.encrypt(np.array([3, 31], dtype=np.uint64)))
        assert [int(t) for t in cks.decrypt(sks.to_host(sks.left_shift_parallelized(x, amount)))] == [5 << 3, 0]
        assert [int(t) for t in cks.decrypt(sks.to_host(sks.scalar_rotate_right_parallelized(x, 5)))] == \
            [(5 >> 5) | ((5 << 27) & 0xFFFFFFFF), 1 << 26]
        assert [int(t) for t in cks.decrypt(sks.to_host(sks.scalar_mul_parallelized(x, 0xDEADBEEF)))] == \
            [(5 * 0xDEADBEEF) % (1 << 32), ((1 << 31) * 0xDEADBEEF) % (1 << 32)]
    if args.family == "div":
        q, r = sks.div_rem_parallelized(x, y)
        assert [int(t) for t in cks.decrypt(sks.to_host(q))] == [5 // 7, (1 << 31) // 3]
        assert [int(t) for t in cks.decrypt(sks.to_host(r))] == [5 % 7, (1 << 31) % 3]
        d, o = sks.unsigned_overflowing_sub_parallelized(x, y)
        assert [int(t) for t in cks.decrypt(sks.to_host(d))] == [(5 - 7) % (1 << 32), (1 << 31) - 3]
        assert [int(t) for t in integer.ClientKey(ck, 1).decrypt(sks.to_host(o))] == [1, 0]
    say("lt and sub decrypt; measuring")
    runs = []
    for K, reps in ((256, 3), (1, 20)):
        runs.append(measure(sks, cks, K, 1 if args.quick else reps, rng, args.family))
        say(f"K = {K} done")
    result = {"family": args.family, "device": torch.cuda.get_device_name(0), "parameters": P.name, "blocks": BLOCKS,
              "runs": runs}
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
