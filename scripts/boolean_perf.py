#!/usr/bin/env python3
"""Gate throughput of the native 32-bit-torus path with random keys (times do not depend
on the keys' validity), from wall time between stream synchronisations and from the engine's own kernel
timer (tfhe_mi355_kernel_timing_*), at 64, 1024 and 4096 gates of one batch:

  * native: tfhe_mi355_boolean_gates_async (prologue, u32 PBS, u32 keyswitch);
  * the yardstick, in the same process and alternating with it: the same number of rows through the u64
    PBS and keyswitch kernels at the same shape (a second context with u64 keys;
    tfhe_mi355_programmable_bootstrap_keyswitch_async) -- what pushing the gates through the existing
    kernels with every word shifted left by 32 would cost (it computes different bits: DESIGN.md 5.15).
    It is measured twice per round so that its own spread is on record.

usage: boolean_perf.py [--set DEFAULT_PARAMETERS | TFHE_LIB_PARAMETERS] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
from tfhe_mi355 import Engine  # noqa: E402
from tfhe_mi355 import boolean as B  # noqa: E402

SETS = {"DEFAULT_PARAMETERS": B.DEFAULT_PARAMETERS, "TFHE_LIB_PARAMETERS": B.TFHE_LIB_PARAMETERS}
COUNTS = (64, 1024, 4096)
ROUNDS, REPS = 3, 10


def run(eng, call, reps=REPS):
    """(wall ms per call with the timer off, {kernel family: ms per call} from a second, timed pass) over
    `reps` calls each, after one warm-up."""
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / reps
    eng.kernel_timing(1)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    t = eng.kernel_times()
    eng.kernel_timing(0)
    return wall, {name: v[0] * v[1] / reps for name, v in t.items()}


def measure(P, rng):
    assert P.pbs_order == 1, "BootstrapKeyswitch sets"
    k, N, n = P.glwe_dimension, P.polynomial_size, P.lwe_dimension
    bsk_words, ksk_words = n * P.pbs_level * (k + 1) ** 2 * N, k * N * P.ks_level * (n + 1)
    e32, e64 = Engine(P, 0), Engine(P, 0)
    e32.upload_bootstrap_key_u32(rng.integers(0, 1 << 32, bsk_words, dtype=np.uint32))
    e32.upload_keyswitch_key_u32(rng.integers(0, 1 << 32, ksk_words, dtype=np.uint32))
    e64.upload_bootstrap_key(rng.integers(0, 1 << 64, bsk_words, dtype=np.uint64))
    e64.upload_keyswitch_key(rng.integers(0, 1 << 64, ksk_words, dtype=np.uint64))
    lut64 = torch.from_numpy(rng.integers(0, 1 << 64, (1, (k + 1) * N), dtype=np.uint64).view(np.int64)).cuda()
    rows = []
    for count in COUNTS:
        a, b = (torch.from_numpy(rng.integers(0, 1 << 32, (count, n + 1), dtype=np.uint32).view(np.int32)).cuda()
                for _ in range(2))
        ops = torch.from_numpy((np.arange(count) % 6).astype(np.uint8)).cuda()
        out32 = torch.zeros((count, n + 1), dtype=torch.int32, device="cuda")
        x64 = torch.from_numpy(rng.integers(0, 1 << 64, (count, n + 1), dtype=np.uint64).view(np.int64)).cuda()
        out64 = torch.zeros((count, n + 1), dtype=torch.int64, device="cuda")
        s32 = torch.empty(max(e32.boolean_gates_scratch_bytes(count, 1), 1), dtype=torch.uint8, device="cuda")
        s64 = torch.empty(max(e64.pbs_ks_scratch_bytes(count), 1), dtype=torch.uint8, device="cuda")
        native = lambda: e32.boolean_gates_async(ops, a, b, out32, count, 1, d_scratch=s32)  # noqa: E731
        yard = lambda: e64.programmable_bootstrap_keyswitch_async(x64, out64, lut64, 1, count,  # noqa: E731
                                                                  d_scratch=s64)
        nat, y1, y2 = [], [], []
        for _ in range(ROUNDS):  # alternating: native, yardstick, yardstick
            nat.append(run(e32, native))
            y1.append(run(e64, yard))
            y2.append(run(e64, yard))
        best = lambda runs: min(runs, key=lambda r: r[0])  # noqa: E731
        n_wall, n_k = best(nat)
        rows.append({
            "gates": count,
            "native_ms": n_wall, "native_gates_per_s": count / (n_wall * 1e-3), "native_kernels_ms": n_k,
            "native_ms_rounds": [r[0] for r in nat],
            "yardstick_ms": [best(y1)[0], best(y2)[0]],
            "yardstick_rows_per_s": [count / (best(y)[0] * 1e-3) for y in (y1, y2)],
            "yardstick_kernels_ms": [best(y1)[1], best(y2)[1]],
            "yardstick_ms_rounds": [[r[0] for r in y1], [r[0] for r in y2]],
            "native_over_yardstick": n_wall / min(best(y1)[0], best(y2)[0]),
        })
        del a, b, ops, out32, x64, out64, s32, s64
    e32.close()
    e64.close()
    return {"parameters": P.name, "k": k, "N": N, "n": n, "pbs": [P.pbs_base_log, P.pbs_level],
            "ks": [P.ks_base_log, P.ks_level], "pbs_order": 1, "reps": REPS, "rounds": ROUNDS, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default="DEFAULT_PARAMETERS")
    ap.add_argument("--out")
    args = ap.parse_args()
    res = measure(SETS[args.set], np.random.default_rng(7))
    out = args.out or os.path.join(ROOT, "profiles", f"boolean_perf_{args.set}.json")
    text = json.dumps(res, indent=1)
    print(text)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
