#!/usr/bin/env python3
"""Cost of the 128-bit-torus PBS on one GPU at the reference's f128 test set
(TEST_PARAMS_4_BITS_NATIVE_U128: n = 742, N = 2048, k = 1, base_log 23, level 1), in batches of 1, 64, 1024
and 4096, best of 3 rounds of 10 calls, wall time between stream synchronisations:

  * f128: tfhe_mi355_programmable_bootstrap_u128_async with a real key; every batch's outputs are decrypted
    and checked once before it is timed;
  * the yardstick, in the same process and alternating with it: the u64 PBS at the identical shape
    (PARAM_MESSAGE_2_CARRY_2's n, N, k, base, level; tfhe_mi355_programmable_bootstrap_async, random key:
    its time does not depend on the key's validity);
  * the share of the f128 wall time spent in pbs_f128_kernel, from the engine's kernel timer;
  * the CPU restatement tests/pbs_ref128.c (the project's own C restatement of DESIGN.md 3b, NOT the
    reference's Rust) on one ciphertext with one thread, and on 16 ciphertexts with 16 threads (it
    parallelises over ciphertexts), as seconds per ciphertext.

usage: f128_perf.py [--batches 1,64,1024,4096] [--rounds 3] [--reps 10] [--n 742] [--no-cpu] [--out result.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pbs128_reference as R  # noqa: E402
from tfhe_mi355 import Engine  # noqa: E402
from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P64  # noqa: E402
from tfhe_mi355.parameters import TEST_PARAMS_4_BITS_NATIVE_U128 as P128  # noqa: E402

BITS = 4


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=P128.lwe_dimension)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    p128, p64 = P128.with_(lwe_dimension=args.n), P64.with_(lwe_dimension=args.n)
    n, N, k = p128.lwe_dimension, p128.polynomial_size, p128.glwe_dimension
    assert (p64.polynomial_size, p64.glwe_dimension, p64.pbs_base_log, p64.pbs_level) == \
        (N, k, p128.pbs_base_log, p128.pbs_level), "the yardstick runs the identical shape"
    rng = np.random.default_rng(7)

    lwe_sk, glwe_sk = R.binary_key(1, n), R.binary_key(2, k * N)
    bsk = R.gen_bsk(3, lwe_sk, glwe_sk, k, N, p128.pbs_base_log, p128.pbs_level, p128.glwe_modular_std_dev, threads=16)
    e128, e64 = Engine.for_u128(p128, 0), Engine(p64, 0)
    e128.upload_bootstrap_key_u128(bsk)
    e64.upload_bootstrap_key(rng.integers(0, 1 << 64, n * p64.pbs_level * (k + 1) ** 2 * N, dtype=np.uint64))
    acc = R.identity_accumulator(N, k, BITS, lambda m: (3 * m + 5) % 16)
    d_acc = torch.from_numpy(acc.view(np.int64)).cuda()
    d_lut64 = torch.from_numpy(rng.integers(0, 1 << 64, (1, (k + 1) * N), dtype=np.uint64).view(np.int64)).cuda()
    delta = 1 << (128 - BITS - 1)

    rows = []
    for count in batches:
        msgs = [i % 16 for i in range(count)]
        cts = R.lwe_encrypt(100 + count, lwe_sk, R.to_words([m * delta for m in msgs]), p128.lwe_modular_std_dev)
        d_in = torch.from_numpy(cts.view(np.int64)).cuda()
        d_out = torch.zeros((count, k * N + 1, 2), dtype=torch.int64, device="cuda")
        s128 = torch.empty(max(e128.pbs_u128_scratch_bytes(count), 1), dtype=torch.uint8, device="cuda")
        x64 = torch.from_numpy(rng.integers(0, 1 << 64, (count, n + 1), dtype=np.uint64).view(np.int64)).cuda()
        out64 = torch.zeros((count, k * N + 1), dtype=torch.int64, device="cuda")
        s64 = torch.empty(max(e64.pbs_scratch_bytes(count), 1), dtype=torch.uint8, device="cuda")
        f128 = lambda: e128.programmable_bootstrap_u128_async(d_in, d_out, d_acc, 1, count,  # noqa: E731
                                                              d_scratch=s128)
        u64 = lambda: e64.programmable_bootstrap_async(x64, out64, d_lut64, 1, count, d_scratch=s64)  # noqa: E731
        f128()
        torch.cuda.synchronize()
        dec = R.decode(R.lwe_decrypt(glwe_sk, d_out.cpu().numpy().view(np.uint64)), BITS)
        assert dec == [(3 * m + 5) % 16 for m in msgs], f"batch {count}: outputs do not decrypt"
        t128, t64 = [], []
        for _ in range(args.rounds):  # alternating
            t128.append(timed(f128, args.reps))
            t64.append(timed(u64, args.reps))
        e128.kernel_timing(1)
        for _ in range(args.reps):
            f128()
        torch.cuda.synchronize()
        kt = e128.kernel_times()
        e128.kernel_timing(0)
        kern_ms = kt.get("pbs_f128_kernel", (0.0, 0))[0]
        rows.append({"batch": count, "decrypts": True,
                     "f128_ms": min(t128), "f128_pbs_per_s": count / (min(t128) * 1e-3), "f128_ms_rounds": t128,
                     "u64_ms": min(t64), "u64_pbs_per_s": count / (min(t64) * 1e-3), "u64_ms_rounds": t64,
                     "f128_over_u64": min(t128) / min(t64),
                     "pbs_f128_kernel_ms": kern_ms, "pbs_f128_kernel_share": kern_ms / min(t128)})
        print(json.dumps(rows[-1]), flush=True)
        del d_in, d_out, s128, x64, out64, s64
    resident = e128.pbs_u128_resident()
    e128.close()
    e64.close()

    cpu = None
    if not args.no_cpu:  # the project's C restatement, not the reference's Rust
        ref = R.RefEngine128(p128, threads=1)
        ref.upload_bootstrap_key_u128(bsk)
        one = R.lwe_encrypt(5, lwe_sk, R.to_words([3 * delta]), p128.lwe_modular_std_dev)
        t0 = time.perf_counter()
        out = ref.programmable_bootstrap_u128(one, acc)
        t1 = time.perf_counter() - t0
        assert R.decode(R.lwe_decrypt(glwe_sk, out), BITS) == [14]
        ref.threads = 16
        many = np.concatenate([one] * 16)
        t0 = time.perf_counter()
        ref.programmable_bootstrap_u128(many, acc)
        t16 = (time.perf_counter() - t0) / 16
        cpu = {"implementation": "tests/pbs_ref128.c (the project's restatement of DESIGN.md 3b, not the Rust)",
               "one_ciphertext_one_thread_s": t1, "sixteen_ciphertexts_sixteen_threads_s_per_ciphertext": t16}

    res = {"parameters": p128.name, "n": n, "N": N, "k": k, "pbs": [p128.pbs_base_log, p128.pbs_level],
           "yardstick": f"u64 PBS at {p64.name}'s n, N, k, base, level (same process, alternating)",
           "rounds": args.rounds, "reps": args.reps, "resident_workgroups": resident,
           "device": torch.cuda.get_device_name(0), "rows": rows, "cpu_restatement": cpu}
    text = json.dumps(res, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "f128_perf_2048_1.json")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
