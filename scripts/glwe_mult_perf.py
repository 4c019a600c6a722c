#!/usr/bin/env python3
"""Per-kernel times of the even transistor's product from the engine's own timer
(tfhe_mi355_kernel_timing_*), with random keys (times do not depend on the keys' validity), at
(k = 1, N = 2048) = PARAM_MESSAGE_2_CARRY_2_KS_PBS and (k = 3, N = 512) = GADGET_AES_PARAMETERS_23 with
pbs 7 x 4, both with the 6 x 4 keyswitch decomposition for the packing and relinearisation keys, at 64,
1024 and 4096 pairs:

  * lwe_mult: the packing keyswitch over 2 x count rows, the tensor kernel, the relinearisation kernel;
  * the yardstick from the same process: the KS + PBS launch over count rows at the same set.

woppbs_lut costs two KS + PBS, one packing launch and one product per input: the product's share of
that chain is reported next to the times.

usage: glwe_mult_perf.py [--set 2048_1 | 512_3] [--out result.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
from tfhe_mi355 import Engine  # noqa: E402
from tfhe_mi355 import parameters as PS  # noqa: E402

SETS = {
    "2048_1": PS.PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(ks_base_log=6, ks_level=4, name="2_2 with ks 6 x 4"),
    "512_3": PS.GADGET_AES_PARAMETERS_23.with_(pbs_base_log=7, pbs_level=4, ks_base_log=6, ks_level=4,
                                               name="AES_23 with pbs 7 x 4, ks 6 x 4"),
}
COUNTS = (64, 1024, 4096)


def rand_dev(shape, rng):
    return torch.from_numpy(rng.integers(0, 1 << 64, shape, dtype=np.uint64).view(np.int64)).cuda()


def timed(eng, call, reps=5):
    """{kernel: ms per call} over `reps` timed calls after one warm-up."""
    for it in range(reps + 1):
        if it == 1:
            eng.kernel_timing(1)
        call()
        torch.cuda.synchronize()
    t = eng.kernel_times()
    eng.kernel_timing(0)
    return {name: v[0] * v[1] / reps for name, v in t.items()}


def measure(P, rng):
    k, N, n, L = P.glwe_dimension, P.polynomial_size, P.lwe_dimension, P.ks_level
    glwe = (k + 1) * N
    eng = Engine(P, 0)
    eng.upload_bootstrap_key(rng.integers(0, 1 << 64, n * P.pbs_level * (k + 1) ** 2 * N, dtype=np.uint64))
    eng.upload_keyswitch_key(rng.integers(0, 1 << 64, k * N * L * (n + 1), dtype=np.uint64))
    eng.upload_packing_keyswitch_key(rng.integers(0, 1 << 64, k * N * L * glwe, dtype=np.uint64), P.ks_base_log, L)
    eng.upload_relinearization_key(rng.integers(0, 1 << 64, k * (k + 1) // 2 * L * glwe, dtype=np.uint64),
                                   P.ks_base_log, L)
    d_lut = rand_dev((1, glwe), rng)
    rows = []
    for count in COUNTS:
        d_l, d_r = rand_dev((count, k * N + 1), rng), rand_dev((count, k * N + 1), rng)
        d_out = torch.zeros((count, k * N + 1), dtype=torch.int64, device="cuda")
        scratch = torch.empty(eng.lwe_mult_scratch_bytes(count), dtype=torch.uint8, device="cuda")
        mult = timed(eng, lambda: eng.lwe_mult_async(d_l, d_r, 4, d_out, count, d_scratch=scratch))
        assert set(mult) == {"packing_keyswitch", "glwe_tensor", "glwe_relin"}, mult
        scratch = torch.empty(eng.ks_pbs_scratch_bytes(count), dtype=torch.uint8, device="cuda")
        boot = timed(eng, lambda: eng.keyswitch_programmable_bootstrap_async(d_l, d_out, d_lut, 1, count,
                                                                             d_scratch=scratch))
        ks_pbs = sum(boot.values())
        product = mult["glwe_tensor"] + mult["glwe_relin"]
        chain = 2 * ks_pbs + mult["packing_keyswitch"] + product
        rows.append({
            "pairs": count,
            "tensor_ms": mult["glwe_tensor"], "relin_ms": mult["glwe_relin"],
            "tensor_us_per_pair": 1e3 * mult["glwe_tensor"] / count,
            "relin_us_per_pair": 1e3 * mult["glwe_relin"] / count,
            "packing_keyswitch_ms": mult["packing_keyswitch"], "packing_rows": 2 * count,
            "ks_pbs_ms": ks_pbs, "ks_pbs_kernels": boot,
            "woppbs_lut_chain_ms": chain, "product_share_of_chain": product / chain,
            # u64 multiply-adds per pair: (k+1)^2 N^2 in the tensor kernel, k(k+1)/2 L (k+1) N^2 in the
            # relinearisation (the extracted body's products are single coefficients and not counted)
            "tensor_GMACs_per_s": count * ((k + 1) ** 2 - 1) * N * N / (mult["glwe_tensor"] * 1e-3) / 1e9,
            "relin_GMACs_per_s": count * (k * (k + 1) // 2) * L * k * N * N / (mult["glwe_relin"] * 1e-3) / 1e9,
        })
        del d_l, d_r, d_out, scratch
    eng.close()
    return {"parameters": P.name, "k": k, "N": N, "n": n, "pbs": [P.pbs_base_log, P.pbs_level],
            "ks_packing_relin": [P.ks_base_log, L], "log_p": 4, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default="2048_1")
    ap.add_argument("--out")
    args = ap.parse_args()
    res = measure(SETS[args.set], np.random.default_rng(7))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
