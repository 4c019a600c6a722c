#!/usr/bin/env python3
"""Per-kernel times of the GGSW operations, from the engine's own timer
(tfhe_mi355_kernel_timing_*), at (N, k, base_log, level) = (2048, 1, 5, 3) on random spectra:

  * one vertical packing of 1024 items, npoly 8, nbits 14 (3 tree launches + 11 rotation steps);
  * the same ciphertext count through one pbs_classic_kernel<2048,1,2> launch, as a yardstick;
  * the external product per node against the batch size, every item with its own GGSW and every
    item pointed at ONE GGSW (the stream served from cache): what the per-item stream costs.

usage: ggsw_perf.py [--out result.json]
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
from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P  # noqa: E402

N, k, B, L = 2048, 1, 5, 3
GGSW_BYTES = L * (k + 1) ** 2 * (N // 2) * 16


def random_spectra(eng, ggsw_count):
    d_f = torch.empty(eng.ggsw_list_fourier_bytes(ggsw_count, L) // 8, dtype=torch.float64, device="cuda")
    for a in range(0, d_f.numel(), 1 << 26):
        d_f[a:a + (1 << 26)] = torch.randn(min(1 << 26, d_f.numel() - a), device="cuda") * 0.1
    return d_f


def vertical_packing(eng, d_f, count=1024, npoly=8, nbits=14):
    d_luts = torch.randint(-2**62, 2**62, (1, npoly, N), dtype=torch.int64, device="cuda")
    d_out = torch.zeros((count, k * N + 1), dtype=torch.int64, device="cuda")
    scratch = torch.empty(eng.vertical_packing_scratch_bytes(npoly, count), dtype=torch.uint8, device="cuda")
    for it in range(4):
        if it == 1:
            eng.kernel_timing(1)
        eng.vertical_packing_async(d_f, B, L, nbits, d_luts, 1, npoly, count, d_out, d_scratch=scratch)
        torch.cuda.synchronize()
    t = eng.kernel_times()
    eng.kernel_timing(0)
    out = {"count": count, "npoly": npoly, "nbits": nbits, "ggsw_bytes_per_cmux": GGSW_BYTES,
           "kernels": {n: {"avg_ms": v[0], "launches": v[1]} for n, v in t.items()}}
    out["ms_per_call"] = sum(v[0] * v[1] for v in t.values()) / 3
    return out


def external_product_sweep(eng, d_f, total):
    d_in = torch.randint(-2**62, 2**62, (total, 2 * N), dtype=torch.int64, device="cuda")
    d_io = torch.zeros((total, 2 * N), dtype=torch.int64, device="cuda")
    d_zero = torch.zeros(total, dtype=torch.int32, device="cuda")
    rows = []
    for count in (256, 1024, 4096, total):
        for shared in (False, True):
            for it in range(4):
                if it == 1:
                    eng.kernel_timing(1)
                eng.ggsw_external_product_async(d_f, total, B, L, d_in, d_io, count, d_zero if shared else None)
                torch.cuda.synchronize()
            ms = eng.kernel_times()["ggsw_external_product"][0]
            eng.kernel_timing(0)
            rows.append({"count": count, "one_shared_ggsw": shared, "ms": ms, "us_per_node": 1e3 * ms / count,
                         "ggsw_GBps": None if shared else count * GGSW_BYTES / (ms * 1e-3) / 1e9})
    return rows


def pbs_yardstick(count=1024):
    p2 = P.with_(pbs_level=2, pbs_base_log=15, name="yardstick_2048_1_2")
    eng = Engine(p2, 0)
    rng = np.random.default_rng(1)
    eng.upload_bootstrap_key(rng.integers(0, 1 << 64, p2.lwe_dimension * 2 * 4 * N, dtype=np.uint64))
    d_in = torch.from_numpy(rng.integers(0, 1 << 64, (count, p2.lwe_dimension + 1), dtype=np.uint64).view(np.int64)).cuda()
    d_lut = torch.from_numpy(rng.integers(0, 1 << 64, 2 * N, dtype=np.uint64).view(np.int64)).cuda()
    d_o = torch.zeros((count, N + 1), dtype=torch.int64, device="cuda")
    for it in range(3):
        if it == 1:
            eng.kernel_timing(1)
        eng.programmable_bootstrap_async(d_in, d_o, d_lut, 1, count)
        torch.cuda.synchronize()
    ms = eng.kernel_times()["pbs_classic_kernel"][0]
    return {"kernel": "pbs_classic_kernel<2048,1,2>", "count": count, "n": p2.lwe_dimension, "ms": ms,
            "us_per_cmux": 1e3 * ms / (count * p2.lwe_dimension)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    eng = Engine(P, 0)
    total = 1024 * 14
    d_f = random_spectra(eng, total)
    res = {"shape": {"N": N, "k": k, "base_log": B, "level": L},
           "vertical_packing": vertical_packing(eng, d_f),
           "external_product": external_product_sweep(eng, d_f, total)}
    del d_f
    torch.cuda.empty_cache()
    res["pbs_yardstick"] = pbs_yardstick()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
