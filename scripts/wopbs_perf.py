#!/usr/bin/env python3
"""Per-kernel times of the bootstrapped half of WoP-PBS, from the engine's own timer
(tfhe_mi355_kernel_timing_*), at WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS with random keys (times do not
depend on the key's validity), 1024 items of 4 bits:

  * extract_bits (delta_log 60, 4 bits): the glue, keyswitch and PBS launches of its three rounds;
  * circuit bootstrap + vertical packing of the 4096 extracted bits: the PBS launch over 12,288 rows,
    the pfpks over the same rows, the Fourier conversion and the four rotation steps;
  * the pfpks alone against the batch size (64, 1024, 12,288 rows), in the int8-MFMA form and -- in a
    child process with TFHE_MI355_PFPKS_NO_MFMA=1 -- the 64-bit integer form, with the key bytes each
    streams per second (every 64-row tile reads the whole key once).

usage: wopbs_perf.py [--out result.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))
from tfhe_mi355 import Engine  # noqa: E402
from tfhe_mi355.parameters import WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS as P  # noqa: E402

N, k, n = P.polynomial_size, P.glwe_dimension, P.lwe_dimension
KEY_WORDS = (k + 1) * (k * N + 1) * P.pfks_level * (k + 1) * N


def rand_dev(shape, rng):
    return torch.from_numpy(rng.integers(0, 1 << 64, shape, dtype=np.uint64).view(np.int64)).cuda()


def engine(rng, with_pbs_keys):
    eng = Engine(P, 0)
    if with_pbs_keys:
        eng.upload_bootstrap_key(rng.integers(0, 1 << 64, n * P.pbs_level * (k + 1) ** 2 * N, dtype=np.uint64))
        eng.upload_keyswitch_key(rng.integers(0, 1 << 64, k * N * P.ks_level * (n + 1), dtype=np.uint64))
    eng.upload_pfpksk_list(rng.integers(0, 1 << 64, KEY_WORDS, dtype=np.uint64), P.pfks_base_log, P.pfks_level)
    return eng


def timed(eng, call, reps=3):
    """{kernel: {avg_ms, launches per call}} over `reps` timed calls after one warm-up."""
    for it in range(reps + 1):
        if it == 1:
            eng.kernel_timing(1)
        call()
        torch.cuda.synchronize()
    t = eng.kernel_times()
    eng.kernel_timing(0)
    return {name: {"avg_ms": v[0], "launches_per_call": v[1] / reps, "ms_per_call": v[0] * v[1] / reps}
            for name, v in t.items()}


def pfpks_sweep(eng, rng, generic):
    name = "pfpks_generic" if generic else "pfpks_mfma"
    stream_bytes = KEY_WORDS * 8  # the u64 key, or its 8 int8 planes: the same bytes up to padding
    rows = []
    for count in (64, 1024, 12288):
        d_in = rand_dev((count, k * N + 1), rng)
        d_out = torch.zeros((count, k + 1, (k + 1) * N), dtype=torch.int64, device="cuda")
        scratch = torch.empty(max(eng.pfpks_scratch_bytes(count), 256), dtype=torch.uint8, device="cuda")
        t = timed(eng, lambda: eng.private_functional_packing_keyswitch_async(d_in, d_out, count, d_scratch=scratch))
        assert set(t) == {name}, t
        ms = t[name]["avg_ms"]
        tiles = (count + 63) // 64
        rows.append({"form": name, "rows": count, "ms": ms, "us_per_row": 1e3 * ms / count,
                     "key_GBps": tiles * stream_bytes / (ms * 1e-3) / 1e9,
                     # every key word meets every row once: KEY_WORDS u64 x digit MACs per row, as 8 + 7
                     # int8 MACs each in the MFMA form
                     "u64_GMACs_per_s": count * KEY_WORDS / (ms * 1e-3) / 1e9,
                     "int8_TMACs_per_s": None if generic else 15 * count * KEY_WORDS / (ms * 1e-3) / 1e12})
        del d_in, d_out, scratch
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--generic-sweep", action="store_true", help="(child) the 64-bit pfpks sweep alone, JSON on stdout")
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    if args.generic_sweep:
        print(json.dumps(pfpks_sweep(engine(rng, False), rng, True)))
        return
    eng = engine(rng, True)
    count, nbits = 1024, 4
    res = {"parameters": P.name, "items": count, "bits": nbits, "pfpksk_bytes": KEY_WORDS * 8}
    d_big = rand_dev((count, k * N + 1), rng)
    d_bits = torch.zeros((count, nbits, n + 1), dtype=torch.int64, device="cuda")
    scratch = torch.empty(eng.extract_bits_scratch_bytes(count), dtype=torch.uint8, device="cuda")
    res["extract_bits"] = timed(eng, lambda: eng.extract_bits_async(d_big, 60, nbits, d_bits, count, d_scratch=scratch))
    del scratch
    d_luts = rand_dev((1, 1, 1, N), rng)
    d_out = torch.zeros((count, 1, k * N + 1), dtype=torch.int64, device="cuda")
    need = eng.circuit_bootstrap_vertical_packing_scratch_bytes(nbits, P.cbs_level, 1, 1, 1, count)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    res["circuit_bootstrap_vertical_packing"] = timed(eng, lambda: eng.circuit_bootstrap_vertical_packing_async(
        d_bits, nbits, P.cbs_base_log, P.cbs_level, d_luts, 1, 1, 1, count, d_out, d_scratch=scratch))
    res["circuit_bootstrap_vertical_packing"]["scratch_bytes"] = need
    res["circuit_bootstrap_vertical_packing"]["pbs_rows"] = count * nbits * P.cbs_level
    del scratch, d_out, d_bits, d_big
    torch.cuda.empty_cache()
    res["pfpks"] = pfpks_sweep(eng, rng, False)
    env = dict(os.environ, TFHE_MI355_PFPKS_NO_MFMA="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--generic-sweep"], env=env, check=True,
                           capture_output=True, text=True, timeout=300)
    res["pfpks"] += json.loads(child.stdout.strip().splitlines()[-1])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
