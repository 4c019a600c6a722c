#!/usr/bin/env python3
"""What compressed ciphertext ingress costs and saves at the host boundary, with random keys (times
do not depend on the keys' validity), 4096 ciphertexts per call, KS -> PBS, at PARAM_MESSAGE_2_CARRY_2_KS_PBS and at
one accepted compact-public-key set, in one process.  Per arm: the median of REPS calls after a warm-up, the arms
taken in turn within each of the REPS rounds (so drift hits all alike).

  host-pointer calls, wall time around the (synchronous) call:
    rows_pageable / rows_pinned       tfhe_mi355_keyswitch_programmable_bootstrap from expanded rows
    from_compact / _seeded_list / _seeded_rows
                                      tfhe_mi355_apply_from from pageable sources (pageable and pinned output)
  device-resident calls, wall time around ASYNC_BATCH calls and one synchronise:
    async_rows                        tfhe_mi355_keyswitch_programmable_bootstrap_async
    async_from_*                      tfhe_mi355_apply_from_async
  the expansion kernels alone (tfhe_mi355_lwe_expand_async), EXPAND_BATCH calls per synchronise: GB/s written.

usage: lwe_ingress_perf.py [--out result.json]
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
from tfhe_mi355 import Engine, LweSource, pinned_empty  # noqa: E402
from tfhe_mi355 import parameters as P  # noqa: E402

COUNT, REPS, ASYNC_BATCH, EXPAND_BATCH = 4096, 12, 4, 50
SETS = ("PARAM_MESSAGE_2_CARRY_2_KS_PBS", "PARAM_MESSAGE_2_CARRY_2_COMPACT_PK_KS_PBS")
KINDS = ("compact", "seeded_list", "seeded_rows")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def timed(f, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def measure(name, rng):
    p = P.ALL.get(name) or P.COMPACT_PK_ALL[name]
    k, N, n = p.glwe_dimension, p.polynomial_size, p.lwe_dimension
    big = k * N
    eng = Engine(p, 0)
    eng.upload_bootstrap_key(rng.integers(0, 1 << 64, n * p.pbs_level * (k + 1) ** 2 * N, dtype=np.uint64))
    eng.upload_keyswitch_key(rng.integers(0, 1 << 64, big * p.ks_level * (n + 1), dtype=np.uint64))
    lut = rng.integers(0, 1 << 64, (1, (k + 1) * N), dtype=np.uint64)
    rows = rng.integers(0, 1 << 64, (COUNT, big + 1), dtype=np.uint64)
    rows_pin, out_pin = pinned_empty(rows.shape), pinned_empty((COUNT, big + 1))
    rows_pin[...] = rows
    out = np.empty((COUNT, big + 1), dtype=np.uint64)
    seeds = rng.integers(0, 1 << 64, (COUNT, 2), dtype=np.uint64)
    host = {
        "compact": LweSource("compact", big, rng.integers(0, 1 << 64, -(-COUNT // big) * big + COUNT, dtype=np.uint64),
                             count=COUNT),
        "seeded_list": LweSource("seeded_list", big, rng.integers(0, 1 << 64, COUNT, dtype=np.uint64), seeds=seeds[0]),
        "seeded_rows": LweSource("seeded_rows", big, rng.integers(0, 1 << 64, COUNT, dtype=np.uint64), seeds=seeds),
    }

    def from_host(kind, o):
        return lambda: eng.apply_from("ks_pbs", host[kind], lut, out=o)

    arms = {
        "rows_pageable": lambda: eng.keyswitch_programmable_bootstrap(rows, lut, out=out),
        "rows_pinned": lambda: eng.keyswitch_programmable_bootstrap(rows_pin, lut, out=out_pin),
    }
    for kind in KINDS:
        arms[f"from_{kind}"] = from_host(kind, out)
        arms[f"from_{kind}_pinned_out"] = from_host(kind, out_pin)
    # device-resident
    d_lut, d_rows = dev(lut), dev(rows)
    d_out = torch.zeros((COUNT, big + 1), dtype=torch.int64, device="cuda")
    d_src = {kind: LweSource(kind, big, dev(s.data), None if s.seeds is None else dev(s.seeds), count=COUNT)
             for kind, s in host.items()}
    s_rows = torch.empty(max(eng.ks_pbs_scratch_bytes(COUNT), 1), dtype=torch.uint8, device="cuda")
    s_from = {kind: torch.empty(eng.apply_from_scratch_bytes("ks_pbs", s.kind, COUNT), dtype=torch.uint8, device="cuda")
              for kind, s in d_src.items()}
    asyncs = {"async_rows": lambda: eng.keyswitch_programmable_bootstrap_async(d_rows, d_out, d_lut, 1, COUNT,
                                                                               d_scratch=s_rows)}
    for kind in KINDS:
        asyncs[f"async_from_{kind}"] = (lambda kind=kind: eng.apply_from_async("ks_pbs", d_src[kind], d_out, d_lut, 1,
                                                                                d_scratch=s_from[kind]))
    s_exp = torch.empty(max(eng.lwe_expand_scratch_bytes(2, big, COUNT), 1), dtype=torch.uint8, device="cuda")
    d_exp = torch.zeros((COUNT, big + 1), dtype=torch.int64, device="cuda")
    expands = {f"expand_{kind}": (lambda kind=kind: eng.lwe_expand_async(d_src[kind], d_exp, d_scratch=s_exp))
               for kind in KINDS}

    samples = {a: [] for a in list(arms) + list(asyncs) + list(expands)}
    for f in list(arms.values()) + list(asyncs.values()) + list(expands.values()):  # warm-up
        f()
    torch.cuda.synchronize()
    same = {kind: bool(np.array_equal(eng.apply_from("ks_pbs", host[kind], lut),
                                      eng.keyswitch_programmable_bootstrap(eng.lwe_expand(host[kind]), lut)))
            for kind in KINDS}
    for _ in range(REPS):
        for a, f in arms.items():
            samples[a].append(timed(f))
        for a, f in asyncs.items():
            samples[a].append(timed(f, ASYNC_BATCH))
        for a, f in expands.items():
            samples[a].append(timed(f, EXPAND_BATCH))
    eng.close()
    res = {"parameters": name, "n": n, "k": k, "N": N, "count": COUNT, "reps": REPS, "outputs_equal_expand_then_call": same,
           "row_bytes": (big + 1) * 8, "source_bytes_per_ciphertext": {
               "rows": (big + 1) * 8, "compact": 8 + 8 * big * (-(-COUNT // big)) / COUNT, "seeded_list": 8, "seeded_rows": 24},
           "arms": {}}
    for a, t in samples.items():
        med = statistics.median(t)
        row = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t)}
        if a.startswith("expand_"):
            row["gb_per_s_written"] = COUNT * (big + 1) * 8 / med / 1e9
        else:
            row["pbs_per_s"] = COUNT / med
        res["arms"][a] = row
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lwe_ingress_perf_2_2.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU fall-back"
    rng = np.random.default_rng(7)
    result = {"device": torch.cuda.get_device_name(0), "sets": [measure(name, rng) for name in SETS]}
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
