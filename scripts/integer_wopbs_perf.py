#!/usr/bin/env python3
"""The composed call of an integer WoP-PBS by kernel family, from the engine's own timer
(tfhe_mi355_kernel_timing_*): WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS with n = 769 and random keys (times
do not depend on the key's validity), 4-block integers without padding -- 16 index bits, a LUT of 32
polynomials per output, 4 outputs -- at K = 1 and K = 64 integers.

Arms, five repeats each (every repeat: one call under the timer for the families' times and launch
counts, one call without it between two events for the wall time):
  * default    one launch per CMUX tree level over (item, output, node), one rotation chain launch;
  * stepwise   TFHE_MI355_VP_STEPWISE=1: the same multi-output addressing, one launch per rotation step;
  * parent     (--parent-lib PATH) another build of the library, e.g. the parent commit's, in a child
               process: there the vertical packing ran once per output between strided copies.

The vertical-packing part of a call is the sum of its ggsw_* families; `vp_by_wall_ms` is the call's wall
time minus every other family, which also holds what no family times (the parent's strided copies, gaps
between launches).  Medians and the spread between repeats are written next to the repeats.

usage: integer_wopbs_perf.py [--out result.json] [--parent-lib libtfhe_mi355.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-rs-odd_amd"))

NBITS, NPOLY, NOUT, REPEATS = 16, 32, 4, 5
COUNTS = (1, 64)


def load_engine():
    """the package, with the signature table cut to the symbols the loaded library has (an older build
    lacks the newer entry points; this script calls none of them)."""
    import torch  # noqa: F401  (one HIP runtime for torch and the engine)
    from tfhe_mi355 import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES[:] = [s for s in _lib.SIGNATURES if hasattr(lib, s[0])]
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    return Engine, P


def measure(eng, P, count, rng):
    import torch

    N, k, n = P.polynomial_size, P.glwe_dimension, P.lwe_dimension

    def rand_dev(shape):
        return torch.from_numpy(rng.integers(0, 1 << 64, shape, dtype=np.uint64).view(np.int64)).cuda()

    d_bits = rand_dev((count, NBITS, n + 1))
    d_luts = rand_dev((1, NOUT, NPOLY, N))
    d_out = torch.zeros((count, NOUT, k * N + 1), dtype=torch.int64, device="cuda")
    need = eng.circuit_bootstrap_vertical_packing_scratch_bytes(NBITS, P.cbs_level, 1, NOUT, NPOLY, count)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call():
        eng.circuit_bootstrap_vertical_packing_async(d_bits, NBITS, P.cbs_base_log, P.cbs_level, d_luts, 1, NOUT, NPOLY,
                                                     count, d_out, d_scratch=scratch)

    call()
    torch.cuda.synchronize()
    repeats = []
    for _ in range(REPEATS):
        eng.kernel_timing(1)
        call()
        torch.cuda.synchronize()
        t = eng.kernel_times()
        eng.kernel_timing(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        fam = {name: {"ms": v[0] * v[1], "launches": v[1]} for name, v in t.items()}
        vp = sum(f["ms"] for name, f in fam.items() if name.startswith("ggsw_"))
        other = sum(f["ms"] for name, f in fam.items() if not name.startswith("ggsw_"))
        wall = e0.elapsed_time(e1)
        repeats.append({"families": fam, "wall_ms": wall, "vp_ms": vp, "vp_by_wall_ms": wall - other,
                        "vp_launches": sum(f["launches"] for name, f in fam.items() if name.startswith("ggsw_"))})
    out = {"count": count, "scratch_bytes": need, "repeats": repeats}
    for key in ("wall_ms", "vp_ms", "vp_by_wall_ms"):
        vals = [r[key] for r in repeats]
        out[key] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    out["vp_launches"] = repeats[0]["vp_launches"]
    return out


def run_arm(stepwise):
    Engine, P = load_engine()
    N, k, n = P.polynomial_size, P.glwe_dimension, P.lwe_dimension
    rng = np.random.default_rng(5)
    eng = Engine(P, 0)
    eng.upload_bootstrap_key(rng.integers(0, 1 << 64, n * P.pbs_level * (k + 1) ** 2 * N, dtype=np.uint64))
    eng.upload_keyswitch_key(rng.integers(0, 1 << 64, k * N * P.ks_level * (n + 1), dtype=np.uint64))
    eng.upload_pfpksk_list(rng.integers(0, 1 << 64, (k + 1) * (k * N + 1) * P.pfks_level * (k + 1) * N, dtype=np.uint64),
                           P.pfks_base_log, P.pfks_level)
    if stepwise:
        os.environ["TFHE_MI355_VP_STEPWISE"] = "1"
    else:
        os.environ.pop("TFHE_MI355_VP_STEPWISE", None)
    return [measure(eng, P, count, rng) for count in COUNTS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-lib", help="another build of libtfhe_mi355.so to run the same call on (child process)")
    ap.add_argument("--child", action="store_true", help="(child) one default arm on TFHE_MI355_LIB, JSON on stdout")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_arm(False)))
        return
    res = {"parameters": "WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS", "nbits": NBITS, "npoly": NPOLY, "nout": NOUT,
           "repeats": REPEATS, "arms": {"default": run_arm(False), "stepwise": run_arm(True)}}
    if args.parent_lib:
        env = dict(os.environ, TFHE_MI355_LIB=os.path.abspath(args.parent_lib))
        env.pop("TFHE_MI355_VP_STEPWISE", None)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True,
                               capture_output=True, text=True, timeout=600)
        res["arms"]["parent"] = json.loads(child.stdout.strip().splitlines()[-1])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
