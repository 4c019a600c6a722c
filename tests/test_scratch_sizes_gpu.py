"""The *_scratch queries of include/tfhe_mi355.h, pinned to recorded values.

Every device-pointer (_async) entry point carves the caller's scratch by the layout its *_scratch query
sums up; tests/test_async_guards_gpu.py shows on the device that the two agree.  This file pins the sums
themselves: tests/golden/scratch_sizes.json holds the reference value of every query, per engine, at each
count (`python tests/test_scratch_sizes_gpu.py --write` records it from the library it loads).  A query the
reference library refuses is absent from the file; the test asserts that the same set of queries succeeds
and that every value is the same.  Queries allocate nothing, so the full-size parameter sets cost a context
each and no more.

  keyless contexts (2_2, mb3, 3_3 at N = 8192, 4_4 at N = 32768, mb3_3g3): the PBS, KS, KS -> PBS and
    PBS -> KS queries at counts 0, 1, 5, 300 and 1025 (past the multi-bit large_chunk of 1024, capi_pbs.cpp);
  the small keyed engines of test_async_guards_gpu.py (ks512, mult1024, ggsw, wop512, the two Boolean
    shapes, the two 128-bit ones): every query of the header at counts 0, 1, 5 and 300, both pbs_order
    values for gates and mux, two (nbits, cbs_level, nout, npoly) tuples for the vertical-packing queries.
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_sizes.json")

KEYLESS = {
    "2_2": "PARAM_MESSAGE_2_CARRY_2_KS_PBS",
    "mb3": "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS",
    "3_3": "PARAM_MESSAGE_3_CARRY_3_KS_PBS",
    "4_4": "PARAM_MESSAGE_4_CARRY_4_KS_PBS",
    "mb3_3g3": "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS",
}
KEYLESS_COUNTS = (0, 1, 5, 300, 1025)
KEYED = ("ks512", "mult1024", "ggsw", "wop512", "bool512", "bool1024", "u128-256", "u128-2048")
KEYED_COUNTS = (0, 1, 5, 300)
# (nbits, cbs_level, nout, npoly): three tree bits + two rotation bits at three levels; one tree bit + three
# rotation bits at two levels.  The vertical_packing query of the header has no nout (one output).
VP_TUPLES = ((5, 3, 1, 8), (4, 2, 2, 2))
LUT_COUNT = 2


def _keyless(name):
    import tfhe_mi355.parameters as P
    from tfhe_mi355 import Engine

    return Engine(getattr(P, name), 0), {}


def _bool(N, k, L, B, ksB, ksL):
    """test_async_guards_gpu._bool_engine without its CPU reference"""
    import dataclasses

    from tfhe_mi355 import Engine
    from tfhe_mi355 import boolean as Bm

    n = 3
    p = dataclasses.replace(Bm.DEFAULT_PARAMETERS, lwe_dimension=n, glwe_dimension=k, polynomial_size=N, pbs_base_log=B,
                            pbs_level=L, ks_base_log=ksB, ks_level=ksL, name=f"scratch_bool_{N}_{k}")
    rng = np.random.default_rng(N + k)
    eng = Engine(p, 0)
    eng.upload_bootstrap_key_u32(rng.integers(0, 1 << 32, n * L * (k + 1) * (k + 1) * N, dtype=np.uint32))
    eng.upload_keyswitch_key_u32(rng.integers(0, 1 << 32, k * N * ksL * (n + 1), dtype=np.uint32))
    return eng, {}


def _u128(N, k, L, B):
    """test_async_guards_gpu._u128_engine without its CPU reference"""
    import pbs128_cases as C
    import pbs128_reference as R
    from tfhe_mi355 import Engine

    n = 2
    eng = Engine.for_u128(C.params(n, N, k, L, B), 0)
    eng.upload_bootstrap_key_u128(R.uniform(N + k, n * L * (k + 1) * (k + 1) * N).reshape(n, L, k + 1, k + 1, N, 2))
    return eng, {}


def make_engine(key):
    """(engine, {name: keyswitching key object})"""
    import test_async_guards_gpu as G

    if key in KEYLESS:
        return _keyless(KEYLESS[key])
    if key in G.BOOL_SHAPES:
        return _bool(*G.BOOL_SHAPES[key])
    if key in G.U128_SHAPES:
        return _u128(*G.U128_SHAPES[key])
    E = G.FACTORIES[key](None)
    return E.eng, {w: getattr(E, "key_" + w) for w in ("mfma", "wide") if hasattr(E, "key_" + w)}


def queries(key, eng, ks_keys):
    """{query name with its shape arguments: f(count)}"""
    q = {
        "programmable_bootstrap": eng.pbs_scratch_bytes,
        "keyswitch": eng.ks_scratch_bytes,
        "keyswitch_programmable_bootstrap": eng.ks_pbs_scratch_bytes,
        "programmable_bootstrap_keyswitch": eng.pbs_ks_scratch_bytes,
    }
    if key in KEYLESS:
        return q
    q.update({
        "packing_keyswitch": eng.pks_scratch_bytes,
        "glwe_mult": eng.glwe_mult_scratch_bytes,
        "lwe_mult": eng.lwe_mult_scratch_bytes,
        "private_functional_packing_keyswitch": eng.pfpks_scratch_bytes,
        "extract_bits": eng.extract_bits_scratch_bytes,
        "programmable_bootstrap_u32": eng.pbs_u32_scratch_bytes,
        "blind_rotate_u32": eng.blind_rotate_u32_scratch_bytes,
        "keyswitch_u32": eng.ks_u32_scratch_bytes,
        "programmable_bootstrap_u128": eng.pbs_u128_scratch_bytes,
        "blind_rotate_u128": eng.blind_rotate_u128_scratch_bytes,
    })
    for name, k in ks_keys.items():
        q[f"keyswitch_with_key({name})"] = lambda c, k=k: eng.keyswitch_with_key_scratch_bytes(k, c)
    for order in (0, 1):
        q[f"boolean_gates(pbs_order={order})"] = lambda c, o=order: eng.boolean_gates_scratch_bytes(c, o)
        q[f"boolean_mux(pbs_order={order})"] = lambda c, o=order: eng.boolean_mux_scratch_bytes(c, o)
    for nbits, level, nout, npoly in VP_TUPLES:
        q[f"vertical_packing(npoly={npoly})"] = lambda c, m=npoly: eng.vertical_packing_scratch_bytes(m, c)
        q[f"circuit_bootstrap(cbs_level={level})"] = lambda c, lv=level: eng.circuit_bootstrap_scratch_bytes(lv, c)
        q[f"circuit_bootstrap_vertical_packing(nbits={nbits},cbs_level={level},lut_count={LUT_COUNT},nout={nout},"
          f"npoly={npoly})"] = (lambda c, a=(nbits, level, nout, npoly):
                                eng.circuit_bootstrap_vertical_packing_scratch_bytes(a[0], a[1], LUT_COUNT, a[2], a[3], c))
    return q


def measure(key):
    """{query: {count: bytes}} of the queries that succeed on engine `key`"""
    from tfhe_mi355._lib import EngineError

    eng, ks_keys = make_engine(key)
    try:
        out = {}
        for name, f in queries(key, eng, ks_keys).items():
            for count in KEYLESS_COUNTS if key in KEYLESS else KEYED_COUNTS:
                try:
                    out.setdefault(name, {})[str(count)] = int(f(count))
                except EngineError:
                    pass
        return out
    finally:
        for k in ks_keys.values():
            k.close()
        eng.close()


def dump(table):
    """the golden file's text: JSON, one line per query"""
    engines = []
    for key in sorted(table):
        rows = [f"  {json.dumps(name)}: {json.dumps(table[key][name], sort_keys=True)}" for name in sorted(table[key])]
        engines.append(f" {json.dumps(key)}: {{\n" + ",\n".join(rows) + "\n }")
    return "{\n" + ",\n".join(engines) + "\n}\n"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("key", list(KEYLESS) + list(KEYED))
def test_scratch_queries_return_the_recorded_bytes(golden, key):
    got, want = measure(key), golden[key]
    print(f"{key}: {got}")
    assert sorted(got) == sorted(want), "another set of queries succeeds"
    for name in want:
        assert got[name] == want[name], f"{key} {name}: {got[name]} bytes, recorded {want[name]}"


if __name__ == "__main__":
    import conftest  # noqa: F401  (puts the repository and the package on sys.path)

    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_scratch_sizes_gpu.py --write")
    table = {key: measure(key) for key in list(KEYLESS) + list(KEYED)}
    with open(GOLDEN, "w") as f:
        f.write(dump(table))
    print(f"wrote {GOLDEN}: {sum(len(v) for q in table.values() for v in q.values())} values")
