"""The unsigned radix division and unsigned_overflowing_sub on the device path (integer._DeviceOps) against the same
DAG on the host path with the oracle engine: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8, both server keys
from one ClientKey seed, the case list of integer_div_cases.py.  Every result must equal the host DAG's bit for bit,
with the same degree, noise, pbs_count and launches, stay resident on the GPU and decrypt to the integer answer; the
device path must be fused layers and nothing else (block layer, batched KS+PBS, block layer, trivial PBS in between);
and a deep division must reach a steady state of its device tables and replay from one captured hipGraph."""
import numpy as np
import pytest

import integer_div_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu

DEEP_BLOCKS = 32                 # T = 64 iterations, about 515 distinct layers: more than the layer-table LRU holds


@pytest.fixture(scope="module")
def div_keys():
    ck, gpu = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    return ck, gpu, cpu


def _same(g, c):
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _watch(monkeypatch, sks):
    """The calls of `sks` in order: "B" ops.block_layer, "P" ops.pbs_buffer (a batched KS+PBS), "T" a trivial PBS,
    "E" one lwe_block_layer_async call of the engine, "H" a host-to-device copy (ops.from_host, ops.index_from_host),
    and the per-block paths "C" ops.copy_block, "M" ops.mul_add, "S" ops.set_trivial, "R" ops.roll, "Q" ops.pbs_rows;
    those made inside one _PbsLayer.flush_fused are grouped in a list of their own."""
    from tfhe_mi355.integer import _PbsLayer

    log, inside = [], []
    ops, eng = sks.ops, sks.ops.eng

    def tap(obj, name, tag):
        real = getattr(obj, name)

        def tapped(*a, **k):
            (inside[-1] if inside else log).append(tag)
            return real(*a, **k)
        monkeypatch.setattr(obj, name, tapped)

    for name, tag in (("block_layer", "B"), ("pbs_buffer", "P"), ("trivial_pbs", "T"), ("copy_block", "C"),
                      ("mul_add", "M"), ("set_trivial", "S"), ("roll", "R"), ("pbs_rows", "Q"), ("from_host", "H"),
                      ("index_from_host", "H")):
        tap(ops, name, tag)
    tap(eng, "lwe_block_layer_async", "E")
    fused = _PbsLayer.flush_fused

    def grouped(layer, reqs):
        if layer.sk is not sks:
            return fused(layer, reqs)
        inside.append([])
        try:
            return fused(layer, reqs)
        finally:
            log.append(inside.pop())
    monkeypatch.setattr(_PbsLayer, "flush_fused", grouped)
    return log


def _calls(events):
    """a fused layer's events without its trivial PBS and its table uploads"""
    return [e for e in events if e not in "TH"]


FUSED = (["B", "E", "P", "B", "E"], ["B", "E", "E", "P", "B", "E"])    # the second: a zero-test sum of five terms
ALL_TRIVIAL = (["B", "E"], ["B", "E", "E"])                            # every request of the layer trivial: no PBS


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_division_equals_host_division(div_keys, monkeypatch, case):
    import torch

    ck, gpu, cpu = div_keys
    enc = C.encrypt(ck, case)
    all_enc = enc["lhs"] + enc["rhs"]
    before = [e.data.copy() for e in all_enc]
    want = C.expected(case)
    log = _watch(monkeypatch, gpu)
    for b in range(C.ROWS // C.K):
        lhs, rhs = C.operands(case, gpu, enc, b)
        del log[:]
        results = C.apply(case, gpu, lhs, rhs, b)
        events = list(log)
        for res in results:
            assert isinstance(res.data, torch.Tensor) and res.data.is_cuda, "the result is not resident on the GPU"
        g = [gpu.to_host(res) for res in results]
        c = [cpu.to_host(res) for res in C.run(case, cpu, enc, b)[0]]
        assert (gpu.pbs_count, gpu.launches) == (cpu.pbs_count, cpu.launches) == C.shadow(case)
        assert len(g) == len(c) == case.results
        for x, y in zip(g, c):
            _same(x, y)
        assert C.decrypted(ck, case, g) == want[b * C.K:(b + 1) * C.K]
        layers = [e for e in events if isinstance(e, list)]
        outside = [e for e in events if not isinstance(e, list)]
        for layer in layers:
            assert set(layer) <= set("BEPTH"), layer
            assert _calls(layer) in FUSED + ALL_TRIVIAL, layer
        assert gpu.launches == outside.count("P") + sum("P" in e for e in layers)
        if case.variant == "dirty":
            continue                                  # full_propagate first: the multiply DAG's launch path, as pinned
        # fused layers alone: no copy_block, mul_add, set_trivial, roll, unfused layer or block-layer call between them
        assert not [e for e in outside if e != "H"], outside
        if case.variant in ("unchecked", "clean"):
            assert len(layers) == gpu.launches and all(_calls(layer) in FUSED for layer in layers)
    assert all(np.array_equal(e.data, d) for e, d in zip(all_enc, before)), "an input batch was written"


def test_a_clean_division_is_a_list_of_fused_layers(div_keys, monkeypatch):
    """div_rem over 8 blocks: 99 fused layers of exactly B E P B E and nothing between them.  A second E before the
    PBS only where compare_blocks_with_zero sums five upper divisor blocks (block_layer chains the fifth term): the
    iterations with 5 upper blocks or more, msb_bit_set = 0 .. 6."""
    ck, gpu, cpu = div_keys
    case = next(c for c in C.CASES if c.id == "div_rem-clean-b8")
    enc = C.encrypt(ck, case)
    lhs, rhs = C.operands(case, gpu, enc, 0)
    C.apply(case, gpu, lhs, rhs, 0)                     # tables on the device
    log = _watch(monkeypatch, gpu)
    results = C.apply(case, gpu, lhs, rhs, 0)
    assert all(isinstance(e, list) for e in log), [e for e in log if not isinstance(e, list)]
    assert "H" not in sum(log, [])
    calls = [_calls(e) for e in log]
    assert len(calls) == 99 == gpu.launches
    assert all(e in FUSED for e in calls)
    wide = [k for k, e in enumerate(calls) if e == FUSED[1]]
    # iterations 0 .. 6 take 4, 4, 5, 5, 6, 6, 6 layers; the zero test's first pass is the second layer of each
    assert wide == [1, 5, 9, 14, 19, 25, 31]
    assert C.decrypted(ck, case, [gpu.to_host(r) for r in results]) == C.expected(case)[:C.K]


# ---- depth: 32 blocks -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep(div_keys):
    """One row of 32 blocks (FheUint64) on the GPU key, and its warm-up call with the host-to-device copies counted."""
    from tfhe_mi355 import integer

    ck, gpu, _ = div_keys
    cks = integer.ClientKey(ck, DEEP_BLOCKS)
    rng = np.random.default_rng(3232)
    pairs = [(int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(1, 2 ** 21))),
             (int(rng.integers(0, 2 ** 63)), int(rng.integers(2 ** 40, 2 ** 41)))]
    ck._enc_counter = 3232 << 8
    enc = [(cks.encrypt(np.asarray([n], dtype=np.uint64)), cks.encrypt(np.asarray([d], dtype=np.uint64))) for n, d in pairs]
    a_d, b_d = gpu.to_device(enc[0][0]), gpu.to_device(enc[0][1])
    copies = []
    real = {name: getattr(gpu.ops, name) for name in ("from_host", "index_from_host")}
    for name, f in real.items():
        setattr(gpu.ops, name, lambda data, f=f, name=name: (copies.append(name), f(data))[1])
    try:
        gpu.pbs_count = gpu.launches = 0
        q, r = gpu.div_rem_parallelized(a_d, b_d)
        first = {"copies": list(copies), "launches": gpu.launches, "q": gpu.to_host(q), "r": gpu.to_host(r)}
    finally:
        for name in real:
            delattr(gpu.ops, name)
    return {"cks": cks, "pairs": pairs, "enc": enc, "a_d": a_d, "b_d": b_d, "first": first}


def _deep_answer(deep, results, which):
    n, d = deep["pairs"][which]
    got = tuple(int(deep["cks"].decrypt(x)[0]) for x in results)
    assert got == (n // d, n % d), (got, n, d)


def test_steady_state_at_depth(div_keys, deep, monkeypatch):
    """A second div_rem_parallelized on operands of the same shape makes no host-to-device copy, though the division
    has more distinct layers than _DeviceOps keeps layer tables: one LUT stack per layer in that LRU would miss on
    every layer of every call."""
    from tfhe_mi355 import integer

    ck, gpu, _ = div_keys
    first = deep["first"]
    _deep_answer(deep, (first["q"], first["r"]), 0)
    assert first["launches"] == C.shadow_of_clean_division(DEEP_BLOCKS)[1] > integer._DeviceOps.CACHE_ENTRIES
    assert "from_host" in first["copies"] and "index_from_host" in first["copies"]
    assert first["copies"].count("from_host") < 32             # the plan's one stack and the trivial PBS' LUTs
    plans = {**gpu.ops._plans._d, **gpu.ops._plans._pinned}
    plan, = [p for key, p in plans.items() if key[0] == "div_rem" and len(key[1][1]) == DEEP_BLOCKS]
    assert len(plan.luts) == 15 and plan.stack.shape[0] == 15
    assert len(plan.indexes) == first["copies"].count("index_from_host") <= first["launches"]
    stacks = len(gpu.ops._stacks)
    copies = []
    for name in ("from_host", "index_from_host"):
        monkeypatch.setattr(gpu.ops, name,
                            lambda data, name=name: copies.append(name) or pytest.fail(f"{name} on the second call"))
    gpu.pbs_count = gpu.launches = 0
    q, r = gpu.div_rem_parallelized(deep["a_d"], deep["b_d"])
    assert copies == [] and gpu.launches == first["launches"] and len(gpu.ops._stacks) == stacks
    q, r = gpu.to_host(q), gpu.to_host(r)
    _same(q, first["q"])
    _same(r, first["r"])
    _deep_answer(deep, (q, r), 0)


# ---- hipGraph -----------------------------------------------------------------------------------------------------------
def _capture(monkeypatch, gpu, dag):
    """`dag` captured into one hipGraph; every engine launch of the capture must go to the one capturing stream (no
    stream argument, the current stream the same throughout: a chain, no parallel branches) and nothing may be
    uploaded"""
    import torch

    streams, eng = [], gpu.ops.eng

    def tap(name):
        real = getattr(eng, name)

        def tapped(*a, stream=None, **k):
            streams.append((stream, torch.cuda.current_stream().cuda_stream))
            return real(*a, stream=stream, **k)
        monkeypatch.setattr(eng, name, tapped)

    for name in ("lwe_block_layer_async", "keyswitch_programmable_bootstrap_async", "trivial_pbs_async"):
        tap(name)
    for name in ("from_host", "index_from_host"):
        monkeypatch.setattr(gpu.ops, name, lambda data, name=name: pytest.fail(f"{name} during the capture"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dag()
    monkeypatch.undo()
    assert streams and all(s is None for s, _ in streams) and len({c for _, c in streams}) == 1
    return graph, out


def test_graph_replay_of_a_division(div_keys, monkeypatch):
    """div_rem_parallelized at 3 blocks captured after a warm-up: the replay equals the eager run, follows operand
    words rewritten in place, and decrypts"""
    import torch

    ck, gpu, cpu = div_keys
    case = next(c for c in C.CASES if c.id == "div_rem-clean-b3")
    other = C.Case("div_rem", "clean", 3, 4242)
    enc, enc2 = C.encrypt(ck, case), C.encrypt(ck, other)

    def host(e):
        return [cpu.to_host(x) for x in cpu.div_rem_parallelized(C.batch_rows(e["lhs"][0], 1), C.batch_rows(e["rhs"][0], 1))]

    ref, ref2 = host(enc), host(enc2)
    assert not np.array_equal(ref[0].data, ref2[0].data)
    a_d, b_d = (gpu.to_device(C.batch_rows(enc[n][0], 1)) for n in ("lhs", "rhs"))

    def dag():
        return gpu.div_rem_parallelized(a_d, b_d)

    for g, c in zip(dag(), ref):                        # warm-up: LUTs, the table plan and scratch are on the device
        _same(gpu.to_host(g), c)
    graph, out = _capture(monkeypatch, gpu, dag)
    graph.replay()
    torch.cuda.synchronize()
    for g, c in zip(out, ref):
        _same(gpu.to_host(g), c)
    a_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc2["lhs"][0], 1).data))   # new operand words, in place
    b_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc2["rhs"][0], 1).data))
    graph.replay()
    torch.cuda.synchronize()
    for g, c in zip(out, ref2):
        _same(gpu.to_host(g), c)
    assert C.decrypted(ck, other, [gpu.to_host(g) for g in out]) == C.expected(other)[C.K:2 * C.K]
    graph = None


def test_graph_replay_at_depth(div_keys, deep, monkeypatch):
    """the 32-block row: one graph of the whole division, replayed on the warm-up's operands and on new ones"""
    import torch

    ck, gpu, _ = div_keys
    a_d, b_d = deep["a_d"], deep["b_d"]
    graph, out = _capture(monkeypatch, gpu, lambda: gpu.div_rem_parallelized(a_d, b_d))
    graph.replay()
    torch.cuda.synchronize()
    _deep_answer(deep, [gpu.to_host(x) for x in out], 0)
    a_d.data.copy_(gpu.ops.from_host(deep["enc"][1][0].data))
    b_d.data.copy_(gpu.ops.from_host(deep["enc"][1][1].data))
    graph.replay()
    torch.cuda.synchronize()
    _deep_answer(deep, [gpu.to_host(x) for x in out], 1)
    a_d.data.copy_(gpu.ops.from_host(deep["enc"][0][0].data))                 # as the other tests of the module found them
    b_d.data.copy_(gpu.ops.from_host(deep["enc"][0][1].data))
    graph = None
