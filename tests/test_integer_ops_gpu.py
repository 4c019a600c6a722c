"""The radix integer operations beyond the multiply DAG on the device path (integer._DeviceOps: one
lwe_block_layer_kernel launch assembles the PBS input rows of a layer, one more scatters its outputs) against the
same DAG on the host path with the oracle engine: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8, both server
keys from one ClientKey seed, the case list of integer_ops_cases.py.  Every result must equal the host DAG's bit
for bit, with the same degree, noise, pbs_count and launches, and decrypt to the integer answer."""
import numpy as np
import pytest

import integer_ops_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops_keys():
    ck, gpu = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    return ck, gpu, cpu


def _same(g, c):
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _watch(monkeypatch, sks):
    """The calls of `sks` in order: "B" ops.block_layer, "P" ops.pbs_buffer (a batched KS+PBS), "T" a trivial PBS,
    "E" one lwe_block_layer_async call of the engine; those made inside one _PbsLayer.flush_fused are grouped in a
    list of their own."""
    from tfhe_mi355.integer import _PbsLayer

    log, inside = [], []
    ops, eng = sks.ops, sks.ops.eng

    def tap(obj, name, tag):
        real = getattr(obj, name)

        def tapped(*a, **k):
            (inside[-1] if inside else log).append(tag)
            return real(*a, **k)
        monkeypatch.setattr(obj, name, tapped)

    tap(ops, "block_layer", "B")
    tap(ops, "pbs_buffer", "P")
    tap(ops, "trivial_pbs", "T")
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


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_ops_equal_host_ops(ops_keys, monkeypatch, case):
    import torch

    ck, gpu, cpu = ops_keys
    enc = C.encrypt(ck, case)
    all_enc = enc["lhs"] + enc["rhs"] + [enc["cond"]]
    before = [e.data.copy() for e in all_enc]
    want, nblocks = C.expected(case)
    log = _watch(monkeypatch, gpu)
    for b in range(C.ROWS // C.K):
        del log[:]
        res = C.run(case, gpu, enc, b)
        assert isinstance(res.data, torch.Tensor) and res.data.is_cuda, "the result is not resident on the GPU"
        g = gpu.to_host(res)
        c = cpu.to_host(C.run(case, cpu, enc, b))
        assert (gpu.pbs_count, gpu.launches) == (cpu.pbs_count, cpu.launches) == C.shadow(case)
        _same(g, c)
        assert C.decrypt(ck, g, nblocks) == want[b * C.K:(b + 1) * C.K]
        # every fused layer: ONE block-layer call before its PBS and ONE after (trivial PBS in between)
        layers = [e for e in log if isinstance(e, list)]
        for events in layers:
            calls = [e for e in events if e in "BP"]
            assert calls in (["B", "P", "B"], ["B"], ["B", "B"]), events   # the last two: every request trivial
            if case.variant != "trivial":
                assert calls == ["B", "P", "B"] and "T" not in events
        outside = [e for e in log if not isinstance(e, list)]
        assert outside.count("B") == (1 if case.op in ("neg", "sub") else 0)   # unchecked_neg: one call, no PBS
        assert gpu.launches == outside.count("P") + sum("P" in e for e in layers)
        if case.op not in ("eq", "ne"):   # the sums of eq / ne over more than 4 blocks go on in further calls
            assert sum(e.count("E") for e in layers) + outside.count("E") == \
                sum(e.count("B") for e in layers) + outside.count("B")
    assert all(np.array_equal(e.data, d) for e, d in zip(all_enc, before)), "an input batch was written"


def test_wide_sums_take_further_calls_in_order(ops_keys, monkeypatch):
    """eq over 8 blocks sums 8 block comparisons: 4 terms in the layer's call, then 3 + 1 in place in two more,
    in stream order, before the PBS"""
    ck, gpu, cpu = ops_keys
    case = next(c for c in C.CASES if c.id == "eq-clean-b8")
    enc = C.encrypt(ck, case)
    log = _watch(monkeypatch, gpu)
    res = gpu.to_host(C.run(case, gpu, enc, 0))
    _same(res, cpu.to_host(C.run(case, cpu, enc, 0)))
    layers = [e for e in log if isinstance(e, list)]
    assert layers == [["B", "E", "P", "B", "E"], ["B", "E", "E", "E", "P", "B", "E"]]


def test_graph_replay_of_a_comparison_and_a_select(ops_keys):
    """lt_parallelized + if_then_else_parallelized (the minimum, spelled out) captured into one hipGraph: the replay
    equals the eager run and follows operand words rewritten in place"""
    import torch

    ck, gpu, cpu = ops_keys
    case = next(c for c in C.CASES if c.id == "min-clean-b5")
    other = C.Case("min", "clean", 5, 4242)
    enc, enc2 = C.encrypt(ck, case), C.encrypt(ck, other)

    def host(e):
        a, b = C.batch_rows(e["lhs"][0], 0), C.batch_rows(e["rhs"][0], 0)
        return cpu.to_host(cpu.if_then_else_parallelized(cpu.lt_parallelized(a, b), a, b))

    ref, ref2 = host(enc), host(enc2)
    assert not np.array_equal(ref.data, ref2.data)
    a_d, b_d = (gpu.to_device(C.batch_rows(enc[n][0], 0)) for n in ("lhs", "rhs"))

    def dag():
        return gpu.if_then_else_parallelized(gpu.lt_parallelized(a_d, b_d), a_d, b_d)

    _same(gpu.to_host(dag()), ref)                      # warm-up: LUTs, layer tables and scratch are on the device
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dag()
    graph.replay()
    torch.cuda.synchronize()
    _same(gpu.to_host(out), ref)
    a_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc2["lhs"][0], 0).data))   # new operand words, in place
    b_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc2["rhs"][0], 0).data))
    graph.replay()
    torch.cuda.synchronize()
    _same(gpu.to_host(out), ref2)
    assert C.decrypt(ck, gpu.to_host(out), 5) == C.expected(other)[0][:C.K]
    graph = None
