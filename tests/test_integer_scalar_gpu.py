"""The radix operations with a clear operand on the device path (integer._DeviceOps) against the same DAG on the
host path with the oracle engine: PARAM_MESSAGE_2_CARRY_2_KS_PBS at lwe_dimension = 8, both server keys from one
ClientKey seed, the case list of integer_scalar_cases.py.  Every result must equal the host DAG's bit for bit, with
the same degree, noise, pbs_count and launches, stay resident on the GPU and decrypt to the integer answer.  A per-row
case hands batches 0 and 1 over as numpy arrays and batch 2 as a torch tensor on the device.  Every fused layer is one
block-layer call, one batched KS+PBS and one more block-layer call, each block-layer call one engine call, whether
it is the plain layer or the one with a clear digit per row; a device tensor of clear operands is never copied; and
a captured hipGraph of scalar_lt follows clear operands and ciphertext words rewritten in place."""
import numpy as np
import pytest

import integer_scalar_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scalar_keys():
    ck, gpu = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    return ck, gpu, cpu


def _same(g, c):
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _watch(monkeypatch, sks):
    """The calls of `sks` in order: "B" ops.block_layer or ops.clear_block_layer, "P" a batched KS+PBS (ops.pbs_buffer,
    ops.pbs_buffer_indexed), "T" a trivial PBS, "E" one lwe_block_layer_async or lwe_clear_block_layer_async call of
    the engine, "H" a host-to-device copy (ops.from_host, ops.index_from_host), and the per-block paths "C"
    ops.copy_block, "M" ops.mul_add, "S" ops.set_trivial, "R" ops.roll, "Q" ops.pbs_rows; those made inside one
    _PbsLayer.flush_fused or flush_clear are grouped in a list of their own."""
    from tfhe_mi355.integer import _PbsLayer

    log, inside = [], []
    ops, eng = sks.ops, sks.ops.eng

    def tap(obj, name, tag):
        real = getattr(obj, name)

        def tapped(*a, **k):
            (inside[-1] if inside else log).append(tag)
            return real(*a, **k)
        monkeypatch.setattr(obj, name, tapped)

    for name, tag in (("block_layer", "B"), ("clear_block_layer", "B"), ("pbs_buffer", "P"), ("pbs_buffer_indexed", "P"),
                      ("trivial_pbs", "T"), ("copy_block", "C"), ("mul_add", "M"), ("set_trivial", "S"), ("roll", "R"),
                      ("pbs_rows", "Q"), ("from_host", "H"), ("index_from_host", "H")):
        tap(ops, name, tag)
    tap(eng, "lwe_block_layer_async", "E")
    tap(eng, "lwe_clear_block_layer_async", "E")

    def group(name):
        real = getattr(_PbsLayer, name)

        def grouped(layer, reqs):
            if layer.sk is not sks:
                return real(layer, reqs)
            inside.append([])
            try:
                return real(layer, reqs)
            finally:
                log.append(inside.pop())
        monkeypatch.setattr(_PbsLayer, name, grouped)

    group("flush_fused")
    group("flush_clear")
    return log


def _calls(events):
    """a fused layer's events without its trivial PBS and its uploads"""
    return [e for e in events if e not in "TH"]


FUSED = (["B", "E", "P", "B", "E"], ["B", "E", "E", "P", "B", "E"])    # the second: a zero-test sum of five terms
ALL_TRIVIAL = (["B", "E"], ["B", "E", "E"], ["B", "E", "B", "E"], ["B", "E", "E", "B", "E"])   # no PBS; with a + 1 after


def _device_rows(gpu, clear):
    import torch

    return torch.from_numpy(clear.view(np.int64)).to(gpu.ops.device)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_scalar_ops_equal_host_scalar_ops(scalar_keys, monkeypatch, case):
    import torch

    ck, gpu, cpu = scalar_keys
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc]
    want, nblocks = C.expected(case), C.result_blocks(case)
    log = _watch(monkeypatch, gpu)
    for b in range(case.batches):
        lhs = C.operand(case, gpu, enc, b)
        clear = C.clear_operand(case, b)
        on_device = case.form == "rows" and b == 2
        handed = _device_rows(gpu, clear) if on_device else clear
        kept = handed.clone() if on_device else handed
        del log[:]
        res = C.apply(case, gpu, lhs, handed, b)
        events = list(log)
        assert isinstance(res.data, torch.Tensor) and res.data.is_cuda, "the result is not resident on the GPU"
        g = gpu.to_host(res)
        c = cpu.to_host(C.run(case, cpu, enc, b)[0])
        assert (gpu.pbs_count, gpu.launches) == (cpu.pbs_count, cpu.launches) == C.shadow(case, b)
        _same(g, c)
        assert C.decrypt(ck, g, nblocks) == want[b * C.K:(b + 1) * C.K]
        if on_device:
            assert torch.equal(handed, kept)
        layers = [e for e in events if isinstance(e, list)]
        outside = [e for e in events if not isinstance(e, list)]
        flat = outside + sum(layers, [])
        for layer in layers:
            assert set(layer) <= set("BEPTH"), layer
            assert _calls(layer) in FUSED + ALL_TRIVIAL, layer
            if case.variant in ("unchecked", "clean") and "T" not in layer:   # "T": the map of a trivial sign
                assert _calls(layer) in FUSED, layer
        assert gpu.launches == outside.count("P") + sum("P" in e for e in layers)
        # a numpy array of clear operands is uploaded once per call, a device tensor and a Python int never
        per_call = 1 if case.form == "rows" and not on_device else 0
        if case.variant in ("unchecked", "clean") and b > 0 and case.form == "rows":
            assert flat.count("H") == per_call, flat           # the LUT stacks came with batch 0
        if case.variant == "dirty" or (case.op in C.ARITHMETIC and case.variant != "unchecked"):
            continue                                  # full_propagate / the carry propagation: the multiply DAG's path
        if case.op in C.ARITHMETIC:                   # one block-layer call, no PBS
            assert [e for e in outside if e != "H"] in (["B", "E"], ["B"]) and not layers
            assert case.form == "int" or [e for e in outside if e != "H"] == ["B", "E"]
        elif case.form == "rows":                     # fused layers alone; max / min: and the trivial radix's one call
            trivial_radix = ["B", "E"] if case.op in C.SELECT else []
            assert [e for e in outside if e not in "HS"] == trivial_radix, outside
            if case.variant in ("unchecked", "clean"):
                assert len(layers) == gpu.launches
        else:                                         # one int: no per-block arithmetic; the bitwise ops' unfused layer
            assert not set(outside) & set("CMR"), outside
    assert all(np.array_equal(e.data, d) for e, d in zip(enc, before)), "an input batch was written"


def test_unchecked_scalar_add_per_row_is_one_engine_call(scalar_keys, monkeypatch):
    ck, gpu, cpu = scalar_keys
    for op in C.ARITHMETIC:
        case = next(c for c in C.CASES if c.id == f"{op}-unchecked-b8-rows")
        enc = C.encrypt(ck, case)
        lhs, clear = C.operand(case, gpu, enc, 1), C.clear_operand(case, 1)
        handed = _device_rows(gpu, clear)
        log = _watch(monkeypatch, gpu)
        res = gpu.to_host(C.apply(case, gpu, lhs, handed, 1))
        assert log == ["B", "E"] and (gpu.pbs_count, gpu.launches) == (0, 0)
        monkeypatch.undo()
        _same(res, cpu.to_host(C.run(case, cpu, enc, 1)[0]))
        assert C.decrypt(ck, res, 8) == C.expected(case)[C.K:2 * C.K]


@pytest.mark.parametrize("op", ["scalar_sub", "scalar_bitand", "scalar_eq", "scalar_lt", "scalar_max"])
def test_a_device_tensor_of_clear_operands_is_never_copied(scalar_keys, monkeypatch, op):
    """the default form on clean operands: after a first call every LUT stack is on the device, and a second call
    with other clear operands in the same tensor makes no host-to-device copy"""
    ck, gpu, cpu = scalar_keys
    case = next(c for c in C.CASES if c.id == f"{op}-clean-b5-rows")
    enc = C.encrypt(ck, case)
    handed = _device_rows(gpu, C.clear_operand(case, 0))
    C.apply(case, gpu, C.operand(case, gpu, enc, 0), handed, 0)
    handed.copy_(_device_rows(gpu, C.clear_operand(case, 1)))
    lhs = C.operand(case, gpu, enc, 1)
    for name in ("from_host", "index_from_host"):
        monkeypatch.setattr(gpu.ops, name, lambda data, name=name: pytest.fail(f"{name} on the second call"))
    res = C.apply(case, gpu, lhs, handed, 0)
    monkeypatch.undo()
    res = gpu.to_host(res)
    _same(res, cpu.to_host(C.run(case, cpu, enc, 1)[0]))
    assert C.decrypt(ck, res, C.result_blocks(case)) == C.expected(case)[C.K:2 * C.K]


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

    for name in ("lwe_block_layer_async", "lwe_clear_block_layer_async", "keyswitch_programmable_bootstrap_async",
                 "trivial_pbs_async"):
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


def test_graph_replay_follows_clear_operands_and_ciphertexts(scalar_keys, monkeypatch):
    """scalar_lt_parallelized at 3 blocks with a device tensor of clear operands, captured after a warm-up: the
    replay equals the eager run; with the clear tensor overwritten in place, and then the ciphertext words, the
    replays equal eager runs on the same inputs"""
    import torch

    ck, gpu, cpu = scalar_keys
    case = next(c for c in C.CASES if c.id == "scalar_lt-clean-b3-rows")
    enc = C.encrypt(ck, case)
    clears = [C.clear_operand(case, b) for b in range(2)]

    def host(b, clear):
        return cpu.to_host(cpu.scalar_lt_parallelized(C.batch_rows(enc[0], b), clear))

    x_d = gpu.to_device(C.batch_rows(enc[0], 0))
    c_d = _device_rows(gpu, clears[0])

    def dag():
        return gpu.scalar_lt_parallelized(x_d, c_d)

    _same(gpu.to_host(dag()), host(0, clears[0]))       # warm-up: the LUT stacks and the scratch are on the device
    graph, out = _capture(monkeypatch, gpu, dag)
    graph.replay()
    torch.cuda.synchronize()
    _same(gpu.to_host(out), host(0, clears[0]))
    c_d.copy_(_device_rows(gpu, clears[1]))             # new clear operands, in place
    graph.replay()
    torch.cuda.synchronize()
    _same(gpu.to_host(out), host(0, clears[1]))
    assert not np.array_equal(host(0, clears[1]).data, host(0, clears[0]).data)
    x_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc[0], 1).data))     # new ciphertext words, in place
    graph.replay()
    torch.cuda.synchronize()
    _same(gpu.to_host(out), host(1, clears[1]))
    _same(gpu.to_host(dag()), host(1, clears[1]))       # and the eager run on the device agrees
    assert C.decrypt(ck, gpu.to_host(out), 1) == C.expected(case)[C.K:2 * C.K]
    graph = None
