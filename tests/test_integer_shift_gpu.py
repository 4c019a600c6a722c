"""The radix shifts and rotations by a clear and by an encrypted amount and scalar_mul on the device path
(integer._DeviceOps) against the same DAG on the host path with the oracle engine: PARAM_MESSAGE_2_CARRY_2_KS_PBS at
lwe_dimension = 8, both server keys from one ClientKey seed, the case list of integer_shift_cases.py.  Every result
must equal the host DAG's bit for bit, with the same degree, noise, pbs_count and launches, stay resident on the
GPU and decrypt to the integer answer; and the device path must reach the block-layer kernel and the batched KS+PBS
and nothing else: no per-block launch, no roll, one engine call per block-layer call."""
import numpy as np
import pytest

import integer_shift_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shift_keys():
    ck, gpu = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    return ck, gpu, cpu


def _same(g, c):
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _watch(monkeypatch, sks):
    """The calls of `sks` in order: "B" ops.block_layer, "P" ops.pbs_buffer (a batched KS+PBS), "T" a trivial PBS,
    "E" one lwe_block_layer_async call of the engine, and the per-block paths "C" ops.copy_block, "M" ops.mul_add,
    "S" ops.set_trivial, "R" ops.roll, "Q" ops.pbs_rows (the unfused layer with its torch.cat); those made inside one
    _PbsLayer.flush_fused are grouped in a list of their own."""
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
                      ("mul_add", "M"), ("set_trivial", "S"), ("roll", "R"), ("pbs_rows", "Q")):
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


def _check_fused_layers(case, layers):
    """every fused layer: ONE block-layer call, ONE batched KS+PBS, ONE block-layer call, each block-layer call one
    engine call (T <= 32 bits here, so a barrel stage is one call too); trivial PBS in between"""
    for events in layers:
        assert set(events) <= set("BEPT"), events
        calls = [e for e in events if e in "BEP"]
        assert calls in (["B", "E", "P", "B", "E"], ["B", "E"], ["B", "E", "B", "E"]), events   # the last two: all trivial
        if not C._trivial(case):
            assert calls == ["B", "E", "P", "B", "E"] and "T" not in events


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_shifts_equal_host_shifts(shift_keys, monkeypatch, case):
    import torch

    ck, gpu, cpu = shift_keys
    enc = C.encrypt(ck, case)
    all_enc = enc["lhs"] + enc["rhs"]
    before = [e.data.copy() for e in all_enc]
    want = C.expected(case)
    log = _watch(monkeypatch, gpu)
    for b in range(case.rows // C.K):
        lhs, rhs = C.operands(case, gpu, enc, b)
        del log[:]
        res = C.apply(case, gpu, lhs, rhs, b)
        events = list(log)
        assert isinstance(res.data, torch.Tensor) and res.data.is_cuda, "the result is not resident on the GPU"
        g = gpu.to_host(res)
        c = cpu.to_host(C.run(case, cpu, enc, b)[0])
        assert (gpu.pbs_count, gpu.launches) == (cpu.pbs_count, cpu.launches) == C.shadow(case)
        _same(g, c)
        assert C.decrypt(ck, g, case.nb) == want[b * C.K:(b + 1) * C.K]
        layers = [e for e in events if isinstance(e, list)]
        outside = [e for e in events if not isinstance(e, list)]
        _check_fused_layers(case, layers)
        assert gpu.launches == outside.count("P") + sum("P" in e for e in layers)
        if case.variant == "dirty":
            continue                                  # full_propagate first: the multiply DAG's launch path, as pinned
        if case.op != "scalar_mul":
            # the shifts and rotations: fused layers alone; outside them at most the one block-layer call of a pure
            # block move.  No copy_block, mul_add, set_trivial, roll or unfused layer.
            assert outside in ([], ["B", "E"]), outside
            assert outside == [] or (not layers and C.shadow(case) == (0, 0))
            if C.shadow(case)[1]:
                assert len(layers) == C.shadow(case)[1] or C._trivial(case)
        else:
            # scalar_mul: the preshifts are ONE fused layer, in front; blockshift keeps its roll and the sum its path
            T, scalar = C.total_bits(case.nb), case.clear
            general = scalar > 1 and scalar & (scalar - 1) != 0
            assert len(layers) <= 1 and (not layers or isinstance(events[0], list))
            if general:
                terms = bin(scalar % 2 ** T).count("1")
                assert outside.count("R") >= terms and (terms < 2 or "M" in outside)
                odd = any((scalar >> i) & 1 for i in range(1, scalar.bit_length(), C.BITS))   # has_at_least_one_set[1]
                assert len(layers) == (1 if odd else 0)
            else:
                assert not set(outside) & set("CMRQ"), outside
    assert all(np.array_equal(e.data, d) for e, d in zip(all_enc, before)), "an input batch was written"


def test_a_barrel_stage_is_one_engine_call(shift_keys, monkeypatch):
    """left_shift over 8 blocks: 16 + 4 extractions, four stages of 16 muxes with three terms each, 8
    recompositions: six fused layers of exactly B E P B E"""
    ck, gpu, cpu = shift_keys
    case = next(c for c in C.CASES if c.id == "left_shift-clean-b8")
    enc = C.encrypt(ck, case)
    lhs, rhs = C.operands(case, gpu, enc, 0)
    log = _watch(monkeypatch, gpu)
    res = gpu.to_host(C.apply(case, gpu, lhs, rhs, 0))
    _same(res, cpu.to_host(C.run(case, cpu, enc, 0)[0]))
    assert log == [["B", "E", "P", "B", "E"]] * 6
    assert (gpu.pbs_count, gpu.launches) == (276, 6)


def test_a_pure_block_move_is_one_block_layer_call(shift_keys, monkeypatch):
    ck, gpu, cpu = shift_keys
    case = next(c for c in C.CASES if c.id == "scalar_right_shift-clean-b5-by2")
    enc = C.encrypt(ck, case)
    lhs, rhs = C.operands(case, gpu, enc, 0)
    log = _watch(monkeypatch, gpu)
    res = gpu.to_host(C.apply(case, gpu, lhs, rhs, 0))
    _same(res, cpu.to_host(C.run(case, cpu, enc, 0)[0]))
    assert log == ["B", "E"] and (gpu.pbs_count, gpu.launches) == (0, 0)
    assert res.noise[-1] == 0 and res.degree[-1] == 0 and not res.data[:, -1, :].any()   # the vacated block
