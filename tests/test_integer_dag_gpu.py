"""The device-resident radix integer DAG (integer._DeviceOps: lwe_ops kernels, layer-table caches, hipGraph
replay) against the same DAG on the host path with the oracle engine: PARAM_MESSAGE_2_CARRY_2_KS_PBS at
lwe_dimension = 8, both server keys from one ClientKey seed.  Every result must equal the host DAG's bit
for bit, with the same degree, noise, pbs_count and launches, and decrypt to the integer answer."""
import numpy as np
import pytest

import integer_dag_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dag_keys():
    ck, gpu = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    return ck, gpu, cpu


def _same(g, c):
    """Host batches g (from the device path) and c (host path): same words and metadata."""
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _watch_layers(monkeypatch, sks):
    """Per _PbsLayer.flush of `sks`: (requests, trivial_pbs calls, PBS rows)."""
    from tfhe_mi355.integer import _PbsLayer

    log, triv = [], [0]
    flush, trivial_pbs = _PbsLayer.flush, sks.ops.trivial_pbs

    def counted_trivial(rb, j, lut):
        triv[0] += 1
        return trivial_pbs(rb, j, lut)

    def watched(layer):
        if layer.sk is not sks:
            return flush(layer)
        n, t0, p0 = len(layer.reqs), triv[0], sks.pbs_count
        flush(layer)
        log.append((n, triv[0] - t0, sks.pbs_count - p0))

    monkeypatch.setattr(sks.ops, "trivial_pbs", counted_trivial)
    monkeypatch.setattr(_PbsLayer, "flush", watched)
    return log


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_dag_equals_host_dag(dag_keys, monkeypatch, case):
    import torch

    ck, gpu, cpu = dag_keys
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc]
    log = _watch_layers(monkeypatch, gpu)
    res = C.run(case, gpu, enc)
    if case.inputs and case.kind != "sum":
        assert isinstance(res.data, torch.Tensor) and res.data.is_cuda
    g = gpu.to_host(res)
    c = cpu.to_host(C.run(case, cpu, enc))
    assert (gpu.pbs_count, gpu.launches) == (cpu.pbs_count, cpu.launches) == C.EXPECTED[case.id]
    _same(g, c)
    assert np.array_equal(C.decrypt(ck, case, g), C.expected(case))
    assert all(np.array_equal(e.data, b) for e, b in zip(enc, before))
    # pbs_count counts the rows that went through the PBS, never the trivial ones
    assert gpu.pbs_count == C.K * sum(n - t for n, t, _ in log)
    assert all(p == C.K * (n - t) for n, t, p in log)
    if case.kind in ("trivial_mul", "trivial_sum") and case.nb > 1:
        assert any(t and p for _, t, p in log), "no layer mixed trivial_pbs rows with PBS rows"


def test_boolean_valued_operand_is_refused(dag_keys):
    ck, gpu, _ = dag_keys
    case = C.CASES[0]
    a = gpu.to_device(C.encrypt(ck, case)[0])
    with pytest.raises(NotImplementedError, match="boolean-valued operand"):
        gpu.mul_parallelized(a, gpu.create_trivial_zero(C.K, case.nb))
    with pytest.raises(NotImplementedError, match="boolean-valued operand"):
        gpu.mul_parallelized(gpu.create_trivial_zero(C.K, case.nb), a)


@pytest.mark.parametrize("nb", C.BLOCKS)
def test_host_operands_equal_resident_operands(dag_keys, nb):
    """Host batches handed straight to mul_parallelized (_resident uploads them), one host and one resident,
    and both resident: the same words; to_device / to_host is the identity; the inputs stay as they were."""
    ck, gpu, cpu = dag_keys
    case = next(c for c in C.CASES if c.kind == "mul" and c.nb == nb)
    a, b = C.encrypt(ck, case)
    a0, b0 = a.data.copy(), b.data.copy()
    a_d, b_d = gpu.to_device(a), gpu.to_device(b)
    back = gpu.to_host(a_d)
    assert np.array_equal(back.data, a0) and back.degree == a.degree and back.noise == a.noise
    ref = cpu.mul_parallelized(a, b)
    for lhs, rhs in ((a, b), (a_d, b), (a, b_d), (a_d, b_d)):
        _same(gpu.to_host(gpu.mul_parallelized(lhs, rhs)), ref)
    assert np.array_equal(a.data, a0) and np.array_equal(b.data, b0)
    assert np.array_equal(gpu.to_host(a_d).data, a0) and np.array_equal(gpu.to_host(b_d).data, b0)
    assert isinstance(a.data, np.ndarray) and a.degree == [C.MSG - 1] * nb


def _rows(rb, k):
    from tfhe_mi355.integer import RadixBatch

    return RadixBatch(rb.data[:k].copy(), list(rb.degree), list(rb.noise))


def _lut_layer(sks, rb, f):
    """One PBS layer applying a LUT made for this call alone to every block; block 0 is trivial."""
    from tfhe_mi355.integer import _PbsLayer

    x = sks.to_device(rb.clone())
    sks._set_trivial(x, 0, 2)
    lut = sks.shortint.generate_lookup_table(f)
    layer = _PbsLayer(sks)
    for j in range(x.num_blocks):
        layer.add(x, j, lut)
    layer.flush()
    return sks.to_host(x)


def test_cache_pressure(dag_keys, monkeypatch):
    """Two cache entries, batch sizes 1 and 3 in turn, and a LUT created, used and dropped in every round
    (so its id() is likely to come back): the device path still equals the host path, and neither cache
    grows past its bound."""
    from tfhe_mi355 import integer

    ck, gpu, cpu = dag_keys
    monkeypatch.setattr(integer._DeviceOps, "CACHE_ENTRIES", 2)
    sks = integer.ServerKey(gpu.shortint)
    assert sks.ops._stacks.cap == 2 and sks.ops._lut_dev.cap == 2
    case = next(c for c in C.CASES if c.kind == "dirty_add" and c.nb == 3)
    enc = C.encrypt(ck, case)
    for rnd in range(6):
        k = (1, 3)[rnd % 2]
        part = [_rows(e, k) for e in enc]
        _same(sks.to_host(C.run(case, sks, part)), cpu.to_host(C.run(case, cpu, part)))
        assert (sks.pbs_count, sks.launches) == (cpu.pbs_count, cpu.launches)
        f = lambda x, r=rnd: (x * x + r) % C.MSG     # noqa: E731
        _same(_lut_layer(sks, part[0], f), _lut_layer(cpu, part[0], f))
        assert len(sks.ops._stacks) <= 2 and len(sks.ops._lut_dev) <= 2


def test_graph_replay(dag_keys, monkeypatch):
    """A captured mul_parallelized: the replay equals the eager run, follows operand words written in place,
    and survives the eviction of every unpinned cache entry: the tables it reads stay pinned."""
    import torch

    from tfhe_mi355 import integer

    ck, gpu, cpu = dag_keys
    cap = 8                                            # the 3-block multiply has 6 distinct layer tables
    monkeypatch.setattr(integer._DeviceOps, "CACHE_ENTRIES", cap)
    sks = integer.ServerKey(gpu.shortint)
    case = next(c for c in C.CASES if c.kind == "mul" and c.nb == 3)
    other = C.Case("mul", 3, 977)
    enc, enc2 = C.encrypt(ck, case), C.encrypt(ck, other)
    ref, ref2 = cpu.mul_parallelized(*enc), cpu.mul_parallelized(*enc2)
    assert not np.array_equal(ref.data, ref2.data)
    a_d, b_d = sks.to_device(enc[0]), sks.to_device(enc[1])

    small = [_rows(e, 1) for e in enc]                 # eager work the graph does not share: K = 1 tables
    sks.add_assign_parallelized(sks.to_device(small[0]), sks.to_device(small[1]))
    unshared = set(sks.ops._stacks._d)
    eager = sks.mul_parallelized(a_d, b_d)             # warm-up: every table of the DAG is on the device
    torch.cuda.synchronize()
    _same(sks.to_host(eager), ref)
    tables = set(sks.ops._stacks._d) - unshared
    assert len(tables) == 6 and len(sks.ops._stacks) <= cap
    pbs0, launches0 = sks.pbs_count, sks.launches

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sks.mul_parallelized(a_d, b_d)
    assert (sks.pbs_count - pbs0, sks.launches - launches0) == C.EXPECTED[case.id]
    pinned = set(sks.ops._stacks._pinned)
    assert pinned == tables, "the tables the capture touched are not pinned"
    held = {k: sks.ops._stacks._pinned[k][1].data_ptr() for k in pinned}

    graph.replay()
    torch.cuda.synchronize()
    _same(sks.to_host(out), ref)

    a_d.data.copy_(sks.ops.from_host(enc2[0].data))    # new operand words, in place
    b_d.data.copy_(sks.ops.from_host(enc2[1].data))
    graph.replay()
    torch.cuda.synchronize()
    _same(sks.to_host(out), ref2)
    assert np.array_equal(C.decrypt(ck, other, sks.to_host(out)), C.expected(other))

    for rnd in range(2 * cap):                         # eager work that evicts every unpinned entry
        f = lambda x, r=rnd: (x + r) % C.MSG           # noqa: E731
        _same(_lut_layer(sks, small[0], f), _lut_layer(cpu, small[0], f))
    assert not unshared & set(sks.ops._stacks._d) and len(sks.ops._stacks._d) <= cap
    assert set(sks.ops._stacks._pinned) == pinned
    assert {k: sks.ops._stacks._pinned[k][1].data_ptr() for k in pinned} == held

    a_d.data.copy_(sks.ops.from_host(enc[0].data))
    b_d.data.copy_(sks.ops.from_host(enc[1].data))
    graph.replay()
    torch.cuda.synchronize()
    _same(sks.to_host(out), ref)
    _same(sks.to_host(sks.mul_parallelized(a_d, b_d)), ref)   # eager after the capture: pinned tables still serve
