"""The device path of the radix integer layer (integer._DeviceOps, the two block-layer kernels, the trivial PBS, the
batched KS+PBS with a LUT stack and per-row indexes) at every modulus pair the layer accepts, against the same DAG on
the host path with the oracle engine: the case list of integer_sets_cases.py, lwe_dimension = 8, both server keys of
a set from one ClientKey seed.  The other GPU tests of the layer run PARAM_MESSAGE_2_CARRY_2 alone; here the layer
meets delta = 2^57 .. 2^61, rows of 1537 .. 32769 words, LUTs of 2048 .. 65536 words, families of up to 256 LUTs, the
k = 3 classic kernel and every path of the large-N PBS.

Every result must be resident on the GPU, equal the host DAG's words bit for bit, have its degree, noise, pbs_count
and launches, decrypt to the plain-integer answer and leave its inputs unwritten.  A clear operand per row is handed
over as a numpy array and as a device tensor that is rewritten in place between two calls; a refused case raises
before any engine call; a captured hipGraph at 3_3 follows rewritten operands and clear operands; and the PBS kernel
that serves a layer is the one a plain keyswitch_programmable_bootstrap of the same row count runs.

What a per-row scalar_eq costs at 4_4: the family of a packed digit is msg^2 = 256 LUTs of 65536 words, a 128 MiB
stack on the device, uploaded once per key.  It is accepted: the engine takes any lut_count, and the case runs here.
"""
import numpy as np
import pytest

import integer_sets_cases as C
from conftest import OracleEngine

pytestmark = pytest.mark.gpu


def _keys_of(s):
    @pytest.fixture(scope="module", name=f"keys_{s}")
    def keys():
        ck, gpu = C.keys(s, None)
        _, cpu = C.keys(s, OracleEngine(C.params(s), threads=8))
        return ck, gpu, cpu
    return keys


keys_3_3, keys_4_4, keys_2_3 = _keys_of("3_3"), _keys_of("4_4"), _keys_of("2_3")
keys_3_2, keys_4_2, keys_1_1 = _keys_of("3_2"), _keys_of("4_2"), _keys_of("1_1")
assert set(C.SETS) == {"3_3", "4_4", "2_3", "3_2", "4_2", "1_1"}


def _same(g, c):
    assert g.degree == c.degree and g.noise == c.noise
    assert g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"


def _host_run(case, cpu, enc, b):
    res = [cpu.to_host(r) for r in C.run(case, cpu, enc, b)]
    return res, (cpu.pbs_count, cpu.launches)


def _check(case, ck, gpu, res, host, want):
    """the results of one device call against the host run of the same rows"""
    import torch

    host_res, host_counts = host
    assert all(isinstance(r.data, torch.Tensor) and r.data.is_cuda for r in res), "a result is not resident on the GPU"
    assert (gpu.pbs_count, gpu.launches) == host_counts
    got = [gpu.to_host(r) for r in res]
    assert len(got) == len(host_res)
    for g, c in zip(got, host_res):
        _same(g, c)
    assert C.decrypted(ck, case, got) == want


def _device_rows(gpu, clear):
    import torch

    return torch.from_numpy(clear.view(np.int64)).to(gpu.ops.device)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_device_case_equals_host_case(request, case):
    """clear operands in their host forms: a Python int, a numpy array"""
    import torch

    ck, gpu, cpu = request.getfixturevalue(f"keys_{case.set}")
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in C.inputs(enc)]
    want = C.expected(case)
    for b in range(C.ROWS // C.K):
        host = _host_run(case, cpu, enc, b)
        lhs, rhs = C.operands(case, gpu, enc, b)
        kept = [x.data.clone() for x in (lhs, rhs) if x is not None]
        res = C.apply(case, gpu, lhs, rhs if rhs is not None else C.clear_operand(case, b))
        _check(case, ck, gpu, res, host, want[b * C.K:(b + 1) * C.K])
        assert all(torch.equal(x.data, k) for x, k in zip([x for x in (lhs, rhs) if x is not None], kept)), \
            "an operand was written on the device"
    assert all(np.array_equal(e.data, d) for e, d in zip(C.inputs(enc), before)), "an input batch was written"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", [c for c in C.CASES if c.form == "rows"], ids=lambda c: c.id)
def test_a_device_tensor_of_clear_operands_is_followed_in_place(request, monkeypatch, case):
    """the clear operands of batch 0 in a device tensor, then those of batch 1 written into the same tensor: the second
    call follows them, and nothing is uploaded for it (every LUT stack came with the first call)"""
    import torch

    ck, gpu, cpu = request.getfixturevalue(f"keys_{case.set}")
    enc = C.encrypt(ck, case)
    want = C.expected(case)
    handed = _device_rows(gpu, C.clear_operand(case, 0))
    lhs, _ = C.operands(case, gpu, enc, 0)
    _check(case, ck, gpu, C.apply(case, gpu, lhs, handed), _host_run(case, cpu, enc, 0), want[:C.K])
    assert torch.equal(handed, _device_rows(gpu, C.clear_operand(case, 0))), "the clear operands were written"
    handed.copy_(_device_rows(gpu, C.clear_operand(case, 1)))
    lhs, _ = C.operands(case, gpu, enc, 1)
    for name in ("from_host", "index_from_host"):
        monkeypatch.setattr(gpu.ops, name, lambda data, name=name: pytest.fail(f"{name} on the second call"))
    res = C.apply(case, gpu, lhs, handed)
    monkeypatch.undo()
    _check(case, ck, gpu, res, _host_run(case, cpu, enc, 1), want[C.K:])


@pytest.mark.timeout(60)
@pytest.mark.parametrize("case", C.REFUSED, ids=lambda c: c.id)
def test_refused_case_raises_before_any_engine_call(request, monkeypatch, case):
    import torch

    ck, gpu, _ = request.getfixturevalue(f"keys_{case.set}")
    enc = C.encrypt(ck, case)
    lhs, rhs = C.operands(case, gpu, enc, 0)
    right = rhs if rhs is not None else C.clear_operand(case, 0)
    if case.form == "rows":
        right = _device_rows(gpu, right)
    kept = [x.data.clone() for x in (lhs, rhs) if x is not None]
    eng, reached = gpu.ops.eng, []
    tapped = [name for name in dir(eng) if name.endswith("_async")]
    assert {"keyswitch_programmable_bootstrap_async", "lwe_block_layer_async", "lwe_clear_block_layer_async",
            "trivial_pbs_async", "lwe_scalar_mul_add_async"} <= set(tapped)
    for name in tapped:
        monkeypatch.setattr(eng, name, lambda *a, name=name, **k: reached.append(name))
    with pytest.raises(NotImplementedError, match=f"{C.method(case)}: {C.SETS[case.set][0]} .*is not supported: "):
        C.apply(case, gpu, lhs, right)
    monkeypatch.undo()
    assert not reached and gpu.pbs_count == 0 and gpu.launches == 0
    assert all(torch.equal(x.data, k) for x, k in zip([x for x in (lhs, rhs) if x is not None], kept))


# ---- the block layers on wide rows ------------------------------------------------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("words", [8193, 16385, 32769])
def test_block_layers_on_wide_rows_are_the_host_formula(keys_1_1, words):
    """_DeviceOps.block_layer and clear_block_layer on random rows of 33, 65 and 129 tiles (the last one a single
    word) against _HostOps' numpy formula: an op with no term, one in place, one of six terms (a second engine call
    goes on in place), and clear digits of 3, 6 and 8 bits, negated and not, with and without an index array.  The
    layers take the row width from the call, so the key of any set serves; 16385 words is no set's row."""
    from tfhe_mi355.integer import _ClearRows, _HostOps

    _, gpu, _ = keys_1_1
    dev, host = gpu.ops, _HostOps(None)
    rng = np.random.default_rng(words)
    a = rng.integers(0, 1 << 64, (C.K, 6, words), dtype=np.uint64)
    y = rng.integers(0, 1 << 64, (C.K, 6, words), dtype=np.uint64)
    clear = rng.integers(0, 1 << 64, C.K, dtype=np.uint64)
    r = [int(x) for x in rng.integers(0, 1 << 64, 8, dtype=np.uint64)]

    def plain(A, Y):
        return [(Y[:, 0, :], r[0], []),
                (Y[:, 1, :], r[1], [(Y[:, 1, :], 3), (A[:, 0, :], r[2])]),
                (Y[:, 2, :], r[3], [(A[:, k, :], k + 1) for k in range(6)])]

    def with_clear(A, Y, ops, rows):
        index = [ops.index_rows(C.K) for _ in range(2)]
        part = lambda **k: dict(dict(rows=rows, negate=0, shift=0, bits=0, scale=0, index=None, lut_base=0), **k)  # noqa: E731
        return index, [(Y[:, 3, :], r[4], [(A[:, 1, :], 1)], part(bits=3, scale=1 << 57, index=index[0])),
                       (Y[:, 4, :], 0, [(Y[:, 4, :], 1)], part(negate=1, shift=5, bits=6, scale=r[5], index=index[1],
                                                               lut_base=64)),
                       (Y[:, 5, :], r[6], [(A[:, k, :], r[7]) for k in range(5)], part(shift=56, bits=8, scale=-(1 << 55))),
                       (Y[:, 0, :], 0, [(Y[:, 0, :], 1)], part(rows=None))]

    a_d, y_d = dev.from_host(a), dev.from_host(y)
    a0 = a.copy()
    host.block_layer(plain(a, y))
    dev.block_layer(plain(a_d, y_d))
    assert np.array_equal(dev.to_host(y_d), y)
    h_index, h_ops = with_clear(a, y, host, _ClearRows(host=clear))
    d_index, d_ops = with_clear(a_d, y_d, dev, _ClearRows(dev=dev.from_host(clear)))
    host.clear_block_layer(h_ops)
    dev.clear_block_layer(d_ops)
    assert np.array_equal(dev.to_host(y_d), y)
    for h, d in zip(h_index, d_index):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), h)
    assert h_index[0].max() < 8 and 64 <= h_index[1].min() and h_index[1].max() < 128
    assert np.array_equal(dev.to_host(a_d), a0) and np.array_equal(a, a0)


# ---- which PBS kernel serves a layer -------------------------------------------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("s", list(C.SETS))
def test_the_layer_runs_the_pbs_kernel_of_a_plain_ks_pbs(request, s):
    """scalar_bitand with a clear operand per row: one fused layer of K * blocks rows, a family of msg LUTs, the index
    array written on the device.  Its kernels, by the engine's kernel timing, are those of a plain host-pointer
    keyswitch_programmable_bootstrap of as many rows with one LUT."""
    ck, gpu, cpu = request.getfixturevalue(f"keys_{s}")
    case = next(c for c in C.CASES if c.set == s and c.op == "scalar_bitand" and c.form == "rows" and c.variant == "clean")
    enc = C.encrypt(ck, case)
    lhs, _ = C.operands(case, gpu, enc, 0)
    eng = gpu.ops.eng
    eng.kernel_timing(1)
    res = C.apply(case, gpu, lhs, C.clear_operand(case, 0))
    layer = set(eng.kernel_times())
    assert (gpu.pbs_count, gpu.launches) == (C.K * case.nb, 1)
    rows = gpu.to_host(lhs).data.reshape(C.K * case.nb, -1)
    eng.kernel_timing(1)
    out = eng.keyswitch_programmable_bootstrap(rows, gpu.lut_message.acc)
    plain = set(eng.kernel_times())
    eng.kernel_timing(0)
    print(f"\n{C.SETS[s][0]}: {C.K * case.nb} rows, layer {sorted(layer)}, plain KS+PBS {sorted(plain)}")
    assert layer == plain and layer - {"keyswitch"}, (layer, plain)
    _check(case, ck, gpu, res, _host_run(case, cpu, enc, 0), C.expected(case)[:C.K])
    assert np.array_equal(out, cpu.shortint.engine_ks_pbs(rows, cpu.lut_message.acc))


# ---- hipGraph ------------------------------------------------------------------------------------------------------
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


@pytest.mark.timeout(120)
def test_graph_replay_at_3_3_follows_operands_and_clear_operands(keys_3_3, monkeypatch):
    """scalar_lt_parallelized with a device tensor of clear operands, then if_then_else_parallelized on its result,
    3 blocks at 3_3, captured after a warm-up.  The replay equals the host run; with both ciphertext operands and the
    clear operands rewritten in place, the next replay equals the host run on those."""
    import torch

    ck, gpu, cpu = keys_3_3
    pair = next(c for c in C.CASES if c.id == "3_3-max-clean-b3")
    clear = next(c for c in C.CASES if c.id == "3_3-scalar_lt-rows-clean-b3")
    enc = C.encrypt(ck, pair)
    clears = [C.clear_operand(clear, b) for b in range(2)]
    v = C.values(pair)

    def want(b):
        rows = range(b * C.K, (b + 1) * C.K)
        return [v["lhs"][r] if v["lhs"][r] < int(clears[b][r % C.K]) else v["rhs"][r] for r in rows]

    picks = [[v["lhs"][b * C.K + r] < int(clears[b][r]) for r in range(C.K)] for b in range(2)]
    assert picks[0] != picks[1] and all(True in p and False in p for p in picks), "both arms, and not the same rows"

    def host(b):
        x, y = (C.batch_rows(enc[n][0], b) for n in ("lhs", "rhs"))
        return cpu.to_host(cpu.if_then_else_parallelized(cpu.scalar_lt_parallelized(x, clears[b]), x, y))

    x_d, y_d = (gpu.to_device(C.batch_rows(enc[n][0], 0)) for n in ("lhs", "rhs"))
    c_d = _device_rows(gpu, clears[0])

    def dag():
        return gpu.if_then_else_parallelized(gpu.scalar_lt_parallelized(x_d, c_d), x_d, y_d)

    _same(gpu.to_host(dag()), host(0))                  # warm-up: the LUT stacks and the scratch are on the device
    graph, out = _capture(monkeypatch, gpu, dag)
    graph.replay()
    torch.cuda.synchronize()
    first = gpu.to_host(out)
    _same(first, host(0))
    assert [t[0] for t in C.decrypted(ck, pair, (first,))] == want(0)
    c_d.copy_(_device_rows(gpu, clears[1]))             # new clear operands and new ciphertext words, in place
    x_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc["lhs"][0], 1).data))
    y_d.data.copy_(gpu.ops.from_host(C.batch_rows(enc["rhs"][0], 1).data))
    graph.replay()
    torch.cuda.synchronize()
    second = gpu.to_host(out)
    _same(second, host(1))
    assert [t[0] for t in C.decrypted(ck, pair, (second,))] == want(1)
    assert not np.array_equal(first.data, second.data)
    graph = None
