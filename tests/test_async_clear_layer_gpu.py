"""tfhe_mi355_lwe_clear_block_layer_async (csrc/lwe_ops.hip lwe_clear_block_layer_kernel): the block layer with
one clear digit per row, against the numpy statement of its formula

    c            = d_clear ? (negate ? 0 - d_clear[r] : d_clear[r]) : 0
    digit(r)     = (c >> clear_shift) & (2^clear_bits - 1)
    dst[r][w]    = sum_t scalar_t * src_t[r][w] + (w == words - 1 ? body_add + digit(r) * clear_scale : 0)
    lut_index[r] = lut_base + digit(r)                                               (all wrapping mod 2^64)

  direct       every word of the destination tensor, of the sources, of the clear operands and of the index array
               (the words that must not change among them), over words 1, 9, 256, 257, 513 (body-only rows, the
               workgroup edge, three tiles), rows 1, 3, 70 and 90 (with a full table an op has 2048 / 25 = 81
               workgroups: 70 rows of two or three tiles and 90 rows of one run past them), one op and one more
               than a table holds; clear_shift + clear_bits at 64 and above, clear_bits 0 and 8, negate on and off,
               clear_scale 0, delta and 2^64 - delta, d_clear NULL, d_lut_index NULL, ops in place, strides above
               `words`; a layer without any clear part against the plain call;
  guard bands  a single-launch and a multi-launch layer as cases of tests/test_async_guards_gpu.py's runner (the
               destination tensor and the index array are one written region), so tests/test_guarded_arena.py sees
               the entry point covered and tests/test_async_graph_gpu.py replays it from a captured hipGraph;
  refusals     the plain call's, clear_shift > 63, clear_bits > 8, an index from clear bits without a clear
               operand; the empty calls.

The guarded cases are registered when this module is imported; its name sorts before test_async_graph_gpu.py, which
takes its copy of the case table at import (see tests/test_async_block_layer_gpu.py).
"""
import ctypes

import numpy as np
import pytest

import test_async_block_layer_gpu as BL
import test_async_guards_gpu as G

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32
ONES = (1 << 64) - 1
DELTA = 1 << 59  # 2_2: 2^63 / 16
CLEAR_ROWS = 3   # rows of the clear tensor [CLEAR_ROWS][rows]: an op takes one of them


def ops_per_launch():
    """engine.h CLEAR_BLOCK_LAYER_OPS_PER_LAUNCH: the entries that fit the 4 KiB of kernel arguments beside the
    three u32 row counts"""
    from tfhe_mi355 import _lib

    return (4096 - 12) // ctypes.sizeof(_lib.TfheMi355ClearBlockOp)


# the clear parts, in turn over the ops of a layer.  clear: row of the clear tensor or None (d_clear NULL);
# index: whether the op writes its row of the index array [n_ops][rows]
CLEAR = [
    dict(clear=0, negate=0, shift=0, bits=2, scale=DELTA, index=True, lut_base=0),
    dict(clear=1, negate=1, shift=2, bits=2, scale=DELTA, index=False, lut_base=0),
    dict(clear=2, negate=0, shift=60, bits=4, scale=(1 << 64) - DELTA, index=True, lut_base=5),     # ends at bit 64
    dict(clear=0, negate=1, shift=62, bits=8, scale=DELTA, index=True, lut_base=1),                 # runs past it
    dict(clear=1, negate=0, shift=7, bits=0, scale=DELTA, index=True, lut_base=7),                  # digit 0
    None,                                                                                           # a plain op
    dict(clear=None, negate=0, shift=0, bits=0, scale=DELTA, index=True, lut_base=3),               # a fixed LUT
    dict(clear=2, negate=0, shift=63, bits=8, scale=0, index=True, lut_base=0),                     # index alone
    dict(clear=0, negate=1, shift=5, bits=8, scale=0x9E3779B97F4A7C15, index=True, lut_base=(1 << 32) - 300),
    dict(clear=1, negate=1, shift=9, bits=4, scale=DELTA, index=False, lut_base=0),
    dict(clear=None, negate=1, shift=3, bits=4, scale=DELTA, index=False, lut_base=9),              # NULL: plain
]


def clear_layer(n_ops, words, start=0):
    """(shapes, ops): `out` [rows][n_ops][words + 3] from `a` [rows][3][words + 1]; op i has i % 4 terms out of
    `a`, is in place as well where i % 5 == 4, and carries CLEAR[(start + i) % len(CLEAR)].  An op is BL's
    ((name, offset, stride), body_add, terms) with the clear part appended."""
    A, O = 3 * (words + 1), n_ops * (words + 3)
    ops = []
    for i in range(n_ops):
        terms = [(("a", ((i + t) % 3) * (words + 1), A), [1, ONES, 4][t]) for t in range(i % 4)]
        if i % 5 == 4:
            terms.append((("out", i * (words + 3), O), 3))
        body_add = (i * 0xD1B54A32D192ED03) % (1 << 64) if i % 3 else 0
        ops.append((("out", i * (words + 3), O), body_add, terms, CLEAR[(start + i) % len(CLEAR)]))
    return {"a": A, "out": O}, ops


def host_tensors(shapes, n_ops, rows, seed):
    host = {name: BL._rand(seed + i, rows * per_row) for i, (name, per_row) in enumerate(shapes.items())}
    clear = BL._rand(seed + 11, CLEAR_ROWS * rows)
    clear[:min(3, rows)] = np.array([0, ONES, 1], dtype=U64)[:min(3, rows)]  # 0 and its negation, all ones, one
    host["clear"] = clear
    host["idx"] = np.random.default_rng(seed + 12).integers(0, 1 << 32, n_ops * rows, dtype=U32)
    return host


def reference(tensors, ops, rows, words):
    """the tensors after the call: BL.reference on the plain parts, then the clear parts"""
    out = BL.reference({k: v for k, v in tensors.items() if k != "idx"}, [op[:3] for op in ops], rows, words)
    out["idx"] = tensors["idx"].copy()
    for i, ((dn, do, ds), _, _, c) in enumerate(ops):
        if c is None:
            continue
        digit = np.zeros(rows, dtype=U64)
        if c["clear"] is not None:
            v = tensors["clear"][c["clear"] * rows:(c["clear"] + 1) * rows]
            v = (U64(0) - v) if c["negate"] else v
            digit = (v >> U64(c["shift"])) & U64((1 << c["bits"]) - 1)
        out[dn][do + np.arange(rows) * ds + words - 1] += digit * U64(c["scale"])
        if c["index"]:
            out["idx"][i * rows:(i + 1) * rows] = ((U64(c["lut_base"]) + digit) & U64(0xFFFFFFFF)).astype(U32)
    return out


def device_ops(ptr, ops, rows):
    """the ops with device addresses, as Engine.clear_block_ops takes them"""
    out = []
    for i, (op, c) in enumerate(zip(BL.device_ops(ptr, [op[:3] for op in ops]), (op[3] for op in ops))):
        if c is not None:
            c = dict(d_clear=None if c["clear"] is None else ptr["clear"] + 8 * c["clear"] * rows,
                     d_lut_index=ptr["idx"] + 4 * i * rows if c["index"] else None,
                     negate=c["negate"], shift=c["shift"], bits=c["bits"], scale=c["scale"], lut_base=c["lut_base"])
        out.append(op + (c,))
    return out


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def _host(t, dtype):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def eng():
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    e = Engine(P.with_(lwe_dimension=4), 0)  # the call takes the caller's `words`, whatever the context's
    yield e
    e.close()


def _run(eng, shapes, ops, rows, words, seed, call=None):
    host = host_tensors(shapes, len(ops), rows, seed)
    dev = {name: _dev(v) for name, v in host.items()}
    table = device_ops({n: t.data_ptr() for n, t in dev.items()}, ops, rows)
    (call or eng.lwe_clear_block_layer_async)(table, rows, words)
    return host, {name: _host(dev[name], host[name].dtype) for name in host}


# ---- direct: every word of every tensor -------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops", ["one", "table+1"])
@pytest.mark.parametrize("rows", [1, 3, 70, 90])
@pytest.mark.parametrize("words", [1, 9, 256, 257, 513])
def test_clear_block_layer_matches_the_formula(eng, words, rows, n_ops):
    n = 1 if n_ops == "one" else ops_per_launch() + 1
    assert n == 1 or n > 2 * len(CLEAR)  # the long layer has every clear part at least twice
    shapes, ops = clear_layer(n, words, start=words + rows)
    host, got = _run(eng, shapes, ops, rows, words, words * 31 + rows)
    want = reference(host, ops, rows, words)
    for name in host:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{name}: {bad.size} words differ, first {bad[0]}, last {bad[-1]}"
    assert np.array_equal(want["a"], host["a"]) and np.array_equal(want["clear"], host["clear"])
    if n > 1:  # the call is not a no-op, and the clear parts are not
        plain = BL.reference({k: v for k, v in host.items() if k != "idx"}, [op[:3] for op in ops], rows, words)
        assert np.flatnonzero(want["out"] != host["out"]).size > n * rows * words * 0.9
        assert (want["out"] != plain["out"]).any() and (want["idx"] != host["idx"]).any()
        assert (want["idx"] == host["idx"]).any()  # ops without an index leave their rows of it


def test_one_op_with_every_clear_part(eng):
    """the single-op launch once per clear part (the parametrised test picks one per shape)"""
    rows, words = 3, 9
    for start in range(len(CLEAR)):
        shapes, ops = clear_layer(1, words, start=start)
        host, got = _run(eng, shapes, ops, rows, words, 50 + start)
        want = reference(host, ops, rows, words)
        for name in host:
            assert np.array_equal(got[name], want[name]), (start, name)


def test_without_a_clear_operand_it_is_the_plain_call(eng):
    rows, words = 3, 257
    shapes, plain_ops = BL.seventy_op_layer(words)
    ops = [op + (None,) for op in plain_ops]
    host, got = _run(eng, shapes, ops, rows, words, 7)
    plain = {name: BL._dev(host[name]) for name in shapes}
    eng.lwe_block_layer_async(BL.device_ops({n: t.data_ptr() for n, t in plain.items()}, plain_ops), rows, words)
    want = reference(host, ops, rows, words)
    for name in shapes:
        assert np.array_equal(got[name], BL._host(plain[name])), name
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["idx"], host["idx"]) and np.array_equal(got["clear"], host["clear"])


def test_a_kept_table_serves_new_clear_operands(eng):
    """the table holds addresses only: the same table after the clear tensor changed in place"""
    import torch

    rows, words = 3, 257
    shapes, ops = clear_layer(ops_per_launch() + 1, words)
    ops = [op for op in ops if not any(t[0][0] == "out" for t in op[2])]  # no op in place: the call can repeat
    host = host_tensors(shapes, len(ops), rows, 90)
    dev = {name: _dev(v) for name, v in host.items()}
    table = eng.clear_block_ops(device_ops({n: t.data_ptr() for n, t in dev.items()}, ops, rows))
    eng.lwe_clear_block_layer_async(table, rows, words)
    first = reference(host, ops, rows, words)
    for name in host:
        assert np.array_equal(_host(dev[name], host[name].dtype), first[name]), name
    other = dict(first, clear=BL._rand(91, CLEAR_ROWS * rows))
    dev["clear"].copy_(torch.from_numpy(other["clear"].view(np.uint8)))
    eng.lwe_clear_block_layer_async(table, rows, words)
    second = reference(other, ops, rows, words)
    assert (second["out"] != first["out"]).any() and (second["idx"] != first["idx"]).any()
    for name in host:
        assert np.array_equal(_host(dev[name], host[name].dtype), second[name]), name


def test_clear_block_layer_refusals_and_empty_calls(eng):
    import torch

    from tfhe_mi355 import EngineError

    words, rows = 9, 2
    y = torch.full((rows * 2 * words,), 7, dtype=torch.int64, device="cuda")
    x = torch.full((rows * words,), 5, dtype=torch.int64, device="cuda")
    c = torch.full((rows,), 6, dtype=torch.int64, device="cuda")
    idx = torch.full((rows,), 8, dtype=torch.int32, device="cuda")
    yp, xp, cp, ip = y.data_ptr(), x.data_ptr(), c.data_ptr(), idx.data_ptr()
    call = eng.lwe_clear_block_layer_async
    full = dict(d_clear=cp, d_lut_index=ip, bits=2, scale=1)
    with pytest.raises(EngineError, match="null destination"):
        call([(yp, 2 * words, 0, [], full), (None, 2 * words, 0, [], None)], rows, words)
    with pytest.raises(EngineError, match="stride smaller than the row"):
        call([(yp, words - 1, 0, [], full)], rows, words)
    with pytest.raises(EngineError, match="stride smaller than the row"):
        call([(yp, 2 * words, 0, [(xp, words - 1, 1)], full)], rows, words)
    with pytest.raises(EngineError, match="zero words"):
        call([(yp, 2 * words, 0, [], full)], rows, 0)
    with pytest.raises(EngineError, match="clear_shift"):
        call([(yp, 2 * words, 0, [], None), (yp, 2 * words, 0, [], dict(full, shift=64))], rows, words)
    with pytest.raises(EngineError, match="clear_bits"):
        call([(yp, 2 * words, 0, [], dict(full, bits=9))], rows, words)
    with pytest.raises(EngineError, match="no clear operand"):
        call([(yp, 2 * words, 0, [], dict(d_lut_index=ip, bits=1))], rows, words)
    with pytest.raises(ValueError, match="at most 4 terms"):
        call([(yp, 2 * words, 0, [(xp, words, 1)] * 5, full)], rows, words)
    with pytest.raises(ValueError, match="unknown fields"):
        call([(yp, 2 * words, 0, [], dict(full, clear_bits=2))], rows, words)
    call([], rows, words)
    call([], rows, 0)
    call([(yp, 2 * words, 1, [(xp, words, 1)], full)], 0, words)
    torch.cuda.synchronize()
    assert (y == 7).all() and (x == 5).all() and (c == 6).all() and (idx == 8).all(), "a refused or an empty call wrote"
    # the limits themselves are served: shift 63, 8 bits; clear bits without an operand or an index are a plain op
    call([(yp, 2 * words, 3, [(None, 0, 9), (xp, words, 2)], dict(full, shift=1, bits=8, scale=100, lut_base=40)),
          (yp + 8 * words, 2 * words, 0, [], dict(bits=8, shift=63, scale=5))], rows, words)
    got = BL._host(y).reshape(rows, 2 * words)
    assert (got[:, :words - 1] == 10).all() and (got[:, words - 1] == 13 + 300).all() and (got[:, words:] == 0).all()
    assert (idx == 43).all() and (c == 6).all()


# ---- guard bands: the entry point as cases of the guarded runner (and of the graph replay) --------------------------
BLOCKS = "clearblocks256"
G.FACTORIES[BLOCKS] = lambda orc: G._pbs_engine(orc, 256, 5, 1, 15, 2, 0, False)
_FIRST_CASE = len(G.CASES)


def _layer_case(cid, rows, words, n_ops, seed):
    shapes, ops = clear_layer(n_ops, words)

    def written(t):
        """the destination tensor and, behind it, the index array (and zeros up to a whole u64): one written region"""
        idx = t["idx"].view(np.uint8)
        return np.concatenate([t["out"].view(np.uint8), idx, np.zeros(-idx.size % 8, dtype=np.uint8)])

    @G.case(cid, BLOCKS, ["lwe_clear_block_layer_async"])
    def build(E, orc):
        eng = E.eng
        host = host_tensors(shapes, n_ops, rows, seed)
        want = reference(host, ops, rows, words)
        regions = [G._rin("a", host["a"], row=words * 8), G._rin("clear", host["clear"], row=rows * 8),
                   G._rout("out", written(host).nbytes, row=words * 8, data=written(host))]

        def call(v):
            ptr = {n: v[n].data_ptr() for n in ("a", "clear", "out")}
            ptr["idx"] = ptr["out"] + host["out"].nbytes
            eng.lwe_clear_block_layer_async(device_ops(ptr, ops, rows), rows, words)

        return G._spec(regions, call, lambda: written(want), "out", (None, 0), None, out_row=shapes["out"] * 8)
    return build


_layer_case("lwe_clear_block_layer-11ops-3x743", 3, 743, len(CLEAR), seed=261)
_layer_case("lwe_clear_block_layer-60ops-2x257", 2, 257, 60, seed=271)

CLEAR_CASES = G.CASES[_FIRST_CASE:]
G._LAST_OF_ENGINE[BLOCKS] = CLEAR_CASES[-1].id


def test_the_guarded_layers_take_one_and_several_launches():
    assert len(CLEAR) <= ops_per_launch() < 60 and ops_per_launch() == 25


@pytest.mark.parametrize("c", CLEAR_CASES, ids=lambda c: c.id)
def test_guarded_clear_block_layer_call(orc, c):
    """the checks of test_async_guards_gpu.test_guarded_call: the numpy formula word for word over the whole
    destination tensor and the index array (the words between the blocks and the rows of ops without an index
    among them), no byte changed outside them, the same output from other prior contents (the operands in place
    restored), the resident key unchanged"""
    G.test_guarded_call(orc, c)
