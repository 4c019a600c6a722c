"""tfhe_mi355_lwe_block_layer_async (csrc/lwe_ops.hip lwe_block_layer_kernel): one layer of block arithmetic in
one launch, against the numpy statement of its formula

    dst[r][w] = sum_t scalar_t * src_t[r][w] + (w == words - 1 ? body_add : 0)      (wrapping mod 2^64)

  direct       every word of the destination tensor and of every source tensor, over the shapes at which the
               indexing can go wrong: body-only rows (words = 1), the workgroup edge (255, 256, 257), an odd row
               length above one tile (743) and the 2_2 row (2049); 1 and 3 rows; term counts 0 .. 4; scalars 0, 1,
               2^64 - 1 and random; body_add 0 and random; an op in place; strides above `words`;
  guard bands  a 7-op layer and a 70-op layer (more than one table of kernel arguments holds: two launches at
               least) as cases of tests/test_async_guards_gpu.py's runner, registered with its `case` decorator, so
               the header-completeness check of tests/test_guarded_arena.py sees them and
               tests/test_async_graph_gpu.py replays them from a captured hipGraph;
  refusals     a NULL destination, a stride below the row, rows of zero words; the empty calls.

The guarded cases are registered when this module is imported.  tests/test_async_graph_gpu.py takes its copy of
the case table when it is imported, so this module has to be collected before it: its name sorts before
test_async_graph_gpu.py.
"""
import numpy as np
import pytest

import test_async_guards_gpu as G

pytestmark = pytest.mark.gpu

U64 = np.uint64
ONES = (1 << 64) - 1


def _rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=U64)


def reference(tensors, ops, rows, words):
    """The formula on flat u64 arrays.  tensors: {name: flat array}; an op is
    ((name, offset, stride), body_add, [((name, offset, stride), scalar), ...]), offsets and strides in words.
    Every op reads the tensors as they were before the call: but for an op in place no destination may overlap
    anything else, so the order does not matter.  Returns the tensors after the call."""
    out = {k: v.copy() for k, v in tensors.items()}
    w = np.arange(words)
    for (dn, do, ds), body_add, terms in ops:
        acc = np.zeros((rows, words), dtype=U64)
        for (sn, so, ss), scalar in terms:
            at = so + np.arange(rows)[:, None] * ss + w[None, :]
            acc += U64(scalar % (1 << 64)) * tensors[sn][at]
        acc[:, -1] += U64(body_add % (1 << 64))
        out[dn][do + np.arange(rows)[:, None] * ds + w[None, :]] = acc
    return out


def device_ops(ptr, ops):
    """the ops with device addresses: ptr[name] is the address of word 0 of the tensor"""
    return [(ptr[dn] + 8 * do, ds, body_add, [(ptr[sn] + 8 * so, ss, scalar) for (sn, so, ss), scalar in terms])
            for (dn, do, ds), body_add, terms in ops]


@pytest.fixture(scope="module")
def eng():
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    e = Engine(P.with_(lwe_dimension=4), 0)  # the call takes the caller's `words`, whatever the context's
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(U64)


# ---- the layers -------------------------------------------------------------------------------------------------
def seven_op_layer(words, seed):
    """(shapes, ops): destination tensor `out` [rows][8 blocks][words + 7], sources `a` [rows][4][words] and `b`
    [rows][2][words + 5].  Blocks 0 .. 6 of `out` are written, block 7 and the padding words are not.
      0  no term: trivial ciphertexts            1  negation with a correcting term (scalar 2^64 - 1)
      2  packing m * hi + lo from two tensors     3  three terms, one with scalar 0
      4  the packed comparison input m * a1 + a0 - m * b1 - b0
      5  in place: 3 * own + a2 + random body     6  a copy (scalar 1) out of the strided tensor"""
    r = [int(x) for x in _rand(seed, 8)]
    A, B, O = 4 * words, 2 * (words + 5), 8 * (words + 7)
    a = lambda j: ("a", j * words, A)                 # noqa: E731
    b = lambda j: ("b", j * (words + 5), B)           # noqa: E731
    o = lambda j: ("out", j * (words + 7), O)         # noqa: E731
    ops = [
        (o(0), r[0], []),
        (o(1), 12 << 59, [(a(0), ONES)]),
        (o(2), 0, [(a(1), 4), (b(0), 1)]),
        (o(3), r[1], [(a(3), r[2]), (b(1), 0), (a(0), 1)]),
        (o(4), 0, [(a(1), 4), (a(0), 1), (b(1), ONES - 3), (b(0), ONES)]),
        (o(5), r[3], [(o(5), 3), (a(2), 1)]),
        (o(6), 0, [(b(1), 1)]),
    ]
    return {"a": A, "b": B, "out": O}, ops


def seventy_op_layer(words):
    """70 destination blocks of `out` [rows][70][words] from `a` [rows][5][words]: op i has i % 5 terms (the
    fifth is in place where i % 10 == 9), scalars and body_add following i"""
    A, O = 5 * words, 70 * words
    ops = []
    for i in range(70):
        terms = [(("a", ((i + t) % 5) * words, A), [1, ONES, 4, i * 0x9E3779B97F4A7C15][t]) for t in range(i % 5)]
        if i % 10 == 9:
            terms[3] = (("out", i * words, O), 5)
        ops.append((("out", i * words, O), (i * 0xD1B54A32D192ED03) % (1 << 64) if i % 3 else 0, terms))
    return {"a": A, "out": O}, ops


# ---- direct: every word of every tensor -------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("words", [1, 255, 256, 257, 743, 2049])
def test_block_layer_matches_the_formula(eng, words, rows):
    shapes, ops = seven_op_layer(words, words + rows)
    host = {name: _rand(words * 31 + rows + i, rows * per_row) for i, (name, per_row) in enumerate(shapes.items())}
    want = reference(host, ops, rows, words)
    dev = {name: _dev(v) for name, v in host.items()}
    eng.lwe_block_layer_async(device_ops({n: t.data_ptr() for n, t in dev.items()}, ops), rows, words)
    for name in host:
        got = _host(dev[name])
        bad = np.flatnonzero(got != want[name])
        assert bad.size == 0, f"{name}: {bad.size} words differ, first {bad[0]}, last {bad[-1]}"
    changed = np.flatnonzero(want["out"] != host["out"]).size  # the call is not a no-op on this tensor
    assert changed > 6 * rows * words * 0.9 and np.array_equal(want["a"], host["a"])


def test_block_layer_over_several_launches_and_a_kept_table(eng):
    rows, words = 3, 257
    shapes, ops = seventy_op_layer(words)
    host = {name: _rand(7 + i, rows * per_row) for i, (name, per_row) in enumerate(shapes.items())}
    want = reference(host, ops, rows, words)
    dev = {name: _dev(v) for name, v in host.items()}
    table = eng.block_ops(device_ops({n: t.data_ptr() for n, t in dev.items()}, ops))
    eng.lwe_block_layer_async(table, rows, words)
    for name in host:
        assert np.array_equal(_host(dev[name]), want[name]), name
    # the same table again: the in-place ops go on from what the first call left
    again = reference(want, ops, rows, words)
    eng.lwe_block_layer_async(table, rows, words)
    assert np.array_equal(_host(dev["out"]), again["out"])


def test_block_layer_refusals_and_empty_calls(eng):
    import torch

    from tfhe_mi355 import EngineError

    words, rows = 9, 2
    y = torch.full((rows * 2 * words,), 7, dtype=torch.int64, device="cuda")
    x = torch.full((rows * words,), 5, dtype=torch.int64, device="cuda")
    yp, xp = y.data_ptr(), x.data_ptr()
    with pytest.raises(EngineError, match="null destination"):
        eng.lwe_block_layer_async([(yp, 2 * words, 0, []), (None, 2 * words, 0, [])], rows, words)
    with pytest.raises(EngineError, match="stride smaller than the row"):
        eng.lwe_block_layer_async([(yp, words - 1, 0, [])], rows, words)
    with pytest.raises(EngineError, match="stride smaller than the row"):
        eng.lwe_block_layer_async([(yp, 2 * words, 0, [(xp, words - 1, 1)])], rows, words)
    with pytest.raises(EngineError, match="zero words"):
        eng.lwe_block_layer_async([(yp, 2 * words, 0, [])], rows, 0)
    with pytest.raises(ValueError, match="at most 4 terms"):
        eng.lwe_block_layer_async([(yp, 2 * words, 0, [(xp, words, 1)] * 5)], rows, words)
    eng.lwe_block_layer_async([], rows, words)
    eng.lwe_block_layer_async([], rows, 0)
    eng.lwe_block_layer_async([(yp, 2 * words, 1, [(xp, words, 1)])], 0, words)
    torch.cuda.synchronize()
    assert (y == 7).all() and (x == 5).all(), "a refused or an empty call wrote"
    # an absent stride on an absent term is not looked at
    eng.lwe_block_layer_async([(yp, 2 * words, 3, [(None, 0, 9), (xp, words, 2)])], rows, words)
    got = _host(y).reshape(rows, 2 * words)
    assert (got[:, :words - 1] == 10).all() and (got[:, words - 1] == 13).all() and (got[:, words:] == 7).all()


# ---- guard bands: the entry point as cases of the guarded runner (and of the graph replay) --------------------------
BLOCKS = "blocks256"
G.FACTORIES[BLOCKS] = lambda orc: G._pbs_engine(orc, 256, 5, 1, 15, 2, 0, False)
_FIRST_CASE = len(G.CASES)


def _layer_case(cid, rows, words, shapes, ops, seed):
    @G.case(cid, BLOCKS, ["lwe_block_layer_async"])
    def build(E, orc):
        eng = E.eng
        host = {name: _rand(seed + i, rows * per_row) for i, (name, per_row) in enumerate(shapes.items())}
        want = reference(host, ops, rows, words)
        regions = [G._rin(name, host[name], row=words * 8) for name in shapes if name != "out"]
        regions.append(G._rout("out", host["out"].nbytes, row=words * 8, data=host["out"]))

        def call(v):
            eng.lwe_block_layer_async(device_ops({n: v[n].data_ptr() for n in shapes}, ops), rows, words)

        return G._spec(regions, call, lambda: want["out"], "out", (None, 0), None, out_row=shapes["out"] * 8)
    return build


_layer_case("lwe_block_layer-7ops-3x743", 3, 743, *seven_op_layer(743, 160), seed=161)
_layer_case("lwe_block_layer-70ops-2x257", 2, 257, *seventy_op_layer(257), seed=171)

BLOCK_CASES = G.CASES[_FIRST_CASE:]
G._LAST_OF_ENGINE[BLOCKS] = BLOCK_CASES[-1].id


@pytest.mark.parametrize("c", BLOCK_CASES, ids=lambda c: c.id)
def test_guarded_block_layer_call(orc, c):
    """the checks of test_async_guards_gpu.test_guarded_call: the numpy formula word for word over the whole
    destination tensor (the words between the blocks among them), no byte changed outside it, the same output
    from other prior contents (the operand in place restored), the resident key unchanged"""
    G.test_guarded_call(orc, c)
