"""The wrap-around trip of every capped grid and persistent loop, bit-exact (np.array_equal) throughout.

Three kernel families cap their grid and walk the rest of the work in a loop whose second trip the other files
never reach, their batches being far smaller than the grid:

  classic u64 PBS  pbs_classic.hip, the PbsConfig::PERSIST shapes: a resident grid whose slots take further
                   ciphertexts from a global ticket (`ct_raw = gridDim.x * CPW + ticket`, the LDS hand-over of the
                   ticket among the k + 1 waves of a slot, nothing re-initialised between two ciphertexts);
  block layer      lwe_ops.hip lwe_block_layer_kernel: min(tiles, BLOCK_LAYER_MAX_WORKGROUPS / n_ops) workgroups
                   per op, tiles handed out with `t += gridDim.x`;
  AES and ingress  csprng.hip csprng_mask_kernel (`i += gridDim.x * 256`), lwe_ingress.hip
                   lwe_compact_expand_kernel and csprng_rows_kernel (`r += gridDim.x`).

TFHE_MI355_GRID_CAP=<n> (csrc/engine.h grid_cap(), read at every launch) caps the first and the third family's
grids, so that a handful of rows wraps them; Engine.pbs_resident() reports the PBS kernel's real grid, which the
tests without the hook overrun by one ciphertext and by one workgroup more.  The block layer needs no hook:
tensors of a few megabytes wrap it.

  a  the PERSIST list of the source, pinned               (no GPU)
  b  ticket trips under the hook: every PERSIST shape, both parities of the CMUX count, one workgroup running its
     whole share back to back (cap 1) and two racing for tickets (cap 2); PBS, blind rotation, KS -> PBS
  c  a ticketed launch replayed from a captured graph: the ticket word is reset by the replay itself
  d  the real grid, no hook: resident * CPW + 1 ciphertexts and one full workgroup more
  e  the block layer, direct: every word of every tensor; the grid constants pinned to engine.h (no GPU)
  f  the block layer under the integer DAG: 16 blocks at K = 17 (and 29, where the comparison's 8-op calls wrap)
     against the same DAG on the oracle engine
  g  the AES mask stream, the seeded key upload, the compact expansion, seeded rows and lists, one composed call,
     under the hook

The PBS cases keep n <= 5 (a kernel does not depend on n beyond its CMUX count) and carry the suite's timeout
mark: a deadlock in the ticket hand-over ends the test instead of the run.
"""
import os
import re
from contextlib import contextmanager
from types import SimpleNamespace as NS

import numpy as np
import pytest

import lwe_ingress_reference as R
import test_async_block_layer_gpu as BL
import test_lwe_ingress_gpu as ING
import test_pbs_shapes_gpu as PS
from conftest import KeySet, OracleEngine

gpu = pytest.mark.gpu

U64 = np.uint64
ONES = U64((1 << 64) - 1)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tfhe-rs-odd_amd", "csrc")

# PbsConfig::PERSIST (csrc/pbs_classic.hip): the shapes whose grid is persistent, with their ciphertexts per
# workgroup (PbsConfig::CPW: 4 at the packed 2_2 shape, else 1)
PERSIST_SHAPES = [(2048, 1, 1), (1024, 1, 2), (256, 5, 1), (1024, 2, 3)]
CPW = {s: 4 if s == (2048, 1, 1) else 1 for s in PERSIST_SHAPES}
_shape_id = lambda s: "N%d_k%d_L%d" % s  # noqa: E731

# csrc/engine.h
BLOCK_LAYER_OPS_PER_LAUNCH = 32
BLOCK_LAYER_MAX_WORKGROUPS = 2048


@contextmanager
def _env(**kv):
    """the library reads TFHE_MI355_GRID_CAP at every launch."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _cap(n):
    return _env(TFHE_MI355_GRID_CAP=str(n))


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(U64)


@pytest.fixture(scope="module")
def eng():
    """a context without keys: the block layer takes the caller's `words`, the expansions the caller's n"""
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    e = Engine(P.with_(lwe_dimension=4), 0)
    yield e
    e.close()


# ---- a. the PERSIST list ------------------------------------------------------------------------------------------
def test_persist_shape_list_is_the_source():
    """the four shapes above are the whole PERSIST expression of PbsConfig, clause for clause: a fifth persistent
    shape (or a clause of another form) fails here, and is then owed its cases below"""
    expr = re.search(r"static constexpr bool PERSIST =(.*?);", _source("pbs_classic.hip"), flags=re.S).group(1)
    clause = r"\(N == (\d+) && K == (\d+) && L == (\d+)\)"
    shapes = [tuple(map(int, m)) for m in re.findall(clause, expr)]
    assert re.sub(clause, "", expr).replace("||", "").strip() == "", expr
    assert len(shapes) == 4 and shapes == PERSIST_SHAPES
    assert set(shapes) <= set(PS.CLASSIC_SHAPES)
    cpw = re.search(r"static constexpr int CPW = PACK4 \? (\d+) : (\d+);", _source("pbs_classic.hip"))
    pack4 = re.search(r"static constexpr bool PACK4 = N == (\d+) && K == (\d+) && L == (\d+);", _source("pbs_classic.hip"))
    assert tuple(map(int, pack4.groups())) == (2048, 1, 1) and tuple(map(int, cpw.groups())) == (4, 1)


def test_block_layer_grid_constants_are_the_source():
    text = _source("engine.h")
    assert int(re.search(r"constexpr int BLOCK_LAYER_OPS_PER_LAUNCH = (\d+);", text).group(1)) == BLOCK_LAYER_OPS_PER_LAUNCH
    assert int(re.search(r"constexpr size_t BLOCK_LAYER_MAX_WORKGROUPS = (\d+);", text).group(1)) == \
        BLOCK_LAYER_MAX_WORKGROUPS
    # the launcher's grid, as _workgroups_per_op below restates it
    assert re.search(r"per_op = std::max\(\(size_t\)1, BLOCK_LAYER_MAX_WORKGROUPS / n\);", _source("lwe_ops.hip"))
    assert re.search(r"std::min\(tiles, per_op\)", _source("lwe_ops.hip"))


# ---- b. ticket trips under the hook -------------------------------------------------------------------------------
def _rows(shape):
    """19 rows; (2048, 1, 1): 3 CUs + 5, the first count past the latency kernel's (capi_pbs.cpp latency_max:
    TFHE_MI355_LATENCY_MAX is read once per process, so the row count selects the kernel)"""
    return 3 * PS._cus() + 5 if shape == (2048, 1, 1) else 19


def _inputs(rng, count, n, glwe_len):
    """row 0: every a~ = 0; row 1: b~ = 2N; the rest random words; two random LUTs taken in turn"""
    cts = rng.integers(0, 2 ** 64, (count, n + 1), dtype=U64)
    cts[0, :-1] = 0
    cts[1, -1] = ONES
    luts = rng.integers(0, 2 ** 64, (2, glwe_len), dtype=U64)
    idx = (np.arange(count) % 2).astype(np.uint32)
    return cts, luts, idx


@pytest.fixture(scope="module")
def pbs_cases(orc):
    """{(shape, n): engine under oracle keys at the wide base 30 // L, inputs, the oracle's outputs}: computed
    once, shared by the caps, never written"""
    made = {}

    def get(shape, n):
        if (shape, n) not in made:
            N, k, L = shape
            p = PS._params(N, k, L, 30 // L, n)
            keys = KeySet(orc, p, seed=17 + n)
            eng = PS._engine(p, keys.bsk)
            eng.upload_keyswitch_key(keys.ksk)
            count = _rows(shape)
            cts, luts, idx = _inputs(np.random.default_rng(1000 * N + 10 * k + L + n), count, n, (k + 1) * N)
            made[shape, n] = NS(p=p, keys=keys, eng=eng, count=count, cts=cts, luts=luts, idx=idx,
                                pbs=keys.fbsk.pbs(cts, luts, idx, threads=8),
                                rot=keys.fbsk.blind_rotate(cts, luts, idx, threads=8))
        return made[shape, n]

    yield get
    for c in made.values():
        c.eng.close()


def _classic_alone(ran):
    assert "pbs_classic_kernel" in ran and "pbs_latency_kernel" not in ran, ran


@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("shape", PERSIST_SHAPES, ids=_shape_id)
def test_ticket_trips_under_the_cap(pbs_cases, shape, n, cap):
    """cap 1: one workgroup takes every further ciphertext, its slots each their share back to back; cap 2: two
    workgroups race for the tickets.  n = 4 and 5: a flag phase left over by a ciphertext would depend on the
    parity of the CMUX count."""
    c = pbs_cases(shape, n)
    assert cap * CPW[shape] < c.count, "the grid covers the batch: no ticket is taken"
    assert c.count > cap * (CPW[shape] - 1), "the launcher spreads this batch: no ticket is taken"
    with _cap(cap):
        got, ran = PS._ran(c.eng, lambda: c.eng.programmable_bootstrap(c.cts, c.luts, c.idx))
        _classic_alone(ran)
        PS._same(got, c.pbs, "pbs")
        got, ran = PS._ran(c.eng, lambda: c.eng.blind_rotate(c.cts, c.luts, c.idx))
        _classic_alone(ran)
        PS._same(got, c.rot, "blind rotation")
    PS._same(c.eng.programmable_bootstrap(c.cts, c.luts, c.idx), c.pbs, "pbs, uncapped afterwards")


@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("shape", PERSIST_SHAPES, ids=_shape_id)
def test_keyswitch_then_ticket_trips_under_the_cap(orc, pbs_cases, shape):
    """KS -> PBS in one call: the ticket word then sits in the fused call's scratch, behind the intermediate rows"""
    c = pbs_cases(shape, 4)
    p, cap = c.p, 2
    big = p.glwe_dimension * p.polynomial_size
    rng = np.random.default_rng(big + p.pbs_level)
    cts = rng.integers(0, 2 ** 64, (c.count, big + 1), dtype=U64)
    cts[0, :-1] = 0
    cts[1, -1] = ONES
    small = orc.keyswitch(c.keys.ksk, big, p.lwe_dimension, p.ks_base_log, p.ks_level, cts)
    exp = c.keys.fbsk.pbs(small, c.luts, c.idx, threads=8)
    assert cap * CPW[shape] < c.count
    with _cap(cap):
        got, ran = PS._ran(c.eng, lambda: c.eng.keyswitch_programmable_bootstrap(cts, c.luts, c.idx))
    _classic_alone(ran)
    PS._same(got, exp, "ks -> pbs")


# ---- c. a ticketed launch from a captured graph --------------------------------------------------------------------
@gpu
@pytest.mark.timeout(60)
def test_ticketed_launch_replays_from_a_graph(pbs_cases):
    """(1024, 1, 2), 19 rows over two workgroups: 17 tickets per launch.  Captured once; two replays, then the
    inputs rewritten in place and a third: each equals the oracle, so each replay found its ticket word at 0 --
    reset by the replay itself, the scratch being left as the launch before left it."""
    import torch

    shape = (1024, 1, 2)
    c = pbs_cases(shape, 4)
    N, k, _ = shape
    eng, count = c.eng, c.count
    other = _inputs(np.random.default_rng(77), count, 4, (k + 1) * N)[0]
    exp_other = c.keys.fbsk.pbs(other, c.luts, c.idx, threads=8)
    assert not np.array_equal(exp_other, c.pbs)
    need = eng.pbs_scratch_bytes(count)
    assert need >= 4, "the persistent grid takes its ticket word from the scratch"
    d_in, d_luts, d_idx = _dev(c.cts), _dev(c.luts), _dev(c.idx)
    d_out = torch.zeros((count, k * N + 1), dtype=torch.int64, device="cuda")
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")

    def call():
        eng.programmable_bootstrap_async(d_in, d_out, d_luts, 2, count, d_lut_indexes=d_idx, d_scratch=scratch)

    with _cap(2):
        assert 2 * CPW[shape] < count
        eng.kernel_timing(1)
        call()  # eager, outside the capture
        PS._same(_host(d_out), c.pbs, "eager")
        ran = set(eng.kernel_times())
        eng.kernel_timing(0)
        _classic_alone(ran)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
    for what, rows, exp in (("replay 1", None, c.pbs), ("replay 2", None, c.pbs), ("replay 3", other, exp_other)):
        if rows is not None:
            d_in.copy_(_dev(rows))
        d_out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        PS._same(_host(d_out), exp, what)
    graph = None


# ---- d. the real grid, no hook ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("shape", PERSIST_SHAPES, ids=_shape_id)
def test_one_past_the_resident_grid(orc, shape):
    """resident * CPW + 1 ciphertexts: one slot of the real grid takes one ticket; one full workgroup more: every
    slot of a workgroup's worth does.  One launch each (the _async form; the host-pointer form cuts its batches
    into chunks)."""
    import torch

    N, k, L = shape
    n = 4
    p = PS._params(N, k, L, 30 // L, n)
    keys = KeySet(orc, p, seed=23)
    eng = PS._engine(p, keys.bsk)
    try:
        resident = eng.pbs_resident()
        assert 256 <= resident <= 8192, resident
        counts = [resident * CPW[shape] + 1, (resident + 1) * CPW[shape] + 1]
        cts, luts, idx = _inputs(np.random.default_rng(N + k + L), counts[1], n, (k + 1) * N)
        exp = keys.fbsk.pbs(cts, luts, idx, threads=16)
        d_in, d_luts, d_idx = _dev(cts), _dev(luts), _dev(idx)
        for count in counts:
            d_out = torch.zeros((count, k * N + 1), dtype=torch.int64, device="cuda")
            scratch = torch.full((eng.pbs_scratch_bytes(count),), 0xA5, dtype=torch.uint8, device="cuda")
            eng.kernel_timing(1)
            eng.programmable_bootstrap_async(d_in, d_out, d_luts, 2, count, d_lut_indexes=d_idx, d_scratch=scratch)
            got = _host(d_out)
            ran = set(eng.kernel_times())
            eng.kernel_timing(0)
            _classic_alone(ran)
            PS._same(got, exp[:count], f"{count} ciphertexts over {resident} workgroups")
    finally:
        eng.close()


@gpu
def test_resident_query_answers_for_the_classic_shapes_only(orc):
    """0 for a classic shape without a persistent grid; refused at N >= 4096, for multi-bit, on a context of
    another torus width"""
    from tfhe_mi355 import Engine, EngineError
    from tfhe_mi355 import boolean as Bm

    e = Engine(PS._params(512, 2, 2, 15, 4), 0)
    assert e.pbs_resident() == 0
    e.close()
    for p in (PS._params(4096, 1, 2, 2, 4), PS._params(2048, 1, 1, 30, 4, 2)):
        e = Engine(p, 0)
        with pytest.raises(EngineError, match="no classic 64-bit-torus PBS kernel"):
            e.pbs_resident()
        e.close()
    e = Engine.for_u128(PS._params(1024, 1, 2, 15, 4), 0)
    with pytest.raises(EngineError, match="128-bit torus"):
        e.pbs_resident()
    e.close()
    p32 = Bm.DEFAULT_PARAMETERS
    e = Engine(p32, 0)
    k, N = p32.glwe_dimension, p32.polynomial_size
    e.upload_keyswitch_key_u32(np.zeros(k * N * p32.ks_level * (p32.lwe_dimension + 1), dtype=np.uint32))
    with pytest.raises(EngineError, match="32-bit-torus keys"):
        e.pbs_resident()
    e.close()


# ---- e. the block layer, direct --------------------------------------------------------------------------------------
def _layer(n_ops, words):
    """(shapes, ops) of n_ops ops out of the layers of test_async_block_layer_gpu.py: term counts 0 .. 4, an op in
    place, strides above `words`.  Up to 7 ops: of the seven-op layer (its tensors are the smaller ones)."""
    if n_ops > 7:
        shapes, ops = BL.seventy_op_layer(words)
        ops = ops[:n_ops]               # op i has i % 5 terms, in place where i % 10 == 9
    else:
        shapes, ops = BL.seven_op_layer(words, words + n_ops)
        ops = [ops[i] for i in {1: [4], 5: [0, 1, 3, 4, 5]}[n_ops]]   # 4 terms; 0, 1, 3, 4 terms and 2 in place
    return shapes, ops


def _workgroups_per_op(n_ops):
    """of each launch of a layer of n_ops ops, before the min with the tiles (lwe_ops.hip launch_lwe_block_layer)"""
    out = []
    for first in range(0, n_ops, BLOCK_LAYER_OPS_PER_LAUNCH):
        out.append(max(1, BLOCK_LAYER_MAX_WORKGROUPS // min(n_ops - first, BLOCK_LAYER_OPS_PER_LAUNCH)))
    return out


@gpu
@pytest.mark.parametrize("n_ops,rows,words,tiles,per_op", [
    (32, 9, 2049, 81, [64]),          # every workgroup a second trip at most, the last tile of each row ragged
    (32, 23, 743, 69, [64]),          # three tiles per row: r = t / 3
    (5, 47, 2049, 423, [409]),        # a partial last trip: 14 workgroups go twice
    (1, 257, 2049, 2313, [2048]),     # one op takes the whole cap
    (33, 9, 2049, 81, [64, 2048]),    # two launches, the first wrapping
], ids=lambda v: str(v) if isinstance(v, int) else "")
def test_block_layer_wraps_its_grid(eng, n_ops, rows, words, tiles, per_op):
    assert rows * -(-words // 256) == tiles and _workgroups_per_op(n_ops) == per_op
    assert tiles > per_op[0], "the grid covers the tiles: a retuned constant has un-wrapped this case"
    shapes, ops = _layer(n_ops, words)
    assert len(ops) == n_ops and {len(t) for _, _, t in ops} >= ({0, 1, 2, 3, 4} if n_ops > 1 else {4})
    host = {name: BL._rand(words * 31 + rows + i, rows * per_row) for i, (name, per_row) in enumerate(shapes.items())}
    want = BL.reference(host, ops, rows, words)
    dev = {name: BL._dev(v) for name, v in host.items()}
    eng.lwe_block_layer_async(BL.device_ops({n: t.data_ptr() for n, t in dev.items()}, ops), rows, words)
    for name in host:
        got = BL._host(dev[name])
        bad = np.flatnonzero(got != want[name])
        assert bad.size == 0, f"{name}: {bad.size} words differ, first {bad[0]}, last {bad[-1]}"
    assert np.flatnonzero(want["out"] != host["out"]).size > n_ops * rows * words * 0.9  # the call is no no-op


# ---- f. the block layer under the integer DAG ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dag_keys():
    """(ClientKey, device ServerKey, oracle-engine ServerKey) of one seed, on the integer_ops_cases.py conventions"""
    import integer_ops_cases as C

    ck, dev = C.keys(None)
    _, cpu = C.keys(OracleEngine(C.params(), threads=8))
    yield ck, dev, cpu
    dev.shortint.engine.close()


@gpu
@pytest.mark.parametrize("op,K,wraps", [("bitand", 17, True), ("lt", 17, False), ("lt", 29, True)])
def test_integer_dag_wraps_the_block_layer(dag_keys, monkeypatch, op, K, wraps):
    """16 blocks on 2_2 at lwe_dimension = 8.  bitand at K = 17: its two layer calls have 16 ops of 17 rows of
    2049 words, 153 tiles per op against 128 workgroups.  lt packs the blocks two by two before its first PBS, so
    its widest calls have 8 ops and 256 workgroups per op: K = 17 does not wrap them (the case stays: the
    comparison DAG on 16 blocks), K = 29 does (261 tiles).  The device key against the same DAG on the oracle
    engine: data, degree, noise, pbs_count equal; the result decrypts to the numpy answer."""
    import integer_ops_cases as C
    from tfhe_mi355 import integer

    nb = 16
    ck, dev, cpu = dag_keys
    ck._enc_counter = (9000 + K) << 8
    cks = integer.ClientKey(ck, nb)
    rng = np.random.default_rng(9000 + K)
    a, b = (rng.integers(0, C.MSG ** nb, K, dtype=U64) for _ in range(2))
    b[0] = a[0]                                    # equal
    b[1] = a[1] ^ U64(1)                           # differ only in block 0
    b[2] = a[2] ^ U64(1 << (2 * nb - 1))           # differ only in the top block
    a[3], b[3] = C.MSG ** nb - 1, 0
    ea, eb = cks.encrypt(a), cks.encrypt(b)
    calls = []
    real = dev.ops.eng.lwe_block_layer_async

    def tapped(ops, rows, words, *args, **kw):
        calls.append((ops[1] if isinstance(ops, tuple) else len(ops), rows, words))
        return real(ops, rows, words, *args, **kw)
    monkeypatch.setattr(dev.ops.eng, "lwe_block_layer_async", tapped)

    out = {}
    for sk in (dev, cpu):
        sk.pbs_count = sk.launches = 0
        res = getattr(sk, f"{op}_parallelized")(sk.to_device(ea), sk.to_device(eb))
        out[sk] = (sk.to_host(res), sk.pbs_count, sk.launches)
    (g, g_pbs, g_launches), (c, c_pbs, c_launches) = out[dev], out[cpu]
    assert (g_pbs, g_launches) == (c_pbs, c_launches) and g_pbs > 0
    assert g.degree == c.degree and g.noise == c.noise and g.data.shape == c.data.shape
    assert np.array_equal(g.data, c.data), f"{np.count_nonzero(g.data != c.data)} words differ"
    want = (a & b) if op == "bitand" else (a < b).astype(U64)
    assert np.array_equal(integer.ClientKey(ck, nb if op == "bitand" else 1).decrypt(g), want)
    wrapped = [(n, rows, words) for n, rows, words in calls
               if rows * -(-words // 256) > _workgroups_per_op(n)[0]]
    assert bool(wrapped) == wraps, f"layer calls (ops, rows, words) {calls}, of which wrap their grid: {wrapped}"


# ---- g. the AES stream and the ingress rows under the hook ---------------------------------------------------------
SEEDS = (0, 0x0123456789ABCDEF_FEDCBA9876543210, (1 << 128) - 1)   # of tests/test_csprng_gpu.py
# seven different seeds: a workgroup that takes several rows expands as many key schedules in a row
ROW_SEEDS = list(SEEDS) + [(i * 0x9E3779B97F4A7C15F39CC0605CEDC835) % (1 << 128) for i in range(4, 8)]


@gpu
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("words", [1001, 100003])
def test_mask_stream_under_the_cap(orc, eng, words, cap):
    """502 and 50003 counters over 1 and 3 workgroups of 256: 2 to 196 trips.  (1001 words under cap 3 need two
    workgroups only: the cap above the grid, one trip each.)"""
    assert ((words + 1) // 2 + 1 > cap * 256) == ((words, cap) != (1001, 3))
    for seed in SEEDS:
        with _cap(cap):
            got = eng.csprng_mask_words(seed, words)
        assert np.array_equal(got, orc.seeded_mask_words(seed, 0, words)), hex(seed)


@gpu
@pytest.mark.parametrize("name", ["PARAM_MESSAGE_2_CARRY_2_KS_PBS", "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS"])
def test_seeded_bsk_upload_under_the_cap(orc, name):
    """the seeded upload of test_csprng_gpu.test_seeded_bsk_upload_equals_decompressed_key with the whole mask
    stream of the key on one workgroup: the Fourier key equals the standard upload's"""
    from test_csprng_gpu import _device_to_host
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import ALL

    P = ALL[name].with_(lwe_dimension=6)
    g = P.grouping_factor
    n_ggsw = (P.lwe_dimension // g) << g if g else P.lwe_dimension
    k, N = P.glwe_dimension, P.polynomial_size
    bodies = np.random.default_rng(2).integers(0, 2 ** 64, n_ggsw * P.pbs_level * (k + 1) * N, dtype=U64)
    assert bodies.size * k > 2 * 256, "one workgroup covers the stream"
    seed = 0x0FED_CBA9_8765_4321_1234_5678_9ABC_DEF0
    std = orc.decompress_seeded_bsk(seed, bodies, n_ggsw, P.pbs_level, k, N)
    a, b = Engine(P, 0), Engine(P, 0)
    try:
        a.upload_bootstrap_key(std)
        with _cap(1):
            b.upload_seeded_bootstrap_key(bodies, seed)
        fa, fb = _device_to_host(*a.fourier_bootstrap_key()), _device_to_host(*b.fourier_bootstrap_key())
        assert np.array_equal(fa, fb)
    finally:
        a.close()
        b.close()


@gpu
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("offset", [16, 24])
@pytest.mark.parametrize("n", [8, 256])
def test_compact_expansion_under_the_cap(eng, n, offset, cap):
    """2 n + 3 rows (three bins, the last of three rows) over 1 and 3 workgroups, the output base at 0 and at 8
    modulo 16: a workgroup meets rows of both parities in turn"""
    import torch

    from tfhe_mi355 import LweSource

    count = 2 * n + 3
    assert count > cap
    box = ING._rand(n + offset + cap, R.compact_words(n, count))
    want = R.expand_compact(box, n, count)
    with _cap(cap):
        assert np.array_equal(eng.lwe_expand(LweSource("compact", n, box, count=count)), want)
        d_box = _dev(box)
        buf = torch.full((count * (n + 1) + 8,), -1, dtype=torch.int64, device="cuda")
        assert buf.data_ptr() % 256 == 0
        eng.lwe_expand_async(LweSource("compact", n, d_box, count=count), buf.data_ptr() + offset)
        got = _host(buf)
    w = offset // 8
    assert np.array_equal(got[w:w + count * (n + 1)].reshape(count, n + 1), want)
    assert (got[:w] == ONES).all() and (got[w + count * (n + 1):] == ONES).all()


@gpu
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [742, 7])
def test_seeded_rows_under_the_cap(orc, eng, n, cap):
    """7 rows of 7 seeds on 1 and 3 workgroups: the key schedule in LDS is rewritten per row behind the barrier at
    the loop's tail (n = 742: two AES passes per row, so both hand-over buffers are reused as well)"""
    from tfhe_mi355 import LweSource

    count = len(ROW_SEEDS)
    assert count == 7 == len(set(ROW_SEEDS)) and count > cap
    bodies = ING._rand(n + cap, count)
    want = R.seeded_rows(orc, ROW_SEEDS, bodies, n)
    assert len({want[r, :n].tobytes() for r in range(count)}) == count
    with _cap(cap):
        got = eng.lwe_expand(LweSource("seeded_rows", n, bodies, seeds=ROW_SEEDS))
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("n", [742, 7])
def test_seeded_list_under_the_cap(orc, eng, n):
    """7 rows of one stream on one workgroup; at n = 742 the stream takes 11 trips"""
    from tfhe_mi355 import LweSource

    seed, count = 0xFEDCBA9876543210_0123456789ABCDEF, 7
    bodies = ING._rand(n + 3, count)
    with _cap(1):
        got = eng.lwe_expand(LweSource("seeded_list", n, bodies, seeds=seed))
    assert np.array_equal(got, R.seeded_list(orc, seed, bodies, n))


@gpu
def test_apply_from_a_compact_source_under_the_cap():
    """one composed call on 2_2 (real keys, lwe_dimension cut to 8): 19 rows of a compact list expanded by two
    workgroups inside apply_from equal lwe_expand followed by KS -> PBS, both without the cap, and decrypt"""
    from tfhe_mi355 import fill_accumulator
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS

    K = ING.Keyed(PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    try:
        op, count = "ks_pbs", 19
        luts = np.stack([fill_accumulator(K.p, f) for f in (lambda x: (3 * x + 1) % 16, lambda x: (x * x) % 16)])
        msgs = (np.arange(count, dtype=U64) * U64(5) + U64(count)) % U64(16)
        idx = (np.arange(count) % 2).astype(np.uint32)
        src = K.source("compact", op, msgs)
        want = K.direct(op, K.eng.lwe_expand(src), luts, idx)
        with _cap(2):
            got = K.eng.apply_from(op, src, luts, idx)
        assert np.array_equal(got, want), "apply_from under the cap differs from lwe_expand followed by the entry point"
        assert np.array_equal(K.decrypt(op, got), np.where(idx == 0, (3 * msgs + 1) % 16, (msgs * msgs) % 16))
    finally:
        K.eng.close()
