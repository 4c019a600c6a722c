"""Compressed ciphertext ingress on the GPU (csrc/lwe_ingress.hip, csrc/capi_ingress.cpp), bit-exact throughout.

  expansion      tfhe_mi355_lwe_expand[_async] against the numpy restatement (tests/lwe_ingress_reference.py) and,
                 for the seeded forms, the oracle's AES-CTR stream;
  guard bands    every new device-pointer entry point as a case of tests/test_async_guards_gpu.py's runner (registered
                 with its `case` decorator, so the header-completeness check of tests/test_guarded_arena.py sees them);
  composition    tfhe_mi355_apply_from[_async] against lwe_expand followed by the operation's own entry point, and by
                 decryption; the refusals; a captured hipGraph; the shortint mirror.

The guarded cases are registered when this module is imported, which pytest does while it collects tests/: the
completeness check of tests/test_guarded_arena.py therefore counts them in a run over tests/ (with or without -m gpu),
not in a run of that file alone.

The host pipeline takes chunks of at least 1024 rows and TFHE_MI355_HOST_CHUNK is read once per process, so the
composed tests reach two chunks with 1025 rows, the smallest count that does.
"""
import dataclasses

import numpy as np
import pytest

import lwe_ingress_reference as R
import test_async_guards_gpu as G
from conftest import decode

pytestmark = pytest.mark.gpu

U64 = np.uint64
KIND = {"rows": 0, "compact": 1, "seeded_list": 2, "seeded_rows": 3}
TWO_CHUNKS = 1025


def _rand(seed, *shape):
    a = np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=U64)
    a.reshape(-1)[:2] = [0, 1 << 63][:a.size]  # the fixed points of negation
    return a


def _seeds(count):
    """all-zero, all-ones, two equal ones in front, then distinct"""
    s = [0, (1 << 128) - 1, 0x0123456789ABCDEF_FEDCBA9876543210, 0x0123456789ABCDEF_FEDCBA9876543210]
    s += [(i * 0x9E3779B97F4A7C15F39CC0605CEDC835) % (1 << 128) for i in range(4, count)]
    return s[:count] if count > 1 else [0x0123456789ABCDEF_FEDCBA9876543210]


@pytest.fixture(scope="module")
def eng():
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    e = Engine(P.with_(lwe_dimension=4), 0)  # expansion takes the caller's n, whatever the context's
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(U64)


# ---- 4. compact expansion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 256, 2048])
def test_compact_expansion_matches_the_restatement(eng, n):
    from tfhe_mi355 import LweSource

    for count in (1, n - 1, n, n + 1, 2 * n + 3):
        box = _rand(n + count, R.compact_words(n, count))
        want = R.expand_compact(box, n, count)
        got = eng.lwe_expand(LweSource("compact", n, box, count=count))
        assert np.array_equal(got, want), (n, count)


@pytest.mark.parametrize("n", [8, 256, 2048])
@pytest.mark.parametrize("offset", [16, 24])
def test_compact_expansion_async_at_both_row_parities(eng, n, offset):
    """the output base 16 and 24 bytes into an aligned buffer: rows are 8-byte aligned and n + 1 is odd, so the
    16-byte stores meet rows at 0 and at 8 modulo 16, from either start"""
    import torch

    from tfhe_mi355 import LweSource

    count = 2 * n + 3
    box = _rand(n + offset, R.compact_words(n, count))
    d_box = _dev(box)
    buf = torch.full((count * (n + 1) + 8,), -1, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 256 == 0
    eng.lwe_expand_async(LweSource("compact", n, d_box, count=count), buf.data_ptr() + offset)
    got = _host(buf)
    w = offset // 8
    assert np.array_equal(got[w:w + count * (n + 1)].reshape(count, n + 1), R.expand_compact(box, n, count))
    ones = U64((1 << 64) - 1)
    assert (got[:w] == ones).all() and (got[w + count * (n + 1):] == ones).all()


# ---- 5, 6. seeded expansion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 742, 2048])
def test_seeded_list_matches_the_oracle_stream(eng, orc, n):
    from tfhe_mi355 import LweSource

    seed = 0xFEDCBA9876543210_0123456789ABCDEF
    for count in (1, 3, 257):
        bodies = _rand(n + count, count)
        got = eng.lwe_expand(LweSource("seeded_list", n, bodies, seeds=seed))
        assert np.array_equal(got, R.seeded_list(orc, seed, bodies, n)), (n, count)


@pytest.mark.parametrize("n", [1, 7, 742, 2048])
def test_seeded_rows_match_the_oracle_stream_of_each_seed(eng, orc, n):
    """pins the device key schedule: every row against the oracle stream of its own seed"""
    from tfhe_mi355 import LweSource

    for count in (1, 2, 257):
        bodies, seeds = _rand(n + count, count), _seeds(count)
        got = eng.lwe_expand(LweSource("seeded_rows", n, bodies, seeds=seeds))
        assert np.array_equal(got, R.seeded_rows(orc, seeds, bodies, n)), (n, count)
        if count == 257:
            assert np.array_equal(got[2, :n], got[3, :n]) and not np.array_equal(got[0, :n], got[1, :n])


def test_core_crypto_mirror(eng, orc):
    from tfhe_mi355 import core_crypto as CC

    n, count = 16, 19
    box = _rand(1, R.compact_words(n, count))
    out = np.zeros((count, n + 1), dtype=U64)
    CC.par_expand_lwe_compact_ciphertext_list(out, box, eng)
    assert np.array_equal(out, R.expand_compact(box, n, count))
    bodies = _rand(2, 5)
    out = np.zeros((5, 8), dtype=U64)
    CC.decompress_seeded_lwe_ciphertext_list(out, bodies, 77, eng)
    assert np.array_equal(out, R.seeded_list(orc, 77, bodies, 7))
    one = np.zeros(8, dtype=U64)
    CC.decompress_seeded_lwe_ciphertext(one, int(bodies[0]), 78, eng)
    assert np.array_equal(one, R.seeded_rows(orc, [78], bodies[:1], 7)[0])
    with pytest.raises(ValueError):
        CC.decompress_seeded_lwe_ciphertext_list(np.zeros((4, 8), dtype=U64), bodies, 77, eng)


def test_expansion_refusals_and_empty_calls(eng):
    from tfhe_mi355 import EngineError, LweSource

    assert eng.lwe_expand(LweSource("seeded_list", 5, np.zeros(0, dtype=U64), seeds=1)).shape == (0, 6)
    with pytest.raises(EngineError, match="power of two"):
        eng.lwe_expand(LweSource("compact", 6, np.zeros(R.compact_words(6, 2), dtype=U64), count=2))
    with pytest.raises(EngineError, match="kind"):
        eng.lwe_expand_scratch_bytes(4, 8, 1)
    with pytest.raises(EngineError, match="lwe_dimension"):
        eng.lwe_expand_scratch_bytes(1, 0, 1)
    rows = _rand(3, 4, 9)
    assert np.array_equal(eng.lwe_expand(LweSource("rows", 8, rows)), rows)
    assert [eng.lwe_expand_scratch_bytes(k, 8, 3) for k in range(4)] == [0, 0, eng.lwe_expand_scratch_bytes(2, 8, 1), 0]
    assert eng.lwe_expand_scratch_bytes(2, 8, 3) > 0 == eng.lwe_expand_scratch_bytes(2, 8, 0)


# ---- 7. guard bands: the new _async entry points as cases of the guarded runner -----------------------------------
INGRESS = "ingress2048"
G.FACTORIES[INGRESS] = lambda orc: G._pbs_engine(orc, 2048, 1, 1, 23, 2, 0, True)
_FIRST_CASE = len(G.CASES)


def _source_regions(kind, n, count, seed):
    """(regions, host arrays) of a source of `count` rows"""
    if kind == "rows":
        data, seeds = _rand(seed, count, n + 1), None
    elif kind == "compact":
        data, seeds = _rand(seed, R.compact_words(n, count)), None
    else:
        data = _rand(seed, count)
        seeds = np.array([[s & (2 ** 64 - 1), s >> 64] for s in (_seeds(count) if kind == "seeded_rows" else [77 << 70 | 5])],
                         dtype=U64)
    regions = [G._rin("data", data, row=(n + 1) * 8 if kind == "rows" else 8)]
    if seeds is not None:
        regions.append(G._rin("seeds", seeds, row=16))
    return regions, data, seeds


def _reference_rows(orc, kind, n, count, data, seeds):
    ints = None if seeds is None else [int(lo) | int(hi) << 64 for lo, hi in seeds]
    if kind == "rows":
        return data
    if kind == "compact":
        return R.expand_compact(data, n, count)
    if kind == "seeded_list":
        return R.seeded_list(orc, ints[0], data, n)
    return R.seeded_rows(orc, ints, data, n)


def _expand_case(kind, n, count):
    @G.case(f"lwe_expand-{kind}-n{n}-{count}", INGRESS, ["lwe_expand_async"])
    def build(E, orc):
        from tfhe_mi355 import LweSource

        eng = E.eng
        regions, data, seeds = _source_regions(kind, n, count, n + count)
        need = eng.lwe_expand_scratch_bytes(KIND[kind], n, count)
        regions.append(G._rout("out", count * (n + 1) * 8, row=(n + 1) * 8))
        if need:
            regions.append(G._rout("scratch", need))

        def call(v):
            src = LweSource(kind, n, v["data"], v.get("seeds"), count=count)
            eng.lwe_expand_async(src, v["out"], d_scratch=v.get("scratch"))

        rows = G._sample(count)
        return G._spec(regions, call, lambda: eng.lwe_expand(LweSource(kind, n, data, seeds, count=count)), "out",
                       ("scratch", need) if need else (None, 0), None,
                       oracle=lambda: (rows, _reference_rows(orc, kind, n, count, data, seeds)[rows]),
                       out_row=(n + 1) * 8)
    return build


for _kind, _n, _count in (("compact", 8, 19), ("compact", 2048, 5), ("seeded_list", 7, 257), ("seeded_list", 742, 3),
                          ("seeded_rows", 7, 257), ("seeded_rows", 2048, 2), ("rows", 7, 5)):
    _expand_case(_kind, _n, _count)


def _apply_case(op, kind, count):
    @G.case(f"apply_from-{op}-{kind}-{count}", INGRESS, ["apply_from_async"])
    def build(E, orc):
        from tfhe_mi355 import LweSource

        eng, p = E.eng, E.p
        n = p.lwe_dimension if op in ("pbs", "pbs_ks") else p.big_lwe_dimension
        w_out = (p.lwe_dimension if op in ("pbs_ks", "ks") else p.big_lwe_dimension) + 1
        regions, data, seeds = _source_regions(kind, n, count, 3 * count + len(op))
        luts = _rand(count + 1, 2, eng.glwe_len)
        idx = (np.arange(count) % 2).astype(np.uint32)
        lut = op != "ks"
        if lut:
            regions += [G._rin("luts", luts, row=eng.glwe_len * 8), G._rin("lut_indexes", idx, row=4)]
        need = eng.apply_from_scratch_bytes(op, KIND[kind], count)
        regions.append(G._rout("out", count * w_out * 8, row=w_out * 8))
        if need:
            regions.append(G._rout("scratch", need))

        def call(v):
            src = LweSource(kind, n, v["data"], v.get("seeds"), count=count)
            eng.apply_from_async(op, src, v["out"], v.get("luts"), 2 if lut else 0, v.get("lut_indexes"),
                                 d_scratch=v.get("scratch"))

        def twin():
            return eng.apply_from(op, LweSource(kind, n, data, seeds, count=count), luts if lut else None,
                                  idx if lut else None)

        return G._spec(regions, call, twin, "out", ("scratch", need) if need else (None, 0), None, out_row=w_out * 8)
    return build


for _op, _kind, _count in (("ks_pbs", "compact", 5), ("ks_pbs", "seeded_list", 3), ("ks", "seeded_rows", 5),
                           ("pbs", "compact", 5), ("pbs_ks", "seeded_rows", 3), ("pbs_ks", "seeded_list", 5),
                           ("ks", "rows", 3)):
    _apply_case(_op, _kind, _count)

INGRESS_CASES = G.CASES[_FIRST_CASE:]
G._LAST_OF_ENGINE[INGRESS] = INGRESS_CASES[-1].id


@pytest.mark.parametrize("c", INGRESS_CASES, ids=lambda c: c.id)
def test_guarded_ingress_call(orc, c):
    """the five checks of test_async_guards_gpu.test_guarded_call: the host-pointer twin word for word (and the
    restatement on sampled rows), no byte changed outside the output and the scratch, the scratch of exactly the
    queried size, the same output from other prior contents, the resident keys unchanged"""
    G.test_guarded_call(orc, c)


def test_scratch_one_byte_short_is_refused(eng):
    import torch

    from tfhe_mi355 import EngineError, LweSource

    n, count = 7, 3
    need = eng.lwe_expand_scratch_bytes(2, n, count)
    src = LweSource("seeded_list", n, _dev(_rand(1, count)), _dev(np.array([1, 2], dtype=U64)), count=count)
    out = torch.zeros(count * (n + 1), dtype=torch.int64, device="cuda")
    with pytest.raises(EngineError, match="scratch"):
        eng.lwe_expand_async(src, out, d_scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert not out.any()


# ---- 8. composed calls ---------------------------------------------------------------------------------------
class Keyed:
    """an engine under real (client-generated) keys of a parameter set with its small dimension cut to 8"""

    def __init__(self, params):
        from tfhe_mi355 import Engine, client

        p = self.p = params.with_(lwe_dimension=8)
        self.small = client.gen_binary_key(21, 1, p.lwe_dimension)
        self.big = client.gen_binary_key(21, 2, p.big_lwe_dimension)
        self.eng = Engine(p, 0)
        self.eng.upload_bootstrap_key(client.gen_bootstrap_key(22, self.small, self.big, p.glwe_dimension, p.polynomial_size,
                                                               p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev))
        self.eng.upload_keyswitch_key(client.gen_keyswitch_key(23, self.big, self.small, p.ks_base_log, p.ks_level,
                                                               p.lwe_modular_std_dev))

    def source(self, kind, op, msgs):
        """a source of `kind` encrypting msgs under the input key of `op`"""
        from tfhe_mi355 import LweSource, client

        p = self.p
        key, std = (self.small, p.lwe_modular_std_dev) if op in ("pbs", "pbs_ks") else (self.big, p.glwe_modular_std_dev)
        pts = msgs * U64(p.delta)
        if kind == "compact":
            pk = client.gen_compact_public_key(31, key, std)
            return LweSource(kind, len(key), client.compact_encrypt(32, pk, pts, std), count=len(msgs))
        if kind == "seeded_list":
            return LweSource(kind, len(key), client.seeded_lwe_encrypt_list(33, 0xABCD << 64 | 9, key, pts, std),
                             seeds=0xABCD << 64 | 9)
        seeds = _seeds(len(msgs))
        return LweSource(kind, len(key), client.seeded_lwe_encrypt(34, seeds, key, pts, std), seeds=seeds)

    def direct(self, op, rows, luts, idx):
        e = self.eng
        return {"pbs": lambda: e.programmable_bootstrap(rows, luts, idx),
                "ks_pbs": lambda: e.keyswitch_programmable_bootstrap(rows, luts, idx),
                "pbs_ks": lambda: e.programmable_bootstrap_keyswitch(rows, luts, idx),
                "ks": lambda: e.keyswitch(rows)}[op]()

    def decrypt(self, op, out):
        from tfhe_mi355 import client

        key = self.small if op in ("pbs_ks", "ks") else self.big
        return decode(client.lwe_decrypt(key, out), self.p.delta) % U64(16)


@pytest.fixture(scope="module")
def keyed_2_2():
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS

    k = Keyed(PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    yield k
    k.eng.close()


@pytest.fixture(scope="module")
def keyed_compact():
    from tfhe_mi355.parameters import PARAM_MESSAGE_3_CARRY_1_COMPACT_PK_PBS_KS

    k = Keyed(PARAM_MESSAGE_3_CARRY_1_COMPACT_PK_PBS_KS)  # N = 2048, keyswitch 6 x 3, 16 plaintext values
    yield k
    k.eng.close()


def _composed(K, op, kind, count):
    from tfhe_mi355 import fill_accumulator

    f = [lambda x: (3 * x + 1) % 16, lambda x: (x * x) % 16]
    luts = np.stack([fill_accumulator(K.p, g) for g in f])
    msgs = (np.arange(count, dtype=U64) * U64(5) + U64(count)) % U64(16)
    idx = (np.arange(count) % 2).astype(np.uint32)
    src = K.source(kind, op, msgs)
    got = K.eng.apply_from(op, src, None if op == "ks" else luts, None if op == "ks" else idx)
    want = K.direct(op, K.eng.lwe_expand(src), luts, idx)
    assert np.array_equal(got, want), "apply_from differs from lwe_expand followed by the entry point"
    expect = msgs if op == "ks" else np.where(idx == 0, (3 * msgs + 1) % 16, (msgs * msgs) % 16)
    assert np.array_equal(K.decrypt(op, got), expect)


@pytest.mark.parametrize("count", [1, 300, TWO_CHUNKS])
@pytest.mark.parametrize("kind", ["compact", "seeded_list", "seeded_rows"])
@pytest.mark.parametrize("op", ["ks_pbs", "ks"])
def test_apply_from_on_2_2(keyed_2_2, op, kind, count):
    _composed(keyed_2_2, op, kind, count)


@pytest.mark.parametrize("count", [1, 300, TWO_CHUNKS])
@pytest.mark.parametrize("kind", ["compact", "seeded_list", "seeded_rows"])
@pytest.mark.parametrize("op", ["pbs", "pbs_ks"])
def test_apply_from_on_a_compact_pk_set(keyed_compact, op, kind, count):
    _composed(keyed_compact, op, kind, count)


def test_apply_from_rows_is_the_existing_call(keyed_2_2):
    from tfhe_mi355 import LweSource, fill_accumulator

    K = keyed_2_2
    rows = _rand(5, 70, K.p.big_lwe_dimension + 1)
    lut = fill_accumulator(K.p, lambda x: x)
    assert np.array_equal(K.eng.apply_from("ks_pbs", LweSource("rows", K.p.big_lwe_dimension, rows), lut),
                          K.eng.keyswitch_programmable_bootstrap(rows, lut))


def test_apply_from_refusals(keyed_2_2):
    from tfhe_mi355 import Engine, EngineError, LweSource, fill_accumulator
    from tfhe_mi355 import boolean as Bm

    K = keyed_2_2
    lut = fill_accumulator(K.p, lambda x: x)
    src = lambda n: LweSource("seeded_list", n, np.zeros(3, dtype=U64), seeds=1)  # noqa: E731
    with pytest.raises(EngineError, match="lwe_dimension 8, but op 1 takes rows of dimension 2048"):
        K.eng.apply_from("ks_pbs", src(8), lut)
    with pytest.raises(EngineError, match="lwe_dimension 2048, but op 0 takes rows of dimension 8"):
        K.eng.apply_from("pbs", src(2048), lut)
    with pytest.raises(EngineError, match="lwe_dimension"):
        K.eng.apply_from_async("ks", LweSource("seeded_list", 8, _dev(np.zeros(3, dtype=U64)), _dev(np.zeros(2, dtype=U64)),
                                               count=3), _dev(np.zeros(27, dtype=U64)))
    multi = Engine(K.p, devices=[0, 0])
    try:
        with pytest.raises(EngineError, match="multi-device"):
            multi.apply_from("ks_pbs", src(2048), lut)
        with pytest.raises(EngineError, match="multi-device"):
            multi.apply_from_scratch_bytes("ks_pbs", 1, 3)
    finally:
        multi.close()
    p32 = dataclasses.replace(Bm.DEFAULT_PARAMETERS, lwe_dimension=3, name="ingress_u32")
    e32 = Engine(p32, 0)
    try:
        rng = np.random.default_rng(1)
        k, N = p32.glwe_dimension, p32.polynomial_size
        e32.upload_bootstrap_key_u32(rng.integers(0, 1 << 32, 3 * p32.pbs_level * (k + 1) * (k + 1) * N, dtype=np.uint32))
        e32.upload_keyswitch_key_u32(rng.integers(0, 1 << 32, k * N * p32.ks_level * 4, dtype=np.uint32))
        with pytest.raises(EngineError, match="32-bit-torus keys"):
            e32.apply_from("ks", LweSource("seeded_list", k * N, np.zeros(3, dtype=U64), seeds=1))
    finally:
        e32.close()
    fresh = Engine(K.p, 0)
    try:
        with pytest.raises(EngineError, match="key not uploaded"):
            fresh.apply_from("ks", src(2048))
    finally:
        fresh.close()


def test_apply_from_scratch_one_byte_short_is_refused(keyed_2_2):
    import torch

    from tfhe_mi355 import EngineError, LweSource

    K, count = keyed_2_2, 3
    n = K.p.big_lwe_dimension
    for kind in ("compact", "seeded_list", "seeded_rows"):
        host = K.source(kind, "ks", np.arange(count, dtype=U64))
        src = LweSource(kind, n, _dev(host.data), None if host.seeds is None else _dev(host.seeds), count=count)
        need = K.eng.apply_from_scratch_bytes("ks", KIND[kind], count)
        assert need >= count * (n + 1) * 8
        out = torch.zeros(count * (K.p.lwe_dimension + 1), dtype=torch.int64, device="cuda")
        with pytest.raises(EngineError, match="scratch"):
            K.eng.apply_from_async("ks", src, out, d_scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        assert not out.any()
        K.eng.apply_from_async("ks", src, out, d_scratch=torch.empty(need, dtype=torch.uint8, device="cuda"))
        assert np.array_equal(_host(out).reshape(count, -1), K.eng.apply_from("ks", host))


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------
def test_apply_from_async_replays_in_a_graph(keyed_2_2):
    """captured once, replayed with other bodies: the outputs follow the bodies (no host state in the call)"""
    import torch

    from tfhe_mi355 import LweSource, fill_accumulator

    K, count, op = keyed_2_2, 6, "ks_pbs"
    n = K.p.big_lwe_dimension
    lut = fill_accumulator(K.p, lambda x: (x + 7) % 16)
    d_lut = _dev(lut)
    srcs = [K.source("seeded_list", op, (np.arange(count, dtype=U64) + U64(s)) % U64(16)) for s in (0, 3, 9)]
    d_bodies, d_seed = _dev(srcs[0].data), _dev(srcs[0].seeds)
    d_out = torch.zeros(count * (n + 1), dtype=torch.int64, device="cuda")
    scratch = torch.empty(K.eng.apply_from_scratch_bytes(op, 2, count), dtype=torch.uint8, device="cuda")
    d_src = LweSource("seeded_list", n, d_bodies, d_seed, count=count)
    K.eng.apply_from_async(op, d_src, d_out, d_lut, 1, d_scratch=scratch)  # warm-up, outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.eng.apply_from_async(op, d_src, d_out, d_lut, 1, d_scratch=scratch)
    for s in srcs[1:]:
        d_bodies.copy_(_dev(s.data))
        d_out.zero_()
        g.replay()
        got = _host(d_out).reshape(count, n + 1)
        assert np.array_equal(got, K.eng.apply_from(op, s, lut))


# ---- 10. the shortint mirror ---------------------------------------------------------------------------------
def test_server_key_takes_compressed_batches(keyed_2_2):
    from tfhe_mi355 import shortint as SI

    K = keyed_2_2
    ck = SI.ClientKey(K.p, seed=21)
    assert np.array_equal(ck.small_lwe_secret_key, K.small) and np.array_equal(ck.glwe_secret_key, K.big)
    sks = SI.ServerKey(None, engine=K.eng, parameters=K.p)
    msgs = [0, 1, 2, 3, 3, 1, 2]
    acc, acc2 = sks.generate_lookup_table(lambda x: (x + 1) % 4), sks.generate_lookup_table(lambda x: (2 * x) % 4)
    accs = [acc if i % 2 == 0 else acc2 for i in range(len(msgs))]
    want = [(m + 1) % 4 if i % 2 == 0 else (2 * m) % 4 for i, m in enumerate(msgs)]

    lst = SI.CompactCiphertextList.deserialize(SI.CompactPublicKey(ck).encrypt_many(msgs).serialize())
    out = sks.apply_lookup_table_batch(lst, accs)
    ref = sks.apply_lookup_table_batch(lst.expand(sks), accs)
    assert all(np.array_equal(a.ct, b.ct) and a.degree == b.degree for a, b in zip(out, ref))
    assert [ck.decrypt(c) for c in out] == want

    comp = [SI.CompressedCiphertext.deserialize(c.serialize()) for c in ck.encrypt_compressed_many(msgs)]
    out = sks.apply_lookup_table_batch(comp, acc)
    ref = sks.apply_lookup_table_batch([c.decompress(sks) for c in comp], acc)
    assert all(np.array_equal(a.ct, b.ct) for a, b in zip(out, ref))
    assert [ck.decrypt(c) for c in out] == [(m + 1) % 4 for m in msgs]


# ---- the accepted compact-public-key sets on the device --------------------------------------------------------
def test_accepted_compact_pk_sets_create_contexts_and_refused_ones_do_not():
    from tfhe_mi355 import Engine, EngineError
    from tfhe_mi355 import parameters as P

    for p in P.COMPACT_PK_ALL.values():
        Engine(p, 0).close()
    table = {t[0]: t for t in P._COMPACT_PK_TABLE}
    for name, msg in P.COMPACT_PK_REFUSED:
        t = table[name]
        p = P.ClassicPBSParameters(t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11], t[12], t[13], 0, name)
        if t[4] == 65536:
            with pytest.raises(EngineError, match="no kernel for N=65536"):
                Engine(p, 0)
        else:  # the context exists; its keyswitch refuses the decomposition at the call (n cut: a small key)
            e = Engine(p.with_(lwe_dimension=4), 0)
            try:
                e.upload_keyswitch_key(np.zeros(p.big_lwe_dimension * p.ks_level * 5, dtype=U64))
                with pytest.raises(EngineError) as err:
                    e.keyswitch(np.zeros((2, p.big_lwe_dimension + 1), dtype=U64))
                assert msg in str(err.value)
            finally:
                e.close()


def test_keyswitch_decompositions_new_with_the_compact_sets_match_the_oracle(orc):
    """the accepted sets bring keyswitch decompositions no earlier set has (2 x 6, 5 x 4, 2 x 11, 1 x 21, 1 x 22; the
    last two have more levels than the scalar arm takes, so the int8-MFMA arm alone serves them)"""
    from tfhe_mi355 import Engine
    from tfhe_mi355 import parameters as P

    old = {(p.ks_base_log, p.ks_level) for p in P.ALL.values()}
    new = sorted({(p.ks_base_log, p.ks_level) for p in P.COMPACT_PK_ALL.values()} - old)
    assert new == [(1, 21), (1, 22), (2, 6), (2, 11), (5, 4)]
    e = Engine(P.PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(lwe_dimension=4), 0)
    try:
        for base_log, level in new:
            in_dim, out_dim = 300, 9
            ksk = _rand(base_log * 100 + level, in_dim * level * (out_dim + 1))
            cts = _rand(level, 5, in_dim + 1)
            key = e.keyswitch_key(ksk, in_dim, out_dim, base_log, level)
            try:
                got = e.keyswitch_with_key(key, cts)
            finally:
                key.close()
            assert np.array_equal(got, orc.keyswitch(ksk, in_dim, out_dim, base_log, level, cts)), (base_log, level)
    finally:
        e.close()
