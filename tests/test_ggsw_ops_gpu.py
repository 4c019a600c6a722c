"""GGSW external product, CMUX and vertical packing on the GPU (csrc/ggsw_ops.hip through the C
ABI), bit-exact (np.array_equal) against the CPU reference of tests/ggsw_reference.py, which is
built from the oracle's blind rotation (tests/test_ggsw_ops.py checks that reference itself).

Shapes (N, k, base_log, level), the smallest that reach every code path: (2048, 1, 5, 3) the WoP 2_2
circuit-bootstrap decomposition; (1024, 2, 7, 3); (512, 3, 4, 6) the deepest level loop; (256, 5, 14,
1) one level, most rows; and the two edges of the 32-bit decomposer, base_log * level = 32 as two
levels of 16 bits and as one level of 32 bits (the digit +2^31).
"""
import numpy as np
import pytest

from ggsw_reference import Ref, ggsw_words, index_bits, lut_value, vp_lut

pytestmark = pytest.mark.gpu

U64 = np.uint64
GLWE_STD = 2.94036859086e-16
SHAPES = [(2048, 1, 5, 3), (1024, 2, 7, 3), (512, 3, 4, 6), (256, 5, 14, 1)]
EDGE_SHAPES = [(256, 5, 16, 2), (256, 5, 32, 1)]
WOP = SHAPES[0]
_cache = {}


def _params(params_2_2, N, k):
    return params_2_2.with_(glwe_dimension=k, polynomial_size=N, pbs_level=1, name=f"ggsw_{N}_{k}")


def _engine(params_2_2, N, k):
    from tfhe_mi355 import Engine

    key = ("engine", N, k)
    if key not in _cache:
        _cache[key] = Engine(_params(params_2_2, N, k), 0)
    return _cache[key]


def _sk(N, k):
    from tfhe_mi355 import client

    key = ("sk", N, k)
    if key not in _cache:
        _cache[key] = client.gen_binary_key(1000 + N + k, 2, k * N)
    return _cache[key]


def _ggsws(bits, shape, seed):
    from tfhe_mi355 import client

    N, k, B, L = shape
    return client.gen_ggsw_list(seed, bits, _sk(N, k), k, N, B, L, GLWE_STD).reshape(len(bits), -1)


def _node_case(orc, shape):
    """5 items and 5 GGSWs of one shape, with the reference products P[g][i] = G_g (x) (ct1_i - ct0_i)
    of every pair computed once.  Rows: ct0 == ct1 (the increment is exactly 0, and the all-zero
    external-product input); ct0 = 0 with every word of ct1 = 1 << 63, and all ones; ct0 all ones with
    ct1 = 0; random."""
    key = ("nodes", shape)
    if key in _cache:
        return _cache[key]
    N, k, B, L = shape
    glwe = (k + 1) * N
    rng = np.random.default_rng(N + 7 * k + B)
    ct0 = rng.integers(0, 1 << 64, (5, glwe), dtype=U64)
    ct1 = rng.integers(0, 1 << 64, (5, glwe), dtype=U64)
    ct1[0] = ct0[0]
    ct0[1], ct1[1] = 0, U64(1 << 63)
    ct0[2], ct1[2] = 0, ~U64(0)
    ct0[3], ct1[3] = ~U64(0), 0
    g = _ggsws([1, 0, 1, 1, 0], shape, 50 + B)
    ref = Ref(orc, k, N, B, L)
    d = ct1 - ct0
    P = np.stack([ref.external_product(g[i], d) for i in range(5)])
    _cache[key] = dict(ct0=ct0, ct1=ct1, d=d, g=g, P=P, inout=rng.integers(0, 1 << 64, (5, glwe), dtype=U64))
    return _cache[key]


IDX = np.array([4, 2, 2, 0, 3], dtype=np.uint32)  # permuted, repeating


def _picked(c, idx):
    sel = np.arange(5) if idx is None else idx
    return c["P"][sel, np.arange(5)]


@pytest.mark.parametrize("shape", SHAPES + EDGE_SHAPES, ids=str)
@pytest.mark.parametrize("idx", [None, IDX], ids=["own", "indexed"])
def test_external_product_bit_exact(orc, params_2_2, shape, idx):
    N, k, B, L = shape
    eng = _engine(params_2_2, N, k)
    c = _node_case(orc, shape)
    got = eng.ggsw_external_product(c["g"], B, L, c["d"], c["inout"].copy(), idx)
    assert np.array_equal(got, c["inout"] + _picked(c, idx))
    assert np.array_equal(got[0], c["inout"][0])  # the all-zero input adds exactly 0


@pytest.mark.parametrize("shape", SHAPES + EDGE_SHAPES, ids=str)
@pytest.mark.parametrize("idx", [None, IDX], ids=["own", "indexed"])
def test_cmux_bit_exact(orc, params_2_2, shape, idx):
    N, k, B, L = shape
    eng = _engine(params_2_2, N, k)
    c = _node_case(orc, shape)
    exp = c["ct0"] + _picked(c, idx)
    ct1 = c["ct1"].copy()
    got = eng.ggsw_cmux(c["g"], B, L, c["ct0"], ct1, idx)
    assert np.array_equal(got, exp)
    assert np.array_equal(got[0], c["ct0"][0])  # ct0 == ct1: the increment is exactly 0
    assert np.array_equal(ct1, c["ct1"])
    a = c["ct0"].copy()
    assert eng.ggsw_cmux(c["g"], B, L, a, c["ct1"], idx, out=a) is a  # out == ct0
    assert np.array_equal(a, exp)


def test_core_crypto_mirror(orc, params_2_2):
    from tfhe_mi355 import core_crypto as cc

    N, k, B, L = WOP
    eng = _engine(params_2_2, N, k)
    c = _node_case(orc, WOP)
    ggsw = cc.GgswCiphertextList(c["g"], k + 1, N, B, L)
    out = c["inout"].copy()
    cc.add_external_product_assign(out, ggsw, c["d"], eng)
    assert np.array_equal(out, c["inout"] + _picked(c, None))
    ct0 = c["ct0"].copy()
    cc.cmux_assign(ct0, c["ct1"], ggsw, eng)
    assert np.array_equal(ct0, c["ct0"] + _picked(c, None))


# ---- vertical packing ---------------------------------------------------------------------------
def _vp_case(orc, shape, nt, nr):
    """3 items with different index bits, two LUTs through lut_indexes; the composed reference."""
    key = ("vp", shape, nt, nr)
    if key in _cache:
        return _cache[key]
    N, k, B, L = shape
    nbits, npoly = nt + nr, 1 << nt
    rng = np.random.default_rng(100 * nt + nr)
    top = 1 << nbits
    indices = [top - 1, int(rng.integers(0, top)), (top // 3) | 1 if top > 2 else 0]
    bits = [b for i in indices for b in index_bits(i, nbits)]
    g = _ggsws(bits, shape, 70 + nbits).reshape(3, nbits, -1)
    if shape == WOP:
        luts = np.stack([vp_lut(npoly, N, nr, 1 << 60, 0), vp_lut(npoly, N, nr, 1 << 60, 5)])
    else:
        luts = rng.integers(0, 1 << 64, (2, npoly, N), dtype=U64)
    lut_idx = np.array([0, 1, 0], dtype=np.uint32)
    ref = Ref(orc, k, N, B, L)
    exp = np.stack([ref.vertical_packing(g[i], luts[lut_idx[i]]) for i in range(3)])
    _cache[key] = dict(g=g, luts=luts, lut_idx=lut_idx, exp=exp, indices=indices, nbits=nbits, npoly=npoly)
    return _cache[key]


VP_CASES = [(WOP, 0, 1), (WOP, 1, 0), (WOP, 3, 2), (WOP, 0, 11), (SHAPES[3], 2, 8)]


@pytest.mark.parametrize("shape,nt,nr", VP_CASES, ids=str)
def test_vertical_packing_bit_exact(orc, params_2_2, shape, nt, nr):
    N, k, B, L = shape
    eng = _engine(params_2_2, N, k)
    c = _vp_case(orc, shape, nt, nr)
    got = eng.vertical_packing(c["g"], B, L, c["luts"], c["lut_idx"])
    assert got.shape == (3, k * N + 1)
    assert np.array_equal(got, c["exp"])
    if shape == WOP:  # every output decrypts to LUT[index]
        pts = orc.lwe_decrypt(_sk(N, k), got)
        for i in range(3):
            want = lut_value(c["indices"][i] + (5 if c["lut_idx"][i] else 0))
            assert ((int(pts[i]) + (1 << 59)) >> 60) % 16 == want, (c["indices"][i], hex(int(pts[i])))
    # one LUT, no lut_indexes: LUT 0 for every item
    one = eng.vertical_packing(c["g"][:1], B, L, c["luts"][0])
    assert np.array_equal(one, c["exp"][:1])


def test_core_crypto_vertical_packing(orc, params_2_2):
    from tfhe_mi355 import core_crypto as cc

    N, k, B, L = WOP
    c = _vp_case(orc, WOP, 3, 2)
    out = np.zeros(k * N + 1, dtype=U64)
    cc.vertical_packing(c["luts"][0], out, cc.GgswCiphertextList(c["g"][0], k + 1, N, B, L), _engine(params_2_2, N, k))
    assert np.array_equal(out, c["exp"][0])


# ---- device-pointer forms -------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _fourier(eng, g_std, level):
    import torch

    g = np.ascontiguousarray(g_std, dtype=U64).reshape(-1, eng.ggsw_words(level))
    d_f = torch.empty(eng.ggsw_list_fourier_bytes(g.shape[0], level), dtype=torch.uint8, device="cuda")
    d_std = _dev(g)
    eng.ggsw_list_convert_async(d_std, g.shape[0], level, d_f)
    torch.cuda.current_stream().synchronize()
    return d_f


def test_async_forms_agree_with_the_synchronous_ones(orc, params_2_2):
    import torch

    N, k, B, L = WOP
    eng = _engine(params_2_2, N, k)
    c = _node_case(orc, WOP)
    d_f = _fourier(eng, c["g"], L)
    assert d_f.numel() == 5 * L * (k + 1) ** 2 * (N // 2) * 16
    d_idx = _dev(IDX.view(np.int32))
    for idx, d_i in ((None, None), (IDX, d_idx)):
        d_io = _dev(c["inout"])
        eng.ggsw_external_product_async(d_f, 5, B, L, _dev(c["d"]), d_io, 5, d_i)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(_host(d_io), c["inout"] + _picked(c, idx))
        d_ct0, d_out = _dev(c["ct0"]), _dev(np.zeros_like(c["ct0"]))
        eng.ggsw_cmux_async(d_f, 5, B, L, d_ct0, _dev(c["ct1"]), d_out, 5, d_i)
        eng.ggsw_cmux_async(d_f, 5, B, L, d_ct0, _dev(c["ct1"]), d_ct0, 5, d_i)  # out == ct0
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(_host(d_out), c["ct0"] + _picked(c, idx))
        assert np.array_equal(_host(d_ct0), c["ct0"] + _picked(c, idx))
    v = _vp_case(orc, WOP, 3, 2)
    d_fv = _fourier(eng, v["g"], L)
    d_out = _dev(np.zeros((3, k * N + 1), dtype=U64))
    eng.vertical_packing_async(d_fv, B, L, v["nbits"], _dev(v["luts"]), 2, v["npoly"], 3, d_out, _dev(v["lut_idx"].view(np.int32)))
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(_host(d_out), v["exp"])


def test_vertical_packing_scratch_is_required(orc, params_2_2):
    import torch

    from tfhe_mi355 import _lib
    from tfhe_mi355._lib import EngineError

    N, k, B, L = WOP
    eng = _engine(params_2_2, N, k)
    v = _vp_case(orc, WOP, 3, 2)
    d_fv = _fourier(eng, v["g"], L)
    need = eng.vertical_packing_scratch_bytes(v["npoly"], 3)
    assert need >= 3 * (4 + 2) * (k + 1) * N * 8
    d_out, d_luts = _dev(np.zeros((3, k * N + 1), dtype=U64)), _dev(v["luts"])
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (eng._h, d_fv.data_ptr(), B, L, v["nbits"], d_luts.data_ptr(), 2, v["npoly"], None, 3, d_out.data_ptr())
    for ptr, nbytes in ((None, 0), (None, need), (scratch.data_ptr(), need - 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_vertical_packing_async", *args, ptr, nbytes, stream)
    _lib.call("tfhe_mi355_vertical_packing_async", *args, scratch.data_ptr(), need, stream)
    torch.cuda.current_stream().synchronize()
    exp0 = np.stack([Ref(orc, k, N, B, L).vertical_packing(v["g"][i], v["luts"][0]) for i in (1,)])
    assert np.array_equal(_host(d_out)[[0, 2]], v["exp"][[0, 2]])  # lut_indexes NULL: LUT 0 (items 0 and 2)
    assert np.array_equal(_host(d_out)[1:2], exp0)


def test_rejected_arguments(orc, params_2_2):
    from tfhe_mi355 import Engine
    from tfhe_mi355._lib import EngineError

    N, k, B, L = WOP
    eng = _engine(params_2_2, N, k)
    w = ggsw_words(k, N, L)
    out = np.zeros(k * N + 1, dtype=U64)

    def vp(nbits, npoly, base_log=B, level=L):
        g = np.zeros((1, nbits * ggsw_words(k, N, level)), dtype=U64)
        return eng.vertical_packing(g, base_log, level, np.zeros((1, npoly, N), dtype=U64))

    with pytest.raises(EngineError, match="not a power of two"):
        vp(3, 3)
    with pytest.raises(EngineError, match="need 3 tree bits"):
        vp(2, 8)
    with pytest.raises(EngineError, match="exceed log2"):
        vp(12, 1)
    with pytest.raises(EngineError, match="base_log \\* level <= 32"):
        vp(3, 2, base_log=11, level=3)
    glwe = np.zeros((1, (k + 1) * N), dtype=U64)
    with pytest.raises(EngineError, match="base_log \\* level <= 32"):
        eng.ggsw_external_product(np.zeros(w, dtype=U64), 11, 3, glwe, glwe.copy())
    with pytest.raises(EngineError, match="base_log \\* level <= 32"):
        eng.ggsw_cmux(np.zeros(w, dtype=U64), 11, 3, glwe, glwe)
    with pytest.raises(EngineError, match="out of range"):
        eng.ggsw_external_product(np.zeros(w, dtype=U64), B, L, glwe, glwe.copy(), np.array([1], dtype=np.uint32))
    with pytest.raises(EngineError, match="for 2 items"):
        two = np.zeros((2, (k + 1) * N), dtype=U64)
        eng.ggsw_cmux(np.zeros(w, dtype=U64), B, L, two, two)
    big = Engine(params_2_2.with_(polynomial_size=4096, name="ggsw_4096"), 0)  # N outside the supported set
    g4 = np.zeros(ggsw_words(1, 4096, 1), dtype=U64)
    x4 = np.zeros((1, 2 * 4096), dtype=U64)
    with pytest.raises(EngineError, match="support N in"):
        big.ggsw_external_product(g4, 5, 1, x4, x4.copy())
    with pytest.raises(EngineError, match="support N in"):
        big.ggsw_cmux(g4, 5, 1, x4, x4)
    with pytest.raises(EngineError, match="support N in"):
        big.vertical_packing(g4.reshape(1, -1), 5, 1, np.zeros((1, 1, 4096), dtype=U64))
    big.close()


def test_multi_device_context_gives_the_single_device_outputs(orc, params_2_2):
    from tfhe_mi355 import Engine

    N, k, B, L = WOP
    multi = Engine(_params(params_2_2, N, k), devices=[0, 0])
    c = _node_case(orc, WOP)
    for idx in (None, IDX):
        got = multi.ggsw_external_product(c["g"], B, L, c["d"], c["inout"].copy(), idx)
        assert np.array_equal(got, c["inout"] + _picked(c, idx))
        assert np.array_equal(multi.ggsw_cmux(c["g"], B, L, c["ct0"], c["ct1"], idx), c["ct0"] + _picked(c, idx))
    v = _vp_case(orc, WOP, 3, 2)
    assert np.array_equal(multi.vertical_packing(v["g"], B, L, v["luts"], v["lut_idx"]), v["exp"])
    multi.close()
