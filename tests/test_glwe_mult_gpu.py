"""The GLWE product with relinearisation on the GPU (csrc/glwe_mult.hip and its entry points in
csrc/capi_gadget.cpp), bit-exact (np.array_equal) against the CPU reference of tests/glwe_mult_reference.py,
which is built from the oracle (tests/test_glwe_mult.py checks that reference).

Engine.glwe_mult runs on arbitrary words (exactness needs no valid ciphertext or key).  Shapes (k, N):
(1, 1024) one block and no R terms; (1, 2048) the most LDS and two output polynomials per thread in the
relinearisation; (2, 512) the first off-diagonal block, one idle thread group; (5, 256) 15 blocks, eight
thread groups.  Every shape runs the 6 x 4 decomposition at log_p 0, 2, 4, 64 (shifts 32, 31, 30, 0);
each of the others runs at one shape: (1, 3) one-bit digits, (31, 2) digits up to 2^30, (7, 9) 63 bits
(closest_representable shifts by 0), (23, 1) one level.  Rows: random; lhs all zero; both all ones (the
longest carry chain); both 1 << 63; all ones times random; a pair whose T_0 holds 2^63, the word whose
top digit is +2^(base_log - 1); then random up to 67 pairs.
"""
import numpy as np
import pytest

import glwe_mult_reference as R

pytestmark = pytest.mark.gpu

U64 = np.uint64
SHAPES = [(1, 1024), (1, 2048), (2, 512), (5, 256)]
OTHER_DECOMPOSITIONS = {(5, 256): (1, 3), (2, 512): (31, 2), (1, 1024): (7, 9), (1, 2048): (23, 1)}
COUNT = 67
_cache = {}


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _rows(k, N, rng):
    g = (k + 1) * N
    lhs, rhs = rng.integers(0, 1 << 64, (2, COUNT, g), dtype=U64)
    lhs[1] = 0
    lhs[2] = rhs[2] = ~U64(0)
    lhs[3] = rhs[3] = U64(1 << 63)
    lhs[4] = ~U64(0)
    # at log_p = 4: A_0 = 2^33 (a constant), A'_0[7] = 2^30, so T_0[7] = 2^63 and its top digit is +2^(B-1)
    lhs[5] = 0
    lhs[5, 0] = U64(1 << 63)
    rhs[5, 7] = U64(1 << 60)
    return lhs, rhs


def _case(params_2_2, k, N, B, L):
    """An engine of the shape with a key of random words uploaded, and the input rows, once."""
    key = ("case", k, N, B, L)
    if key not in _cache:
        from tfhe_mi355 import Engine

        rng = np.random.default_rng(1000 * k + N + 17 * B + L)
        eng = _cache.get(("eng", k, N))
        if eng is None:
            eng = _cache[("eng", k, N)] = Engine(params_2_2.with_(glwe_dimension=k, polynomial_size=N, pbs_level=1,
                                                                  name=f"glwe_mult_{N}_{k}"), 0)
        rlk = rng.integers(0, 1 << 64, (k * (k + 1) // 2, L, (k + 1) * N), dtype=U64)
        lhs, rhs = _rows(k, N, rng)
        _cache[key] = dict(eng=eng, rlk=rlk, lhs=lhs, rhs=rhs, B=B, L=L, exp={})
    c = _cache[key]
    c["eng"].upload_relinearization_key(c["rlk"], B, L)  # engines are shared between decompositions
    return c


def _expected(orc, c, k, N, log_p):
    if log_p not in c["exp"]:
        c["exp"][log_p] = R.glwe_mult(orc, c["lhs"], c["rhs"], c["rlk"], k, N, c["B"], c["L"], log_p)
    return c["exp"][log_p]


def _check_all_forms(orc, c, k, N, log_p):
    eng, lhs, rhs = c["eng"], c["lhs"], c["rhs"]
    exp = _expected(orc, c, k, N, log_p)
    exp_lwe = R.sample_extract(exp, k, N)
    got = eng.glwe_mult(lhs, rhs, log_p)
    assert got.shape == (COUNT, (k + 1) * N) and np.array_equal(got, exp)
    got = eng.glwe_mult(lhs, rhs, log_p, extract=True)
    assert got.shape == (COUNT, k * N + 1) and np.array_equal(got, exp_lwe)
    for row in (0, 2):  # count 1: a random pair, and all ones times all ones
        assert np.array_equal(eng.glwe_mult(lhs[row], rhs[row], log_p), exp[row:row + 1])
        assert np.array_equal(eng.glwe_mult(lhs[row], rhs[row], log_p, extract=True), exp_lwe[row:row + 1])


@pytest.mark.parametrize("log_p", [0, 2, 4, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_glwe_mult_bit_exact(orc, params_2_2, shape, log_p):
    k, N = shape
    c = _case(params_2_2, k, N, 6, 4)
    _check_all_forms(orc, c, k, N, log_p)
    assert not c["eng"].glwe_mult(c["lhs"][1], c["rhs"][1], log_p).any()  # lhs = 0: every product and digit is 0


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_glwe_mult_other_decompositions(orc, params_2_2, shape):
    k, N = shape
    B, L = OTHER_DECOMPOSITIONS[shape]
    c = _case(params_2_2, k, N, B, L)
    d = R.decompose(R.tensor_product(orc, c["lhs"][:8], c["rhs"][:8], k, N, 4)[1], B, L)
    assert d.max() == 1 << (B - 1)  # the rows do reach the largest digit
    _check_all_forms(orc, c, k, N, 4)


def test_host_form_chunks_a_large_batch(orc, params_2_2):
    """4100 pairs cross the host-pointer form's 4096-pair chunk: the 67 reference pairs repeated."""
    k, N = 2, 512
    c = _case(params_2_2, k, N, 6, 4)
    exp = _expected(orc, c, k, N, 4)
    reps = -(-4100 // COUNT)
    lhs, rhs = (np.tile(x, (reps, 1))[:4100] for x in (c["lhs"], c["rhs"]))
    assert np.array_equal(c["eng"].glwe_mult(lhs, rhs, 4, extract=True),
                          np.tile(R.sample_extract(exp, k, N), (reps, 1))[:4100])


def test_kernel_timer_names(orc, params_2_2):
    c = _case(params_2_2, 2, 512, 6, 4)
    eng = c["eng"]
    eng.kernel_timing(1)
    eng.glwe_mult(c["lhs"][:3], c["rhs"][:3], 4)
    ran = eng.kernel_times()
    eng.kernel_timing(0)
    assert set(ran) == {"glwe_tensor", "glwe_relin"} and all(v[1] == 1 for v in ran.values()), ran


def test_refusals(orc, params_2_2):
    import torch

    from tfhe_mi355 import Engine, EngineError, _lib
    from tfhe_mi355.parameters import PARAM_MESSAGE_1_CARRY_4_KS_PBS

    k, N = 2, 512
    c = _case(params_2_2, k, N, 6, 4)
    eng, lhs, rhs = c["eng"], c["lhs"][:3], c["rhs"][:3]
    for log_p in (3, 63, 65, 66):
        with pytest.raises(EngineError, match="log_p"):
            eng.glwe_mult(lhs, rhs, log_p)
    assert eng.glwe_mult(lhs[:0], rhs[:0], 4).shape == (0, (k + 1) * N)  # count 0: no launch, no error
    with pytest.raises(EngineError, match="expected"):
        eng.upload_relinearization_key(c["rlk"].ravel()[:-1], 6, 4)
    with pytest.raises(EngineError, match="expected"):
        eng.upload_relinearization_key(c["rlk"], 6, 3)
    for B, L in ((0, 4), (32, 1), (8, 8), (6, 0)):
        with pytest.raises(EngineError, match="decomposition"):
            eng.upload_relinearization_key(c["rlk"], B, L)
    eng.upload_relinearization_key(c["rlk"], 6, 4)  # a refused upload leaves the engine usable
    # device-pointer form: out on top of an input, short or missing scratch
    need = eng.glwe_mult_scratch_bytes(3)
    assert need >= 3 * (k * (k + 1) // 2) * N * 8
    d_l, d_r = _dev(lhs), _dev(rhs)
    d_out = _dev(np.zeros((3, (k + 1) * N), dtype=U64))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(EngineError, match="overlaps"):
        _lib.call("tfhe_mi355_glwe_mult_async", eng._h, d_l.data_ptr(), d_r.data_ptr(), 4, 0, d_r.data_ptr(), 3,
                  scratch.data_ptr(), need, stream)
    for ptr, nbytes in ((None, 0), (None, need), (scratch.data_ptr(), need - 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_glwe_mult_async", eng._h, d_l.data_ptr(), d_r.data_ptr(), 4, 0, d_out.data_ptr(), 3,
                      ptr, nbytes, stream)
    with pytest.raises(EngineError, match="overlaps"):
        both = np.concatenate([lhs, rhs])
        _lib.call("tfhe_mi355_glwe_mult", eng._h, both[:3].ctypes.data_as(_lib.u64p), both[3:].ctypes.data_as(_lib.u64p),
                  4, 0, both[2:].ctypes.data_as(_lib.u64p), 3)
    # no key: every call and both scratch queries say so
    fresh = Engine(eng.params, 0)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.glwe_mult(lhs, rhs, 4)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.glwe_mult_scratch_bytes(3)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.lwe_mult_scratch_bytes(3)
    fresh.upload_relinearization_key(c["rlk"], 6, 4)
    with pytest.raises(EngineError, match="packing keyswitching key not uploaded"):
        fresh.lwe_mult(lhs[:, :k * N + 1], rhs[:, :k * N + 1], 4)
    with pytest.raises(EngineError, match="packing keyswitching key not uploaded"):
        fresh.lwe_mult_scratch_bytes(3)
    fresh.close()
    # a shape outside the accepted set
    big = Engine(PARAM_MESSAGE_1_CARRY_4_KS_PBS, 0)  # k = 1, N = 4096
    with pytest.raises(EngineError, match="N must be a power of two in"):
        big.upload_relinearization_key(np.zeros((1, 4, 2 * 4096), dtype=U64), 6, 4)
    with pytest.raises(EngineError, match="N must be a power of two in"):
        big.glwe_mult(np.zeros((1, 2 * 4096), dtype=U64), np.zeros((1, 2 * 4096), dtype=U64), 4)
    with pytest.raises(EngineError, match="N must be a power of two in"):
        big.glwe_mult_scratch_bytes(1)
    big.close()


def test_async_forms_with_exact_scratch_on_a_side_stream(orc, params_2_2):
    """glwe_mult_async and lwe_mult_async with the caller's scratch of exactly the queried size, on a
    stream that is not the default one, against the host forms' reference."""
    import torch

    k, N = 5, 256
    c = _case(params_2_2, k, N, 6, 4)
    eng, exp = c["eng"], _expected(orc, c, k, N, 4)
    side = torch.cuda.Stream()
    d_l, d_r = _dev(c["lhs"]), _dev(c["rhs"])
    torch.cuda.synchronize()
    for extract, want in ((False, exp), (True, R.sample_extract(exp, k, N))):
        d_out = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
        scratch = torch.empty(eng.glwe_mult_scratch_bytes(COUNT), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.glwe_mult_async(d_l, d_r, 4, extract, d_out, COUNT, stream=side, d_scratch=scratch)
        side.synchronize()
        assert np.array_equal(_host(d_out), want)
    m = _lwe_case(orc)
    eng = m["eng"]
    d_out = torch.zeros(m["exp"].shape, dtype=torch.int64, device="cuda")
    scratch = torch.empty(eng.lwe_mult_scratch_bytes(COUNT), dtype=torch.uint8, device="cuda")
    d_l, d_r = _dev(m["lhs"]), _dev(m["rhs"])
    torch.cuda.synchronize()
    eng.lwe_mult_async(d_l, d_r, m["log_p"], d_out, COUNT, stream=side, d_scratch=scratch)
    side.synchronize()
    assert np.array_equal(_host(d_out), m["exp"])


# ---- lwe_mult on a real key ---------------------------------------------------------------------------------
def _lwe_case(orc):
    """The SHA3-shaped test set: client keys, both gadget keys uploaded, 67 pairs (the first 16 encrypt every
    message pair of Z_4, the others are random words) and the reference's output."""
    if "lwe" not in _cache:
        from tfhe_mi355 import Engine, client

        P = R.mult_sets()["sha3"]
        k, N, B, L = P.glwe_dimension, P.polynomial_size, P.ks_base_log, P.ks_level
        sk = client.gen_binary_key(21, 2, k * N)
        pksk = client.gen_packing_keyswitch_key(22, sk, sk, k, N, B, L, P.glwe_modular_std_dev)
        rlk = client.gen_relinearization_key(23, sk, k, N, B, L, P.glwe_modular_std_dev)
        rng = np.random.default_rng(24)
        lhs, rhs = rng.integers(0, 1 << 64, (2, COUNT, k * N + 1), dtype=U64)
        pairs = [(a, b) for a in range(4) for b in range(4)]
        lhs[:16] = client.lwe_encrypt(25, sk, np.array([a << 62 for a, _ in pairs], dtype=U64), P.glwe_modular_std_dev)
        rhs[:16] = client.lwe_encrypt(26, sk, np.array([b << 62 for _, b in pairs], dtype=U64), P.glwe_modular_std_dev)
        log_p = 2  # p = 4
        exp = R.lwe_mult(orc, lhs, rhs, pksk, (B, L), rlk, (B, L), k, N, log_p)
        _cache["lwe"] = dict(P=P, sk=sk, pksk=pksk, rlk=rlk, lhs=lhs, rhs=rhs, exp=exp, pairs=pairs, log_p=log_p)
        eng = Engine(P, 0)
        eng.upload_packing_keyswitch_key(pksk, B, L)
        eng.upload_relinearization_key(rlk, B, L)
        _cache["lwe"]["eng"] = eng
    return _cache["lwe"]


def test_lwe_mult_equals_reference_chain(orc):
    from tfhe_mi355 import client

    m = _lwe_case(orc)
    eng = m["eng"]
    eng.kernel_timing(1)
    got = eng.lwe_mult(m["lhs"], m["rhs"], m["log_p"])
    ran = eng.kernel_times()
    eng.kernel_timing(0)
    assert np.array_equal(got, m["exp"])
    # ONE packing-keyswitch launch over the 2 x 67 rows, then the product's two kernels
    assert {n: v[1] for n, v in ran.items()} == {"packing_keyswitch": 1, "glwe_tensor": 1, "glwe_relin": 1}, ran
    assert np.array_equal(eng.lwe_mult(m["lhs"][5], m["rhs"][5], m["log_p"]), m["exp"][5:6])
    phases = client.lwe_decrypt(m["sk"], got[:16])
    dec = ((phases + U64(1 << 61)) >> U64(62)).astype(np.int64) % 4
    assert dec.tolist() == [a * b % 4 for a, b in m["pairs"]]


def test_two_shards_on_one_device_match_a_single_device(orc, params_2_2):
    from tfhe_mi355 import Engine

    k, N = 2, 512
    c = _case(params_2_2, k, N, 6, 4)
    exp = _expected(orc, c, k, N, 4)
    multi = Engine(c["eng"].params, devices=[0, 0])
    assert multi.multi_device
    multi.upload_relinearization_key(c["rlk"], 6, 4)  # once: it reaches both shards
    assert np.array_equal(multi.glwe_mult(c["lhs"], c["rhs"], 4), exp)
    assert np.array_equal(multi.glwe_mult(c["lhs"], c["rhs"], 4, extract=True), R.sample_extract(exp, k, N))
    multi.close()
    m = _lwe_case(orc)
    P = m["P"]
    multi = Engine(P, devices=[0, 0])
    multi.upload_packing_keyswitch_key(m["pksk"], P.ks_base_log, P.ks_level)
    multi.upload_relinearization_key(m["rlk"], P.ks_base_log, P.ks_level)
    assert np.array_equal(multi.lwe_mult(m["lhs"], m["rhs"], m["log_p"]), m["exp"])
    multi.close()


# ---- gadget.ServerKey on the GPU against the same chain on the CPU reference engine ----------------------------
def _server_keys(name):
    if ("sk", name) not in _cache:
        from tfhe_mi355 import gadget

        P = R.mult_sets()[name]
        ck = gadget.ClientKey(P, seed=5)
        _cache[("sk", name)] = (ck, gadget.ServerKey(ck), gadget.ServerKey(ck, engine=R.RefEngine(P)))
    return _cache[("sk", name)]


def test_server_key_lwe_mult_matches_reference_engine(orc):
    from tfhe_mi355.gadget import Encoding

    ck, gpu, ref = _server_keys("sha3")
    enc = Encoding.new_trivial_wopbs(4)
    pairs = [(a, b) for a in range(4) for b in range(4)]
    lhs = ck.encrypt_arithmetic_many([a for a, _ in pairs], enc)
    rhs = ck.encrypt_arithmetic_many([b for _, b in pairs], enc)
    got, want = gpu.lwe_mult_batch(lhs, rhs, enc), ref.lwe_mult_batch(lhs, rhs, enc)
    assert all(np.array_equal(g.ct, w.ct) and g.encoding == w.encoding == enc for g, w in zip(got, want))
    assert ck.decrypt_many(got) == [a * b % 4 for a, b in pairs]


@pytest.mark.parametrize("fname", ["x+1", "3x^2+2"])
def test_server_key_woppbs_lut_matches_reference_engine(orc, fname):
    from tfhe_mi355.gadget import Encoding

    f = {"x+1": lambda x: (x + 1) % 4, "3x^2+2": lambda x: (3 * x * x + 2) % 4}[fname]
    ck, gpu, ref = _server_keys("aes23")
    enc = Encoding.new_trivial_wopbs(4)
    cts = ck.encrypt_arithmetic_many([0, 1, 2, 3], enc)
    got, want = gpu.woppbs_lut_batch(cts, enc, f), ref.woppbs_lut_batch(cts, enc, f)
    assert all(np.array_equal(g.ct, w.ct) and g.encoding == w.encoding == enc for g, w in zip(got, want))
    assert ck.decrypt_many(got) == [R.woppbs_lut_clear(x, enc, enc, f) for x in range(4)]
