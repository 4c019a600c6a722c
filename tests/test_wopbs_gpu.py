"""The bootstrapped half of WoP-PBS on the GPU (csrc/pfpks.hip, the WoP glue of csrc/lwe_ops.hip and
the launch structure of csrc/capi_wopbs.cpp), bit-exact (np.array_equal) against the CPU reference of
tests/wopbs_reference.py, which is built from the oracle (tests/test_wopbs.py checks that reference).

pfpks shapes (N, k, base_log, level), random u64 keys (exactness needs no valid key): (2048, 1, 15, 2)
the WoP 2_2 / 1_1 shape and (512, 3, 9, 3) WoP 1_2, both int8-MFMA; (1024, 2, 24, 2) and (256, 5, 31, 2)
the 64-bit kernel (digits wider than 16 bits; the digit +2^30); (512, 1, 7, 6) the deepest level loop;
(512, 1, 17, 3) the 64-bit kernel with a level count that does not divide its 128-row LDS chunk.
"""
import ctypes

import numpy as np
import pytest

from ggsw_reference import Ref, lut_value, vp_lut
from wopbs_reference import decrypt_case, pfpks, pfpksk_shape, wop_keys, wop_ref_for

pytestmark = pytest.mark.gpu

U64 = np.uint64
PFPKS_SHAPES = [(2048, 1, 15, 2), (512, 3, 9, 3), (1024, 2, 24, 2), (256, 5, 31, 2), (512, 1, 7, 6), (512, 1, 17, 3)]
SMALLEST = (512, 1, 7, 6)
_cache = {}


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _sync():
    import torch

    torch.cuda.current_stream().synchronize()


# ---- pfpks ------------------------------------------------------------------------------------------
def _pfpks_rows(N, k, B, L, count, rng):
    """all zero; only the body nonzero; every word 1 << 63; every word all ones (the rounding overflow
    wraps to 0); word i with the digit +2^(B-1) at level 1 + i % L (its field is 2^(B-1), the fields
    around it zero); random -- then random rows up to `count`."""
    w = k * N + 1
    x = rng.integers(0, 1 << 64, (max(count, 6), w), dtype=U64)
    x[0] = 0
    x[1] = 0
    x[1, -1] = rng.integers(1, 1 << 64, dtype=U64)
    x[2] = U64(1 << 63)
    x[3] = ~U64(0)
    x[4] = np.array([1 << (64 - B * (1 + i % L) + B - 1) for i in range(w)], dtype=U64)
    return x


def _pfpks_case(orc, params_2_2, shape):
    """engine with a random key of the shape uploaded, the rows and their reference output, once."""
    if ("pfpks", shape) in _cache:
        return _cache[("pfpks", shape)]
    from tfhe_mi355 import Engine

    N, k, B, L = shape
    rng = np.random.default_rng(N + 3 * k + B)
    key = rng.integers(0, 1 << 64, int(np.prod(pfpksk_shape(k, N, L))), dtype=U64)
    eng = Engine(params_2_2.with_(glwe_dimension=k, polynomial_size=N, pbs_level=1, name=f"pfpks_{N}_{k}"), 0)
    eng.upload_pfpksk_list(key, B, L)
    x = _pfpks_rows(N, k, B, L, 67 if (N, k) == SMALLEST[:2] else 6, rng)
    d = Ref(orc, k, N, B, L).digits(x[4]).astype(np.int64)
    assert all(d[lvl].max() == 1 << (B - 1) for lvl in range(L))  # the row does hold +2^(B-1) at every level
    exp = pfpks(orc, key, k, N, B, L, x)
    _cache[("pfpks", shape)] = dict(eng=eng, key=key, x=x, exp=exp)
    return _cache[("pfpks", shape)]


@pytest.mark.parametrize("shape", PFPKS_SHAPES, ids=str)
def test_pfpks_bit_exact(orc, params_2_2, shape):
    N, k, B, L = shape
    c = _pfpks_case(orc, params_2_2, shape)
    eng = c["eng"]
    eng.kernel_timing(1)
    got = eng.private_functional_packing_keyswitch(c["x"][:6])
    ran = set(eng.kernel_times())
    eng.kernel_timing(0)
    assert got.shape == (6, k + 1, (k + 1) * N)
    assert np.array_equal(got, c["exp"][:6])
    assert not got[0].any()  # the all-zero row gives exactly zero
    assert ran == ({"pfpks_mfma"} if B <= 15 else {"pfpks_generic"}), ran
    one = eng.private_functional_packing_keyswitch(c["x"][5])  # count 1: the random row
    assert np.array_equal(one, c["exp"][5:6])
    if (N, k) == SMALLEST[:2]:  # 67 rows cross a 64-row tile, in both kernels
        assert np.array_equal(eng.private_functional_packing_keyswitch(c["x"]), c["exp"])


@pytest.mark.parametrize("shape", [(2048, 1, 15, 2), (256, 5, 31, 2)], ids=str)
def test_pfpks_async_equals_host_form(orc, params_2_2, shape):
    N, k, B, L = shape
    c = _pfpks_case(orc, params_2_2, shape)
    d_out = _dev(np.zeros((6, k + 1, (k + 1) * N), dtype=U64))
    c["eng"].private_functional_packing_keyswitch_async(_dev(c["x"][:6]), d_out, 6)
    _sync()
    assert np.array_equal(_host(d_out), c["exp"][:6])


def test_pfpks_errors(orc, params_2_2):
    import torch

    from tfhe_mi355 import Engine, EngineError, _lib

    N, k, B, L = PFPKS_SHAPES[0]
    c = _pfpks_case(orc, params_2_2, PFPKS_SHAPES[0])
    eng = c["eng"]
    need = eng.pfpks_scratch_bytes(6)
    assert need >= 2 * 64 * (k * N + 1) * L  # the two int8 digit planes of one 64-row tile
    d_in, d_out = _dev(c["x"][:6]), _dev(np.zeros((6, k + 1, (k + 1) * N), dtype=U64))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for ptr, nbytes in ((None, 0), (None, need), (scratch.data_ptr(), need - 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_private_functional_packing_keyswitch_async", eng._h, d_in.data_ptr(),
                      d_out.data_ptr(), 6, ptr, nbytes, stream)
    fresh = Engine(eng.params, 0)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.private_functional_packing_keyswitch(c["x"][:1])
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.pfpks_scratch_bytes(1)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.circuit_bootstrap_scratch_bytes(3, 1)
    with pytest.raises(EngineError, match="not uploaded"):
        fresh.circuit_bootstrap(np.zeros((1, fresh.n + 1), dtype=U64), 63, 5, 3)
    for bl, lv in ((32, 1), (0, 2), (16, 4), (15, 0)):
        with pytest.raises(EngineError, match="invalid pfpks decomposition"):
            fresh.upload_pfpksk_list(c["key"], bl, lv)
    with pytest.raises(EngineError, match="words, expected"):
        fresh.upload_pfpksk_list(c["key"][:-1], B, L)
    fresh.close()


# ---- bit extraction, circuit bootstrap, composition: two WoP settings with real keys, n cut to 96 -------
def _wop_params(name):
    from tfhe_mi355 import parameters as P

    return {"2_2": P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS, "1_2": P.WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS}[name].with_(
        lwe_dimension=96)


def _wop_case(orc, name, devices=None):
    key = ("wop", name, devices)
    if key in _cache:
        return _cache[key]
    from tfhe_mi355 import Engine, client
    from tfhe_mi355.shortint import ClientKey

    p = _wop_params(name)
    if ("wopkeys", name) not in _cache:
        cks = ClientKey(p, 40 + len(name))
        _cache[("wopkeys", name)] = (cks,) + wop_keys(cks)
    cks, bsk, ksk, pfpksk = _cache[("wopkeys", name)]
    eng = Engine(p, 0) if devices is None else Engine(p, devices=list(devices))
    eng.upload_bootstrap_key(bsk)
    eng.upload_keyswitch_key(ksk)
    eng.upload_pfpksk_list(pfpksk, p.pfks_base_log, p.pfks_level)
    rng = np.random.default_rng(p.polynomial_size)
    c = dict(p=p, cks=cks, eng=eng, ref=wop_ref_for(orc, p, bsk, ksk, pfpksk), pfpksk=pfpksk,
             small=rng.integers(0, 1 << 64, (3, p.lwe_dimension + 1), dtype=U64),
             big=rng.integers(0, 1 << 64, (3, p.big_lwe_dimension + 1), dtype=U64))
    # index bits at q/2 under the small key, most significant first
    c["idx4"] = [5, 10, 15]
    c["idx12"] = [0xA35, 0x0FC, 0x7FF]
    for nb, idx in ((4, c["idx4"]), (12, c["idx12"])):
        bits = np.array([[(i >> (nb - 1 - b)) & 1 for b in range(nb)] for i in idx], dtype=U64)
        c[f"bits{nb}"] = client.lwe_encrypt(50 + nb, cks.small_lwe_secret_key, bits.ravel() << U64(63),
                                            p.lwe_modular_std_dev).reshape(len(idx), nb, -1)
    _cache[key] = c
    return c


def _ref(c, what, fn):
    """reference results, once per case (shared by the tests that compare against them)."""
    if what not in c:
        c[what] = fn()
    return c[what]


@pytest.mark.parametrize("name", ["2_2", "1_2"])
@pytest.mark.parametrize("delta_log", [63, 60])
def test_circuit_bootstrap_bit_exact(orc, name, delta_log):
    c = _wop_case(orc, name)
    p = c["p"]
    exp = _ref(c, ("cbs", delta_log), lambda: c["ref"].circuit_bootstrap(c["small"], delta_log, p.cbs_base_log, p.cbs_level))
    got = c["eng"].circuit_bootstrap(c["small"], delta_log, p.cbs_base_log, p.cbs_level)
    assert got.shape == (3, p.cbs_level, p.glwe_dimension + 1, (p.glwe_dimension + 1) * p.polynomial_size)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("name", ["2_2", "1_2"])
@pytest.mark.parametrize("delta_log,nbits", [(60, 4), (60, 1), (61, 3)])
def test_extract_bits_bit_exact(orc, name, delta_log, nbits):
    """nbits 1 is the keyswitch alone; (61, 3) reaches delta_log + nbits = 64."""
    c = _wop_case(orc, name)
    exp = _ref(c, ("eb", delta_log, nbits), lambda: c["ref"].extract_bits(c["big"], delta_log, nbits))
    got = c["eng"].extract_bits(c["big"], delta_log, nbits)
    assert got.shape == (3, nbits, c["p"].lwe_dimension + 1)
    assert np.array_equal(got, exp)


def _composed_inputs(c, nbits, npoly, nout, lut_count):
    p = c["p"]
    nr = nbits - (npoly.bit_length() - 1)
    luts = np.stack([np.stack([vp_lut(npoly, p.polynomial_size, nr, 1 << 60, shift=3 * l + o) for o in range(nout)])
                     for l in range(lut_count)])
    idx = np.array([1, 0, 1], dtype=np.uint32)[:len(c[f"bits{nbits}"])] if lut_count > 1 else None
    return luts, idx


@pytest.mark.parametrize("name,nbits,npoly,nout,lut_count", [
    ("2_2", 4, 1, 1, 1),     # rotation only
    ("2_2", 12, 2, 2, 2),    # one tree bit, 11 rotation bits, two outputs, two LUTs through lut_indexes
    ("1_2", 4, 1, 1, 1),
    ("1_2", 12, 8, 2, 2),    # N = 512 rotates by at most 9 bits: three tree bits
])
def test_composed_call_bit_exact(orc, name, nbits, npoly, nout, lut_count):
    c = _wop_case(orc, name)
    p = c["p"]
    luts, idx = _composed_inputs(c, nbits, npoly, nout, lut_count)
    bits = c[f"bits{nbits}"]
    exp = _ref(c, ("cbvp", nbits, npoly, nout), lambda: c["ref"].circuit_bootstrap_vertical_packing(
        bits, p.cbs_base_log, p.cbs_level, luts, idx))
    got = c["eng"].circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, luts, idx)
    assert got.shape == (3, nout, p.big_lwe_dimension + 1)
    assert np.array_equal(got, exp)
    # and the looked-up values decrypt: output o of item i is lut_value(index + shift)
    pts = orc.lwe_decrypt(c["cks"].large_lwe_secret_key, got.reshape(-1, got.shape[-1])).reshape(3, nout)
    for i, index in enumerate(c[f"idx{nbits}"]):
        for o in range(nout):
            shift = 3 * (0 if idx is None else int(idx[i])) + o
            assert int((int(pts[i, o]) + (1 << 59)) >> 60) % 16 == lut_value(index + shift)


def test_async_forms_equal_host_forms(orc):
    c = _wop_case(orc, "2_2")
    p, eng = c["p"], c["eng"]
    k1, glwe = p.glwe_dimension + 1, (p.glwe_dimension + 1) * p.polynomial_size
    d_bits = _dev(np.zeros((3, 4, p.lwe_dimension + 1), dtype=U64))
    eng.extract_bits_async(_dev(c["big"]), 60, 4, d_bits, 3)
    _sync()
    assert np.array_equal(_host(d_bits), eng.extract_bits(c["big"], 60, 4))
    d_ggsw = _dev(np.zeros((3, p.cbs_level, k1, glwe), dtype=U64))
    eng.circuit_bootstrap_async(_dev(c["small"]), 60, p.cbs_base_log, p.cbs_level, d_ggsw, 3)
    _sync()
    assert np.array_equal(_host(d_ggsw), eng.circuit_bootstrap(c["small"], 60, p.cbs_base_log, p.cbs_level))
    luts, idx = _composed_inputs(c, 12, 2, 2, 2)
    d_out = _dev(np.zeros((3, 2, p.big_lwe_dimension + 1), dtype=U64))
    eng.circuit_bootstrap_vertical_packing_async(_dev(c["bits12"]), 12, p.cbs_base_log, p.cbs_level, _dev(luts), 2, 2, 2,
                                                 3, d_out, _dev(idx.view(np.int32)))
    _sync()
    assert np.array_equal(_host(d_out), eng.circuit_bootstrap_vertical_packing(c["bits12"], p.cbs_base_log, p.cbs_level,
                                                                              luts, idx))


def test_wop_scratch_and_argument_errors(orc):
    import torch

    from tfhe_mi355 import EngineError, _lib

    c = _wop_case(orc, "2_2")
    p, eng = c["p"], c["eng"]
    stream = torch.cuda.current_stream().cuda_stream
    d_big, d_small = _dev(c["big"]), _dev(c["small"])
    d_bits = _dev(np.zeros((3, 4, p.lwe_dimension + 1), dtype=U64))
    d_ggsw = _dev(np.zeros((3, eng.ggsw_words(p.cbs_level)), dtype=U64))
    need_eb, need_cb = eng.extract_bits_scratch_bytes(3), eng.circuit_bootstrap_scratch_bytes(p.cbs_level, 3)
    assert need_eb >= 3 * 3 * (p.big_lwe_dimension + 1) * 8 and need_cb >= 9 * (p.big_lwe_dimension + 1) * 8
    scratch = torch.empty(max(need_eb, need_cb), dtype=torch.uint8, device="cuda")
    for ptr, cut in ((None, 0), (scratch.data_ptr(), 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_extract_bits_async", eng._h, d_big.data_ptr(), 60, 4, d_bits.data_ptr(), 3, ptr,
                      need_eb - cut if ptr else 0, stream)
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_circuit_bootstrap_async", eng._h, d_small.data_ptr(), 60, p.cbs_base_log, p.cbs_level,
                      d_ggsw.data_ptr(), 3, ptr, need_cb - cut if ptr else 0, stream)
    need_vp = eng.circuit_bootstrap_vertical_packing_scratch_bytes(4, p.cbs_level, 1, 1, 1, 3)
    d_out, d_lut = _dev(np.zeros((3, p.big_lwe_dimension + 1), dtype=U64)), _dev(np.zeros(p.polynomial_size, dtype=U64))
    with pytest.raises(EngineError, match="scratch too small"):
        _lib.call("tfhe_mi355_circuit_bootstrap_vertical_packing_async", eng._h, _dev(c["bits4"]).data_ptr(), 4,
                  p.cbs_base_log, p.cbs_level, d_lut.data_ptr(), 1, 1, 1, None, 3, d_out.data_ptr(),
                  scratch.data_ptr(), need_vp - 256, stream)
    out = np.zeros((3, 4, p.lwe_dimension + 1), dtype=U64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for delta_log, nbits, msg in ((61, 4, "exceeds the 64 bits"), (60, 0, "no bit"), (0, 2, "delta_log 0")):
        with pytest.raises(EngineError, match=msg):
            _lib.call("tfhe_mi355_extract_bits", eng._h, c["big"].ctypes.data_as(u64p), delta_log, nbits,
                      out.ctypes.data_as(u64p), 3)
    with pytest.raises(ValueError, match="out of range"):
        eng.extract_bits(c["big"], 61, 4)
    with pytest.raises(EngineError, match="base_log \\* level <= 32"):
        eng.circuit_bootstrap(c["small"], 60, 11, 3)
    with pytest.raises(EngineError, match="not a power of two"):
        eng.circuit_bootstrap_vertical_packing(c["bits4"], p.cbs_base_log, p.cbs_level,
                                               np.zeros((1, 1, 3, p.polynomial_size), dtype=U64))


def test_two_shards_on_one_device_match_a_single_device(orc):
    c = _wop_case(orc, "2_2")
    m = _wop_case(orc, "2_2", devices=(0, 0))
    p, eng, multi = c["p"], c["eng"], m["eng"]
    assert multi.multi_device
    x = np.concatenate([c["big"], c["big"][::-1]])
    assert np.array_equal(multi.private_functional_packing_keyswitch(x), eng.private_functional_packing_keyswitch(x))
    assert np.array_equal(multi.extract_bits(c["big"], 60, 4), eng.extract_bits(c["big"], 60, 4))
    assert np.array_equal(multi.circuit_bootstrap(c["small"], 60, p.cbs_base_log, p.cbs_level),
                          eng.circuit_bootstrap(c["small"], 60, p.cbs_base_log, p.cbs_level))
    luts, idx = _composed_inputs(c, 12, 2, 2, 2)
    assert np.array_equal(multi.circuit_bootstrap_vertical_packing(c["bits12"], p.cbs_base_log, p.cbs_level, luts, idx),
                          eng.circuit_bootstrap_vertical_packing(c["bits12"], p.cbs_base_log, p.cbs_level, luts, idx))
    multi.close()
    del _cache[("wop", "2_2", (0, 0))]


def test_core_crypto_mirrors(orc):
    from tfhe_mi355 import core_crypto as cc

    c = _wop_case(orc, "2_2")
    p, eng = c["p"], c["eng"]
    k1, N = p.glwe_dimension + 1, p.polynomial_size
    keys = cc.LwePrivateFunctionalPackingKeyswitchKeyList(c["pfpksk"], p.big_lwe_dimension, k1, N, p.pfks_base_log,
                                                          p.pfks_level, eng)
    bsk, ksk = cc.FourierLweBootstrapKey(eng), cc.LweKeyswitchKey(eng)
    glwe = np.zeros(k1 * N, dtype=U64)
    want = eng.private_functional_packing_keyswitch(c["big"][0])
    for g in range(k1):
        cc.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(keys, g, glwe, c["big"][0])
        assert np.array_equal(glwe, want[0, g])
    bits = np.zeros((4, p.lwe_dimension + 1), dtype=U64)
    cc.extract_bits_from_lwe_ciphertext(c["big"][1], bits, bsk, ksk, 60, 4)
    assert np.array_equal(bits, eng.extract_bits(c["big"][1], 60, 4)[0])
    ggsw = cc.GgswCiphertextList(np.zeros(2 * eng.ggsw_words(p.cbs_level), dtype=U64), k1, N, p.cbs_base_log, p.cbs_level)
    cc.circuit_bootstrap_boolean(bsk, c["small"][:2], ggsw, 60, keys)
    assert np.array_equal(ggsw.data.ravel(), eng.circuit_bootstrap(c["small"][:2], 60, p.cbs_base_log, p.cbs_level).ravel())
    luts, _ = _composed_inputs(c, 12, 2, 2, 1)
    out = np.zeros((2, p.big_lwe_dimension + 1), dtype=U64)
    cc.circuit_bootstrap_boolean_vertical_packing(luts[0].reshape(4, N), bsk, out, c["bits12"][0], keys, p.cbs_level,
                                                  p.cbs_base_log)
    assert np.array_equal(out, eng.circuit_bootstrap_vertical_packing(c["bits12"][:1], p.cbs_base_log, p.cbs_level,
                                                                      luts)[0])
    with pytest.raises(ValueError, match="Mismatched input LweDimension"):
        cc.private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(keys, 0, glwe, c["big"][0][:-1])
    with pytest.raises(ValueError, match="do not divide"):
        cc.circuit_bootstrap_boolean_vertical_packing(luts[0].reshape(4, N), bsk, np.zeros((3, out.shape[1]), dtype=U64),
                                                      c["bits12"][0], keys, p.cbs_level, p.cbs_base_log)


# ---- decryption with the real WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS keys ----------------------------------
def _real_keys(orc):
    if "real" not in _cache:
        from tfhe_mi355.shortint import ServerKey, WopbsKey

        d = decrypt_case(orc)
        sks = ServerKey(d["cks"], bsk=d["bsk"], ksk=d["ksk"])
        _cache["real"] = (d, sks, WopbsKey(sks, d["P"], d["pfpksk"]))
    return _cache["real"]


def test_all_16_messages_without_padding_decrypt(orc):
    d, sks, wk = _real_keys(orc)
    cks = d["cks"]
    lut = wk.generate_lut_without_padding(d["cts_a"][0], lut_value)
    assert np.array_equal(lut, d["lut_a"])
    res = wk.programmable_bootstrapping_without_padding(d["cts_a"], lut)
    assert np.array_equal(np.stack([r.ct for r in res]), d["out_a"][:, 0])
    assert np.array_equal(cks.decrypt_message_and_carry_without_padding_many(res), [lut_value(m % 4) for m in range(16)])
    assert cks.decrypt_without_padding(res[5]) == lut_value(1) % 4


def test_three_blocks_as_one_12_bit_index_decrypt(orc):
    d, sks, wk = _real_keys(orc)
    P, eng = d["P"], wk.engine
    bits = eng.extract_bits(d["x_b"], 60, 4)
    assert np.array_equal(bits, d["bits_b"])
    out = eng.circuit_bootstrap_vertical_packing(bits.reshape(2, 12, -1), P.cbs_base_log, P.cbs_level, d["lut_b"])
    assert np.array_equal(out, d["out_b"])
    pts = orc.lwe_decrypt(d["cks"].large_lwe_secret_key, out[:, 0])
    assert [int((int(v) + (1 << 59)) >> 60) % 16 for v in pts] == [lut_value(i) for i in d["index_b"]]


def test_shortint_wopbs_with_padding(orc):
    """WopbsKey.wopbs on ciphertexts with a padding bit: delta_log 59, the 4 message and carry bits."""
    d, sks, wk = _real_keys(orc)
    cks = d["cks"]
    cts = cks.encrypt_many([0, 1, 2, 3])
    lut = wk.generate_lut(cts[0], lambda x: (x * x + 1) % 4)
    assert int(lut[2]) == ((2 * 2 + 1) % 4) << 59 and not lut[16:].any()
    res = wk.wopbs(cts, lut)
    x = np.stack([c.ct for c in cts])
    exp = d["ref"].circuit_bootstrap_vertical_packing(d["ref"].extract_bits(x, 59, 4), d["P"].cbs_base_log,
                                                      d["P"].cbs_level, lut.reshape(1, 1, 1, -1))
    assert np.array_equal(np.stack([r.ct for r in res]), exp[:, 0])
    assert [cks.decrypt(r) for r in res] == [(m * m + 1) % 4 for m in range(4)]
