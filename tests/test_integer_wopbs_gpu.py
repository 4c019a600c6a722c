"""Integer WoP-PBS on the GPU: the multi-output vertical packing and the rotation chain of
csrc/ggsw_ops.hip (through the composed call and tfhe_mi355_vertical_packing), the keyswitching key
objects (tfhe_mi355_keyswitch_with_key) and integer.WopbsKey on the engine.  Every comparison is
bit-exact (np.array_equal): the engine against tests/wopbs_reference.WopRef / ggsw_reference.Ref, the
default launch structure against TFHE_MI355_VP_STEPWISE=1, the API against the CPU stand-in of
tests/integer_wopbs_cases.py running the same keys.

Sets: WOPBS 2_2 (N = 2048, k = 1, cbs 5 x 3) and WOPBS 1_2 (N = 512, k = 3, cbs 3 x 5) and
PARAM_MESSAGE_2_CARRY_2_KS_PBS with lwe_dimension cut to 96; one end-to-end decryption at the real sets.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import integer_wopbs_cases as cases
from ggsw_reference import Ref, lut_value, vp_lut
from wopbs_reference import decrypt_case, wop_keys, wop_ref_for

pytestmark = pytest.mark.gpu

U64 = np.uint64
_cache = {}


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _sync():
    import torch

    torch.cuda.current_stream().synchronize()


@contextmanager
def _env(**kv):
    """the library reads TFHE_MI355_VP_STEPWISE and TFHE_MI355_GGSW_GRID at every launch."""
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


# ---- the composed call: outputs as a node dimension, the rotation chain ----------------------------------
def _wop_case(orc, name, devices=None):
    """engine with the real keys of one cut WoP set, the CPU reference on the same keys."""
    key = ("wop", name, devices)
    if key in _cache:
        return _cache[key]
    from tfhe_mi355 import Engine

    cks = cases.client_key(f"wop_{name}", 40 + len(name))
    p = cks.parameters
    if ("keys", name) not in _cache:
        _cache[("keys", name)] = wop_keys(cks)
    bsk, ksk, pfpksk = _cache[("keys", name)]
    eng = Engine(p, 0) if devices is None else Engine(p, devices=list(devices))
    eng.upload_bootstrap_key(bsk)
    eng.upload_keyswitch_key(ksk)
    eng.upload_pfpksk_list(pfpksk, p.pfks_base_log, p.pfks_level)
    if ("ref", name) not in _cache:
        _cache[("ref", name)] = wop_ref_for(orc, p, bsk, ksk, pfpksk)
    _cache[key] = dict(p=p, cks=cks, eng=eng, ref=_cache[("ref", name)])
    return _cache[key]


def _composed(orc, name, nbits, npoly, nout, lut_count):
    """3 items: their index bits under the small key, the LUTs (output o of LUT l looks up
    lut_value(index + 3 l + o)), the reference outputs; once per shape."""
    key = ("composed", name, nbits, npoly, nout, lut_count)
    if key in _cache:
        return _cache[key]
    from tfhe_mi355 import client

    c = _wop_case(orc, name)
    p = c["p"]
    top = 1 << nbits
    indices = [top - 1, (top // 3) | 1 if top > 2 else 0, top // 2]
    bits = np.array([[(i >> (nbits - 1 - b)) & 1 for b in range(nbits)] for i in indices], dtype=U64)
    x = client.lwe_encrypt(90 + nbits, c["cks"].small_lwe_secret_key, bits.ravel() << U64(63),
                           p.lwe_modular_std_dev).reshape(3, nbits, -1)
    nr = nbits - (npoly.bit_length() - 1)
    luts = np.stack([np.stack([vp_lut(npoly, p.polynomial_size, nr, 1 << 60, shift=3 * l + o) for o in range(nout)])
                     for l in range(lut_count)])
    idx = np.array([1, 0, 1], dtype=np.uint32) if lut_count > 1 else None
    exp = c["ref"].circuit_bootstrap_vertical_packing(x, p.cbs_base_log, p.cbs_level, luts, idx)
    _cache[key] = dict(indices=indices, bits=x, luts=luts, idx=idx, exp=exp, nr=nr)
    return _cache[key]


COMPOSED = [
    ("2_2", 5, 1, 3, 1),    # the chain starts from a LUT leaf
    ("2_2", 12, 2, 3, 2),   # tree -> chain hand-off, two LUTs through lut_indexes
    ("2_2", 1, 1, 1, 1),    # a chain of one step: first and last
    ("2_2", 3, 8, 2, 1),    # no rotation bit: no chain, the last tree level extracts
    ("1_2", 12, 8, 3, 1),   # 9 = log2 N rotation bits: the step of degree N/2
]


@pytest.mark.parametrize("name,nbits,npoly,nout,lut_count", COMPOSED)
def test_composed_call_multi_output_bit_exact(orc, name, nbits, npoly, nout, lut_count):
    c = _wop_case(orc, name)
    p, eng = c["p"], c["eng"]
    s = _composed(orc, name, nbits, npoly, nout, lut_count)
    got = eng.circuit_bootstrap_vertical_packing(s["bits"], p.cbs_base_log, p.cbs_level, s["luts"], s["idx"])
    assert got.shape == (3, nout, p.big_lwe_dimension + 1)
    assert np.array_equal(got, s["exp"])
    with _env(TFHE_MI355_VP_STEPWISE="1"):
        eng.kernel_timing(1)
        step = eng.circuit_bootstrap_vertical_packing(s["bits"], p.cbs_base_log, p.cbs_level, s["luts"], s["idx"])
        ran = eng.kernel_times()
        eng.kernel_timing(0)
    assert np.array_equal(step, got)
    assert "ggsw_rotate_chain" not in ran and ran.get("ggsw_rotate", (0, 0))[1] == s["nr"]
    # every output decrypts to lut_value(index + shift)
    pts = orc.lwe_decrypt(c["cks"].large_lwe_secret_key, got.reshape(-1, got.shape[-1])).reshape(3, nout)
    for i, index in enumerate(s["indices"]):
        for o in range(nout):
            shift = 3 * (0 if s["idx"] is None else int(s["idx"][i])) + o
            assert int((int(pts[i, o]) + (1 << 59)) >> 60) % 16 == lut_value(index + shift), (i, o)


def test_launch_counts_one_tree_level_one_chain(orc):
    """(12 bits, 2 polynomials, 3 outputs): one CMUX tree launch over count * nout nodes, one chain launch
    for the 11 rotation steps and the extraction, no step-wise rotation launch."""
    c = _wop_case(orc, "2_2")
    p, eng = c["p"], c["eng"]
    s = _composed(orc, "2_2", 12, 2, 3, 2)
    eng.kernel_timing(1)
    got = eng.circuit_bootstrap_vertical_packing(s["bits"], p.cbs_base_log, p.cbs_level, s["luts"], s["idx"])
    ran = eng.kernel_times()
    eng.kernel_timing(0)
    assert np.array_equal(got, s["exp"])
    assert ran["ggsw_cmux_tree"][1] == 1 and ran["ggsw_rotate_chain"][1] == 1, ran
    assert "ggsw_rotate" not in ran, ran
    nr0 = _composed(orc, "2_2", 3, 8, 2, 1)
    eng.kernel_timing(1)
    eng.circuit_bootstrap_vertical_packing(nr0["bits"], p.cbs_base_log, p.cbs_level, nr0["luts"])
    ran = eng.kernel_times()
    eng.kernel_timing(0)
    assert ran["ggsw_cmux_tree"][1] == 3 and "ggsw_rotate_chain" not in ran and "ggsw_rotate" not in ran, ran


@pytest.mark.parametrize("N,k,B,L", [(512, 1, 7, 3), (512, 3, 4, 6), (256, 5, 7, 3)], ids=str)
def test_node_loop_wraps_under_a_one_workgroup_grid(orc, params_2_2, N, k, B, L):
    """TFHE_MI355_GGSW_GRID=1: 9 items over ONE workgroup make the persistent loop of the tree launch, of
    the chain launch and of the step-wise rotation launches wrap: 4 node slots at k = 1 (three passes, the
    last with one node), 2 at k = 3 (five passes, the last with one node), 1 at k = 5 (nine passes).
    No context exists at (N, k) = (256, 1) -- the classic PBS has no instance of that shape and context
    creation refuses it -- so (512, 1) carries the four-slot layout and (256, 5) the N = 256 kernels.
    GGSWs of random bits under a random key, random LUTs."""
    from tfhe_mi355 import Engine, client

    eng = Engine(params_2_2.with_(glwe_dimension=k, polynomial_size=N, pbs_level=1, name=f"wrap_{N}_{k}"), 0)
    rng = np.random.default_rng(N + k)
    nbits, npoly = 4, 2
    sk = client.gen_binary_key(2000 + N + k, 2, k * N)
    g = client.gen_ggsw_list(80 + k, [int(b) for b in rng.integers(0, 2, 9 * nbits)], sk, k, N, B, L,
                             2.94036859086e-16).reshape(9, nbits, -1)
    luts = rng.integers(0, 1 << 64, (2, npoly, N), dtype=U64)
    idx = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1], dtype=np.uint32)
    ref = Ref(orc, k, N, B, L)
    exp = np.stack([ref.vertical_packing(g[i], luts[idx[i]]) for i in range(9)])
    assert np.array_equal(eng.vertical_packing(g, B, L, luts, idx), exp)      # the full grid
    with _env(TFHE_MI355_GGSW_GRID="1"):
        assert np.array_equal(eng.vertical_packing(g, B, L, luts, idx), exp)
        with _env(TFHE_MI355_VP_STEPWISE="1"):
            assert np.array_equal(eng.vertical_packing(g, B, L, luts, idx), exp)
    eng.close()


def test_async_form_scratch_and_two_shards(orc):
    import torch

    from tfhe_mi355 import EngineError, _lib

    c = _wop_case(orc, "2_2")
    p, eng = c["p"], c["eng"]
    s = _composed(orc, "2_2", 12, 2, 3, 2)
    d_bits, d_luts, d_idx = _dev(s["bits"]), _dev(s["luts"]), _dev(s["idx"].view(np.int32))
    d_out = _dev(np.zeros((3, 3, p.big_lwe_dimension + 1), dtype=U64))
    eng.circuit_bootstrap_vertical_packing_async(d_bits, 12, p.cbs_base_log, p.cbs_level, d_luts, 2, 3, 2, 3, d_out, d_idx)
    _sync()
    assert np.array_equal(_host(d_out), s["exp"])
    # the scratch query is the exact need: the GGSW lists, then the larger of the circuit bootstrap's scratch
    # and the two ping-pong lists of count * nout GLWEs each (npoly 2: max(npoly / 2, 1) = max(npoly / 4, 1) = 1)
    need = eng.circuit_bootstrap_vertical_packing_scratch_bytes(12, p.cbs_level, 2, 3, 2, 3)
    glwe_b = (p.glwe_dimension + 1) * p.polynomial_size * 8
    ggsw_b = 3 * 12 * eng.ggsw_words(p.cbs_level) * 8
    rest = max(eng.circuit_bootstrap_scratch_bytes(p.cbs_level, 3 * 12), 2 * 3 * 3 * glwe_b)
    assert need == 2 * ggsw_b + rest                          # standard and Fourier lists are the same size
    assert need == eng.circuit_bootstrap_vertical_packing_scratch_bytes(12, p.cbs_level, 2, 1, 2, 3)  # cbs dominates
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for ptr, nbytes in ((None, 0), (scratch.data_ptr(), need - 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_circuit_bootstrap_vertical_packing_async", eng._h, d_bits.data_ptr(), 12, p.cbs_base_log,
                      p.cbs_level, d_luts.data_ptr(), 2, 3, 2, d_idx.data_ptr(), 3, d_out.data_ptr(), ptr, nbytes, stream)
    # the plain vertical packing's scratch scales as before (one output)
    assert eng.vertical_packing_scratch_bytes(8, 3) == 3 * 4 * glwe_b + 3 * 2 * glwe_b
    m = _wop_case(orc, "2_2", devices=(0, 0))
    assert m["eng"].multi_device
    assert np.array_equal(m["eng"].circuit_bootstrap_vertical_packing(s["bits"], p.cbs_base_log, p.cbs_level, s["luts"],
                                                                     s["idx"]), s["exp"])
    m["eng"].close()
    del _cache[("wop", "2_2", (0, 0))]


# ---- keyswitching keys as objects ----------------------------------------------------------------------------
KS_CASES = [(2048, 2048, 6, 2, True), (1536, 96, 9, 3, False)]   # (in, out, base_log, level, int8 MFMA form)


@pytest.mark.parametrize("in_dim,out_dim,B,L,mfma", KS_CASES, ids=str)
def test_keyswitch_with_key_bit_exact(orc, params_2_2, in_dim, out_dim, B, L, mfma):
    from tfhe_mi355 import Engine

    rng = np.random.default_rng(in_dim + out_dim)
    ksk = rng.integers(0, 1 << 64, in_dim * L * (out_dim + 1), dtype=U64)
    x = rng.integers(0, 1 << 64, (67, in_dim + 1), dtype=U64)
    x[0], x[1], x[2] = 0, U64(1 << 63), ~U64(0)
    exp = orc.keyswitch(ksk, in_dim, out_dim, B, L, x)
    eng = Engine(params_2_2, 0)                     # dimensions no parameter set of the context describes
    key = eng.keyswitch_key(ksk, in_dim, out_dim, B, L)
    assert (eng.keyswitch_with_key_scratch_bytes(key, 67) > 0) == mfma
    eng.kernel_timing(1)
    got = eng.keyswitch_with_key(key, x)
    assert eng.kernel_times()["keyswitch"][1] == 1
    eng.kernel_timing(0)
    assert got.shape == (67, out_dim + 1)
    assert np.array_equal(got, exp)
    assert np.array_equal(eng.keyswitch_with_key(key, x[5]), exp[5:6])
    d_out = _dev(np.full((70, out_dim + 1), 0x5A5A5A5A5A5A5A5A, dtype=U64))
    eng.keyswitch_with_key_async(key, _dev(x), d_out, 67)
    _sync()
    assert np.array_equal(_host(d_out)[:67], exp)
    assert (_host(d_out)[67:] == U64(0x5A5A5A5A5A5A5A5A)).all()
    multi = Engine(params_2_2, devices=[0, 0])
    mkey = multi.keyswitch_key(ksk, in_dim, out_dim, B, L)
    assert np.array_equal(multi.keyswitch_with_key(mkey, x), exp)
    mkey.close()
    multi.close()
    key.close()
    eng.close()


def test_keyswitch_key_errors(orc, params_2_2):
    import torch

    from tfhe_mi355 import Engine, EngineError, _lib

    eng = Engine(params_2_2, 0)
    ksk = np.zeros(64 * 2 * 9, dtype=U64)
    with pytest.raises(EngineError, match="words, expected"):
        eng.keyswitch_key(ksk[:-1], 64, 8, 6, 2)
    for in_dim, out_dim in ((0, 8), (64, 0)):
        with pytest.raises(EngineError, match="zero dimension"):
            eng.keyswitch_key(ksk, in_dim, out_dim, 6, 2)
    for B, L in ((32, 2), (0, 2), (6, 0), (7, 10)):
        with pytest.raises(EngineError, match="decomposition"):
            eng.keyswitch_key(ksk, 64, 8, B, L)
    key = eng.keyswitch_key(ksk, 64, 8, 6, 2)
    need = eng.keyswitch_with_key_scratch_bytes(key, 3)
    assert need > 0
    d_in, d_out = _dev(np.zeros((3, 65), dtype=U64)), _dev(np.zeros((3, 9), dtype=U64))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for ptr, nbytes in ((None, 0), (None, need), (scratch.data_ptr(), need - 256)):
        with pytest.raises(EngineError, match="scratch too small"):
            _lib.call("tfhe_mi355_keyswitch_with_key_async", eng._h, key._h, d_in.data_ptr(), d_out.data_ptr(), 3, ptr,
                      nbytes, stream)
    other = Engine(params_2_2, 0)
    with pytest.raises(ValueError, match="another engine"):
        other.keyswitch_with_key(key, np.zeros((1, 65), dtype=U64))
    with pytest.raises(EngineError, match="another context"):
        _lib.call("tfhe_mi355_keyswitch_with_key_async", other._h, key._h, d_in.data_ptr(), d_out.data_ptr(), 3,
                  scratch.data_ptr(), need, stream)
    key.close()
    with pytest.raises(ValueError, match="closed"):
        eng.keyswitch_with_key(key, np.zeros((1, 65), dtype=U64))
    other.close()
    eng.close()


# ---- integer.WopbsKey on the engine equals the CPU stand-in on the same keys --------------------------------
def _gpu_only_for_wopbs(name, seed=61):
    if ("gpu_only", name) not in _cache:
        from tfhe_mi355 import integer
        from tfhe_mi355.shortint import ServerKey

        cks = cases.client_key(name, seed)
        _cache[("gpu_only", name)] = integer.WopbsKey.new_wopbs_key_only_for_wopbs(cks, ServerKey(cks))
    return _cache[("gpu_only", name)]


VALUES = np.array([27, 54], dtype=U64)


def test_integer_wopbs_api_equals_the_stand_in_2_2(orc):
    from tfhe_mi355 import integer

    cks, cpu = cases.standin_only_for_wopbs("wop_2_2")
    gpu = _gpu_only_for_wopbs("wop_2_2")
    ick = integer.ClientKey(cks, 3)
    ct = ick.encrypt(VALUES)
    lut = cpu.generate_lut_radix(ct, lambda x: 2 * x + 1)
    got = gpu.wopbs(ct, lut)
    assert np.array_equal(got.data, cpu.wopbs(ct, lut).data)
    assert np.array_equal(ick.decrypt(got), (2 * VALUES + 1) % 64)
    # a device-resident batch comes back device-resident, with the same words
    import torch

    dev = integer.RadixBatch(_dev(ct.data), list(ct.degree), list(ct.noise))
    back = gpu.wopbs(dev, lut)
    assert isinstance(back.data, torch.Tensor) and back.data.is_cuda
    assert np.array_equal(_host(back.data), got.data)


def test_integer_wopbs_without_padding_equals_the_stand_in_2_2(orc):
    from tfhe_mi355 import integer

    cks, cpu = cases.standin_only_for_wopbs("wop_2_2")
    gpu = _gpu_only_for_wopbs("wop_2_2")
    ick = integer.ClientKey(cks, 3)
    ct = ick.encrypt_without_padding(VALUES)
    lut = cpu.generate_lut_radix_without_padding(ct, lambda x: 2 * x)
    got = gpu.wopbs_without_padding(ct, lut)
    assert np.array_equal(got.data, cpu.wopbs_without_padding(ct, lut).data)
    assert np.array_equal(ick.decrypt_without_padding(got), (2 * VALUES) % 64)


def test_integer_bivariate_wopbs_equals_the_stand_in(orc):
    from tfhe_mi355 import integer

    cks, cpu = cases.standin_only_for_wopbs("wop_2_2")
    gpu = _gpu_only_for_wopbs("wop_2_2")
    ick = integer.ClientKey(cks, 3)
    other = np.array([5, 62], dtype=U64)
    ct1, ct2 = ick.encrypt(VALUES), ick.encrypt(other)
    lut = cpu.generate_lut_bivariate_radix(ct1, ct2, lambda x, y: 2 * x * y)
    got = gpu.bivariate_wopbs_with_degree(ct1, ct2, lut)
    assert got.num_blocks == 3
    assert np.array_equal(got.data, cpu.bivariate_wopbs_with_degree(ct1, ct2, lut).data)
    assert np.array_equal(ick.decrypt(got), (2 * VALUES * other) % 64)


def test_integer_wopbs_without_padding_equals_the_stand_in_1_2(orc):
    """WOPBS 1_2: 3 blocks of 3 bits = 9 = log2 N bits, a LUT of one polynomial: the chain alone, from the
    LUT leaf up to the step of degree N/2, three outputs."""
    from tfhe_mi355 import integer

    cks, cpu = cases.standin_only_for_wopbs("wop_1_2")
    gpu = _gpu_only_for_wopbs("wop_1_2")
    ick = integer.ClientKey(cks, 3)
    values = np.array([5, 6], dtype=U64)
    ct = ick.encrypt_without_padding(values)
    lut = cpu.generate_lut_radix_without_padding(ct, lambda x: x + 1)
    assert lut.shape == (3, 512)
    got = gpu.wopbs_without_padding(ct, lut)
    assert np.array_equal(got.data, cpu.wopbs_without_padding(ct, lut).data)
    # the reference's generator reads output block o at bit log2(carry) * o of f (wopbs/mod.rs:622-625), which
    # is the radix digit only where carry modulus = message modulus; at 1_2 block o holds bit 2 o of f
    want = [sum(((int(v) + 1) >> (2 * o) & 1) << o for o in range(3)) for v in values]
    assert np.array_equal(ick.decrypt_without_padding(got), want)


def test_cross_set_round_trip_at_the_real_sets(orc, params_2_2, keys_2_2):
    """PARAM_MESSAGE_2_CARRY_2_KS_PBS (the session's keys) -> WOPBS 2_2 (decrypt_case's keys) -> wopbs ->
    back: K = 2 integers of 3 blocks, f = 2x, decrypted under the PBS client key."""
    from tfhe_mi355 import Engine, client, integer
    from tfhe_mi355.shortint import NOISE_NOMINAL, ServerKey, WopbsKey

    d = decrypt_case(orc)
    P, W, wcks = params_2_2, d["P"], d["cks"]
    sks = ServerKey(None, engine=Engine(P, 0), bsk=keys_2_2.bsk, ksk=keys_2_2.ksk, parameters=P)
    wsks = ServerKey(None, engine=Engine(W, 0), bsk=d["bsk"], ksk=d["ksk"], parameters=W)
    to_wop = client.gen_keyswitch_key(301, keys_2_2.glwe_sk, wcks.large_lwe_secret_key, P.ks_base_log, P.ks_level,
                                      W.lwe_modular_std_dev)
    to_pbs = client.gen_keyswitch_key(302, wcks.large_lwe_secret_key, keys_2_2.lwe_sk, P.ks_base_log, P.ks_level,
                                      P.lwe_modular_std_dev)
    sw = WopbsKey(wsks, W, d["pfpksk"], pbs_server_key=sks,
                  ksk_pbs_to_wopbs=wsks.engine.keyswitch_key(to_wop, P.big_lwe_dimension, W.big_lwe_dimension,
                                                             P.ks_base_log, P.ks_level),
                  ksk_wopbs_to_pbs=sks.engine.keyswitch_key(to_pbs, W.big_lwe_dimension, P.lwe_dimension,
                                                            P.ks_base_log, P.ks_level))
    wk = integer.WopbsKey.new_from_shortint(sw)
    values = np.array([42, 27], dtype=U64)
    digits = np.stack([(values >> U64(2 * j)) % U64(4) for j in range(3)], axis=1)          # [K][blocks]
    x = orc.lwe_encrypt(303, keys_2_2.glwe_sk, digits.ravel() * U64(P.delta), P.glwe_modular_std_dev)
    ct = integer.RadixBatch(x.reshape(2, 3, -1), [3, 3, 3], [NOISE_NOMINAL] * 3)
    wct = wk.keyswitch_to_wopbs_params(sks, ct)
    res = wk.wopbs(wct, wk.generate_lut_radix(wct, lambda v: 2 * v))
    out = wk.keyswitch_to_pbs_params(res)
    assert out.data.shape == (2, 3, P.big_lwe_dimension + 1)
    pts = orc.lwe_decrypt(keys_2_2.glwe_sk, np.ascontiguousarray(out.data.reshape(6, -1)))
    dec = (((pts + U64(P.delta >> 1)) // U64(P.delta)) % U64(4)).reshape(2, 3)
    assert [int(r[0] + 4 * r[1] + 16 * r[2]) for r in dec] == [(2 * 42) % 64, (2 * 27) % 64]
