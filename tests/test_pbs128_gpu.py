"""128-bit-torus PBS on the GPU: bit-exact against the CPU restatement (tests/pbs_ref128.c) at every accepted
shape, within the exact CMUX's bound, decrypting at the reference's test shape, and refusing what it does not
compute."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pbs128_cases as C  # noqa: E402
import pbs128_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048]
SHAPES = [(N, k) for N in SIZES for k in (1, 2, 3) if (k + 1) * N <= 4096]


def _engine(p):
    from tfhe_mi355 import Engine

    return Engine.for_u128(p, 0)


def _ref(p, bsk):
    ref = R.RefEngine128(p)
    ref.upload_bootstrap_key_u128(bsk)
    return ref


def _max_distance(a, b) -> int:
    return max(R.mod_distance(x, y) for x, y in zip(R.to_ints(a), R.to_ints(b)))


@pytest.mark.parametrize("N", SIZES)
def test_tables_equal_python(N):
    from tfhe_mi355.engine import debug_fft128_tables

    twist, tw = debug_fft128_tables(N)
    want_twist, want_tw = R.tables(N)
    assert np.array_equal(twist.view(np.uint64), want_twist.view(np.uint64))
    assert np.array_equal(tw.view(np.uint64), want_tw.view(np.uint64))


def test_backward_conversion_equals_big_integers():
    from tfhe_mi355.engine import debug_torus128_from_f128

    hi, lo = C.backward_inputs(100000, seed=11)
    acc = R.uniform(12, len(hi))
    got = debug_torus128_from_f128(hi, lo, acc)
    assert np.array_equal(got, R.torus_from_f128(hi, lo, acc))  # the restatement, every input
    acc_i, got_i = R.to_ints(acc), R.to_ints(got)
    for i in range(len(hi)):  # and big-integer arithmetic
        assert got_i[i] == (acc_i[i] + R.exact_torus_from_dd(float(hi[i]), float(lo[i]))) & R.MASK128, (hi[i], lo[i])
    assert np.array_equal(debug_torus128_from_f128(hi[:50], lo[:50]), R.torus_from_f128(hi[:50], lo[:50]))


@pytest.mark.parametrize("N,k,level,base_log,n", [(256, 2, 2, 7, 3), (2048, 1, 1, 23, 2)])
def test_fourier_key_through_blind_rotation(N, k, level, base_log, n):
    """Every key polynomial enters the result: all mask elements rotate, every row and column is read."""
    case = C.parity_case(N, k, level, base_log, batch=2, n=n)
    lwe = R.uniform(77 + N, 2 * (n + 1)).reshape(2, n + 1, 2)
    eng = _engine(case.params)
    eng.upload_bootstrap_key_u128(case.bsk)
    got = eng.blind_rotate_u128(lwe, case.luts, case.idx)
    eng.close()
    ref = _ref(case.params, case.bsk)
    assert np.array_equal(got, ref.blind_rotate_u128(lwe, case.luts, case.idx))
    # sensitivity: flipping one bit of the LAST key polynomial changes the reference's result
    bsk2 = case.bsk.copy()
    bsk2[-1, -1, -1, -1, N // 2, 0] ^= np.uint64(1) << np.uint64(40)
    assert not np.array_equal(got, _ref(case.params, bsk2).blind_rotate_u128(lwe, case.luts, case.idx))


@pytest.mark.parametrize("N,k,level,base_log", [(256, 2, 2, 7), (2048, 1, 1, 23)])
def test_one_crafted_cmux(N, k, level, base_log):
    eng = None
    for rotation in (1, N - 1):
        case = C.one_cmux_case(N, k, level, base_log, rotation)
        if eng is None:
            eng = _engine(case.params)
            eng.upload_bootstrap_key_u128(case.bsk)
            ref = _ref(case.params, case.bsk)
        got = eng.blind_rotate_u128(case.lwe, case.acc)
        assert np.array_equal(got, ref.blind_rotate_u128(case.lwe, case.acc)), rotation
        want = R.exact_cmux(case.acc, case.bsk[0], rotation, N, k, base_log, level)
        d, bound = _max_distance(got[0], want), C.cmux_bound(N, k, level, base_log)
        print(f"({N},{k},{level},{base_log}) rotation {rotation}: distance 2^{math.log2(max(d, 1)):.2f}, "
              f"bound 2^{math.log2(bound):.1f}")
        assert d <= bound
    eng.close()


@pytest.mark.parametrize("level,base_log", [(1, 7), (1, 23), (3, 7), (3, 23)])
@pytest.mark.parametrize("N,k", SHAPES)
def test_pbs_bit_exact(N, k, level, base_log):
    eng = _engine(C.params(5, N, k, level, base_log))
    batch = eng.pbs_u128_resident() + 1
    assert batch > 1
    case = C.parity_case(N, k, level, base_log, batch)
    eng.upload_bootstrap_key_u128(case.bsk)
    got = eng.programmable_bootstrap_u128(case.lwe, case.luts, case.idx)
    eng.close()
    assert got.shape == (batch, k * N + 1, 2)
    assert np.array_equal(got, _ref(case.params, case.bsk).programmable_bootstrap_u128(case.lwe, case.luts, case.idx))


@pytest.mark.parametrize("N,k,level,base_log", [(512, 2, 3, 7), (2048, 1, 1, 23)])
def test_modulus_127_rounding(N, k, level, base_log):
    case = C.parity_case(N, k, level, base_log, batch=4)
    eng = _engine(case.params)
    eng.upload_bootstrap_key_u128(case.bsk)
    ref = _ref(case.params, case.bsk)
    for fn in ("programmable_bootstrap_u128", "blind_rotate_u128"):
        got = getattr(eng, fn)(case.lwe, case.luts, case.idx, ciphertext_modulus_log=127)
        assert np.array_equal(got, getattr(ref, fn)(case.lwe, case.luts, case.idx, ciphertext_modulus_log=127)), fn
        assert not np.any(got[..., 0] & np.uint64(1)), fn
    native = eng.programmable_bootstrap_u128(case.lwe, case.luts, case.idx)
    assert np.any(native[..., 0] & np.uint64(1))  # the rounding is not a no-op on these outputs
    eng.close()


def test_decryption_at_reference_shape():
    """(N, k, L, b) = (2048, 1, 1, 23), sigma_glwe = 8.6457178e-32 (TEST_PARAMS_4_BITS_NATIVE_U128), n cut to 64."""
    from tfhe_mi355 import core_crypto as cc

    N, n, bits = 2048, 64, 4
    p = C.params(n, N, 1, 1, 23)
    lwe_sk, glwe_sk = R.binary_key(51, n), R.binary_key(52, N)
    bsk = R.gen_bsk(53, lwe_sk, glwe_sk, 1, N, 23, 1, C.GLWE_STD, threads=16)
    fbsk = cc.convert_standard_lwe_bootstrap_key_to_fourier_128(bsk, p)
    msgs = list(range(1 << bits))
    delta = 1 << (128 - bits - 1)
    cts = R.lwe_encrypt(54, lwe_sk, R.to_words([m * delta for m in msgs]), p.lwe_modular_std_dev)
    f = lambda m: (3 * m + 5) % 16  # noqa: E731
    accs = np.stack([R.identity_accumulator(N, 1, bits), R.identity_accumulator(N, 1, bits, f)])
    both = np.concatenate([cts, cts])
    idx = np.repeat(np.arange(2, dtype=np.uint32), len(msgs))
    out = cc.programmable_bootstrap_f128_lwe_ciphertext_batch(both, accs, fbsk, lut_indexes=idx)
    fbsk.engine.close()
    dec = R.decode(R.lwe_decrypt(glwe_sk, out), bits)
    assert dec[:16] == msgs
    assert dec[16:] == [f(m) for m in msgs]


def test_async_on_a_stream_and_scratch():
    import torch

    from tfhe_mi355 import EngineError

    N, k, level, base_log, batch = 512, 2, 3, 7, 6
    case = C.parity_case(N, k, level, base_log, batch)
    eng = _engine(case.params)
    eng.upload_bootstrap_key_u128(case.bsk)
    want = eng.programmable_bootstrap_u128(case.lwe, case.luts, case.idx)
    want_glwe = eng.blind_rotate_u128(case.lwe, case.luts, case.idx, ciphertext_modulus_log=100)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()  # noqa: E731
    d_in, d_luts = dev(case.lwe), dev(case.luts)
    d_idx = torch.from_numpy(case.idx.view(np.int32)).cuda()
    need = eng.pbs_u128_scratch_bytes(batch)
    assert need > 0 and need == eng.blind_rotate_u128_scratch_bytes(batch)
    assert eng.pbs_u128_scratch_bytes(0) == 0
    stream = torch.cuda.Stream()
    d_out = torch.zeros((batch, k * N + 1, 2), dtype=torch.int64, device="cuda")
    d_glwe = torch.zeros((batch, (k + 1) * N, 2), dtype=torch.int64, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.programmable_bootstrap_u128_async(d_in, d_out, d_luts, 2, batch, d_lut_indexes=d_idx, stream=stream,
                                              d_scratch=scratch)
        eng.blind_rotate_u128_async(d_in, d_glwe, d_luts, 2, batch, d_lut_indexes=d_idx, stream=stream,
                                    d_scratch=scratch, ciphertext_modulus_log=100)
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(d_glwe.cpu().numpy().view(np.uint64), want_glwe)
    # one byte less scratch is an error, and nothing runs
    d_out.fill_(7)
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    for call in (eng.programmable_bootstrap_u128_async, eng.blind_rotate_u128_async):
        with pytest.raises(EngineError, match="scratch too small"):
            call(d_in, d_out, d_luts, 2, batch, d_lut_indexes=d_idx, stream=stream, d_scratch=short)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7).all()
    # count = 0 is a no-op
    assert eng.programmable_bootstrap_u128(np.zeros((0, 6, 2), dtype=np.uint64), case.luts).shape == (0, k * N + 1, 2)
    eng.programmable_bootstrap_u128_async(d_in, d_out, d_luts, 2, 0, stream=stream)
    eng.close()


@pytest.mark.parametrize("kw,message", [
    (dict(N=4096), "polynomial_size must be 256, 512, 1024 or 2048"),
    (dict(k=4, N=512), "glwe_dimension must be 1, 2 or 3"),
    (dict(k=3, N=2048), r"\(k\+1\)\*N must be <= 4096"),
    (dict(level=5, base_log=7), r"pbs_level must be in \[1, 4\]"),
    (dict(base_log=32), r"pbs_base_log must be in \[2, 31\]"),
    (dict(level=4, base_log=31, N=512), None),  # 124 < 128: accepted
])
def test_shape_refusals(kw, message):
    from tfhe_mi355 import EngineError

    a = dict(n=2, N=1024, k=1, level=1, base_log=23)
    a.update(kw)
    p = C.params(a["n"], a["N"], a["k"], a["level"], a["base_log"])
    if message is None:
        _engine(p).close()
        return
    with pytest.raises(EngineError, match=message):
        _engine(p)


def test_base_log_times_level_128_is_refused():
    """base_log * level = 128 needs base_log = 32 (4 levels) or 64 (2 levels), both beyond base_log <= 31: the
    call is refused, and the message names the first limit it breaks."""
    from tfhe_mi355 import EngineError

    with pytest.raises(EngineError, match=r"pbs_base_log must be in \[2, 31\]"):
        _engine(C.params(2, 512, 1, 4, 32))
    with pytest.raises(EngineError, match=r"pbs_base_log must be in \[2, 31\]"):
        _engine(C.params(2, 512, 1, 2, 64))


def test_modulus_log_refusals():
    from tfhe_mi355 import EngineError

    case = C.parity_case(256, 1, 1, 7, batch=1)
    eng = _engine(case.params)
    eng.upload_bootstrap_key_u128(case.bsk)
    for m in (64, 129, 0):
        with pytest.raises(EngineError, match=r"ciphertext_modulus_log must be in \[65, 128\]"):
            eng.programmable_bootstrap_u128(case.lwe, case.luts, ciphertext_modulus_log=m)
    ref = _ref(case.params, case.bsk)
    assert np.array_equal(eng.programmable_bootstrap_u128(case.lwe, case.luts, ciphertext_modulus_log=65),
                          ref.programmable_bootstrap_u128(case.lwe, case.luts, ciphertext_modulus_log=65))
    with pytest.raises(EngineError, match="expected"):
        eng.upload_bootstrap_key_u128(case.bsk[:, :, :, :, :-1])
    eng.close()


def test_width_mixing_is_refused():
    from tfhe_mi355 import Engine, EngineError
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P22

    # the 2_2 shape (2048, 1, base 23, level 1) is within both widths' limits: an ordinary context takes either
    p = P22.with_(lwe_dimension=2, name="u128_mixing")
    bsk128 = R.uniform(61, 2 * 4 * 2048).reshape(2, 1, 2, 2, 2048, 2)
    bsk64 = np.ascontiguousarray(bsk128[..., 1])
    lwe128, lut128 = R.uniform(62, 3).reshape(1, 3, 2), R.uniform(63, 4096).reshape(1, 4096, 2)
    e64 = Engine(p, 0)
    e64.upload_bootstrap_key(bsk64)
    with pytest.raises(EngineError, match="64-bit-torus keys"):
        e64.upload_bootstrap_key_u128(bsk128)
    with pytest.raises(EngineError, match="64-bit-torus keys"):
        e64.programmable_bootstrap_u128(lwe128, lut128)
    e64.close()
    e128 = Engine(p, 0)
    e128.upload_bootstrap_key_u128(bsk128)
    with pytest.raises(EngineError, match="128-bit-torus keys"):
        e128.upload_bootstrap_key(bsk64)
    with pytest.raises(EngineError, match="128-bit-torus keys"):
        e128.upload_bootstrap_key_u32(bsk64.astype(np.uint32))
    with pytest.raises(EngineError, match="128-bit-torus keys"):
        e128.programmable_bootstrap(lwe128[..., 1], lut128[..., 1])
    ref = _ref(p, bsk128)
    assert np.array_equal(e128.programmable_bootstrap_u128(lwe128, lut128),
                          ref.programmable_bootstrap_u128(lwe128, lut128))  # and still serves its own width
    e128.close()
    # a context created for the 128-bit torus serves nothing else, with or without a key
    only = _engine(C.params(2, 256, 1, 1, 7))
    with pytest.raises(EngineError, match="created for the 128-bit torus"):
        only.upload_bootstrap_key(np.zeros(2 * 4 * 256, dtype=np.uint64))
    only.close()


def test_multi_device_context_is_refused():
    from tfhe_mi355 import Engine, EngineError
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P22

    p = P22.with_(lwe_dimension=2, name="u128_multi")
    eng = Engine(p, devices=[0, 0])
    for call in (lambda: eng.upload_bootstrap_key_u128(np.zeros((2, 1, 2, 2, 2048, 2), dtype=np.uint64)),
                 lambda: eng.programmable_bootstrap_u128(np.zeros((1, 3, 2), dtype=np.uint64),
                                                         np.zeros((1, 4096, 2), dtype=np.uint64)),
                 lambda: eng.pbs_u128_scratch_bytes(1), lambda: eng.pbs_u128_resident()):
        with pytest.raises(EngineError, match="multi-device"):
            call()
    eng.close()
