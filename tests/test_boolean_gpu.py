"""The 32-bit-torus path on the GPU (csrc/pbs_classic32.hip, keyswitch32.hip, boolean_ops.hip and the
"32-bit torus" section of the C ABI), bit-exact against RefEngine32 (tests/boolean_reference.py: the
oracle's FFT DAG, the fma MAC and backward conversion of boolean_ref32.c, exact integer keyswitch)."""
import dataclasses

import numpy as np
import pytest

from boolean_cases import gate_inputs, run_gate_batch
from boolean_reference import RefEngine32, conversion_edge_fractions, conversion_expected, decompose32, widen
from pbs_edge_inputs32 import crafted_case32, unit_mask32
from test_keyswitch_reference import edge_rows
from tfhe_mi355 import boolean as B

pytestmark = pytest.mark.gpu

U32 = np.uint32
# N, k, L, the set's base_log, one other base_log (base_log * L <= 30)
SHAPES = [(512, 2, 3, 6, 9), (1024, 2, 2, 10, 15), (1024, 1, 4, 5, 7), (1024, 1, 3, 7, 10)]


def _params(N, k, L, base_log, n, **kw):
    return dataclasses.replace(B.DEFAULT_PARAMETERS, lwe_dimension=n, glwe_dimension=k, polynomial_size=N,
                               pbs_base_log=base_log, pbs_level=L, name=f"bool_{N}_{k}_{L}_{base_log}_{n}", **kw)


def _engine(p):
    from tfhe_mi355 import Engine

    return Engine(p, 0)


def _same(got, exp, what):
    assert got.dtype == exp.dtype == U32 and got.shape == exp.shape, what
    bad = np.flatnonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, f"{what}: rows {bad.tolist()[:16]} differ, {np.count_nonzero(got != exp)} words"


def _pbs_pair(N, k, L, base_log, n, seed):
    """(engine, reference) of a shape under the same random u32 bootstrapping key."""
    p = _params(N, k, L, base_log, n)
    bsk = np.random.default_rng(seed).integers(0, 1 << 32, n * L * (k + 1) * (k + 1) * N, dtype=U32)
    eng, ref = _engine(p), RefEngine32(p)
    eng.upload_bootstrap_key_u32(bsk)
    ref.upload_bootstrap_key_u32(bsk)
    return eng, ref


def _pbs_rows(N, n, count, seed):
    """random words; zero and unit mask words; bodies 0, 1 << 31 and 2^32 - 1."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (count, n + 1), dtype=U32)
    bodies = [0, 1 << 31, (1 << 32) - 1]
    for r in range(count):
        if count > 1 or seed % 2:
            x[r, -1] = bodies[(r + seed) % 3]
        if r % 3 == 1:
            x[r, :n] = 0
        elif r % 3 == 2:
            x[r, :n] = unit_mask32(N)
        else:
            x[r, 0] = 0  # one zero mask word among random ones
    return x


def _extract(glwe, k, N):
    """sample extraction at degree 0 of [count][(k+1)N] u32 accumulators."""
    g = glwe.reshape(-1, k + 1, N)
    out = np.empty((g.shape[0], k * N + 1), dtype=U32)
    mask = g[:, :k]
    out[:, :-1] = np.concatenate([mask[:, :, :1], (U32(0) - mask[:, :, :0:-1]).astype(U32)], axis=2).reshape(
        g.shape[0], -1)
    out[:, -1] = g[:, k, 0]
    return out


# ---- 1. PBS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("which", [0, 1], ids=["set_base", "other_base"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}_{s[1]}_{s[2]}")
def test_pbs_bit_exact(shape, which, n):
    N, k, L = shape[:3]
    base_log = shape[3 + which]
    eng, ref = _pbs_pair(N, k, L, base_log, n, seed=N + k + L + n)
    rng = np.random.default_rng(base_log)
    luts = rng.integers(0, 1 << 32, (2, (k + 1) * N), dtype=U32)  # random LUTs: a constant one hides rotation errors
    eng.kernel_timing(1)
    for count in (1, 3):
        x = _pbs_rows(N, n, count, seed=count + n)
        idx = (np.arange(count, dtype=np.uint32) + 1) % 2
        exp = ref.programmable_bootstrap_u32(x, luts, idx)
        exp_glwe = ref.blind_rotate_u32(x, luts, idx)
        _same(exp, _extract(exp_glwe, k, N), "reference forms")
        got = eng.programmable_bootstrap_u32(x, luts, idx)
        got_glwe = eng.blind_rotate_u32(x, luts, idx)
        _same(got_glwe, exp_glwe, f"glwe_out, count {count}")
        _same(got, exp, f"extracted, count {count}")
        _same(got, _extract(got_glwe, k, N), "the two forms agree")
    if n == 1:
        # the crafted case: the first (only) CMUX decomposes ties, carries, the +2^(B-1) digit and the
        # rounding overflow, directly, negated (b~ = N) and through the body's rounding overflow (b~ = 2N)
        cts, lut, D = crafted_case32(base_log, L, N, k, seed=7)
        assert decompose32(D, base_log, L).max() == 1 << (base_log - 1)
        _same(eng.blind_rotate_u32(cts, lut), ref.blind_rotate_u32(cts, lut), "crafted, glwe_out")
        _same(eng.programmable_bootstrap_u32(cts, lut), ref.programmable_bootstrap_u32(cts, lut), "crafted")
    ran = set(eng.kernel_times())
    assert ran == {"pbs_classic32_kernel"}, ran  # the u32 kernel family, not the u64 one
    eng.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}_{s[1]}_{s[2]}")
def test_pbs_one_past_a_resident_grid(shape):
    """one ciphertext per workgroup: resident + 1 ciphertexts make the grid run a second wave."""
    N, k, L, base_log = shape[:4]
    eng, ref = _pbs_pair(N, k, L, base_log, 5, seed=3 * N + k)
    resident = eng.pbs_u32_resident()
    assert 256 <= resident <= 8192, resident
    count = resident + 1
    x = _pbs_rows(N, 5, count, seed=11)
    luts = np.random.default_rng(5).integers(0, 1 << 32, (2, (k + 1) * N), dtype=U32)
    idx = (np.arange(count, dtype=np.uint32) // 3) % 2
    _same(eng.programmable_bootstrap_u32(x, luts, idx), ref.programmable_bootstrap_u32(x, luts, idx),
          f"{count} ciphertexts")
    eng.close()


def test_pbs_async_on_device_tensors():
    import torch

    N, k, L, base_log = SHAPES[0][:4]
    eng, ref = _pbs_pair(N, k, L, base_log, 5, seed=9)
    x = _pbs_rows(N, 5, 7, seed=2)
    lut = np.random.default_rng(1).integers(0, 1 << 32, (1, (k + 1) * N), dtype=U32)
    dev = lambda a: torch.from_numpy(np.array(a).view(np.int32)).cuda()  # noqa: E731
    d_out = torch.zeros((7, k * N + 1), dtype=torch.int32, device="cuda")
    eng.programmable_bootstrap_u32_async(dev(x), d_out, dev(lut), 1, 7)
    torch.cuda.current_stream().synchronize()
    _same(d_out.cpu().numpy().view(U32), ref.programmable_bootstrap_u32(x, lut), "device form")
    eng.close()


# ---- 2. Fourier key ---------------------------------------------------------------------------------
def _engine_position(N):
    """FFT position of each element of the engine's spectrum layout (test_serialization.py)."""
    e = np.arange(N // 2)
    lane, s = e % 64, e // 64
    if N == 1024:
        return 64 * (lane & 7) + 8 * (lane >> 3) + s
    assert N == 512
    return 16 * (lane & 15) + (lane >> 4) + 4 * s


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: f"{s[0]}_{s[1]}_{s[2]}")
def test_fourier_key_is_the_oracles_of_the_widened_key(orc, shape):
    import ctypes

    import torch

    N, k, L, base_log = shape[:4]
    n, M = 3, N // 2
    p = _params(N, k, L, base_log, n)
    bsk = np.random.default_rng(N).integers(0, 1 << 32, n * L * (k + 1) * (k + 1) * N, dtype=U32)
    bsk[:4] = [0, 1 << 31, (1 << 32) - 1, (1 << 31) - 1]
    eng = _engine(p)
    eng.upload_bootstrap_key_u32(bsk)
    ptr, nbytes = eng.fourier_bootstrap_key()
    assert nbytes == n * L * (k + 1) * (k + 1) * M * 16
    host = np.empty(nbytes // 8, dtype=np.float64)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
    got = host.view(np.complex128).reshape(-1, M)
    exp = orc.FourierBsk(widen(bsk), n, k, N, base_log, L).fourier().reshape(-1, M)
    exp = np.ascontiguousarray(exp[:, _engine_position(N)])
    exp = np.ldexp(exp.view(np.float64), -int(np.log2(M))).view(np.complex128)  # the resident 1/M
    bad = np.count_nonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad == 0, f"{bad} of {got.size * 2} doubles differ"
    eng.close()


# ---- 3. keyswitch -------------------------------------------------------------------------------------
KS_PAIRS = [(3, 4), (3, 5), (2, 7), (2, 8)]


@pytest.fixture(scope="module")
def ks_engine():
    eng = _engine(_params(512, 2, 3, 6, 2))
    yield eng
    eng.close()


def _ks_rows(B, L, in_dim, count, seed):
    """the worst-case digit rows of test_keyswitch_reference.edge_rows, in the top 32 bits (the 32-bit
    decomposer reads the same bits: the rounding bit is 63 - B L >= 33)."""
    return (edge_rows(B, L, in_dim + 1, count, seed=seed) >> np.uint64(32)).astype(U32)


@pytest.mark.parametrize("arm", [1, 2], ids=["integer", "mfma"])
@pytest.mark.parametrize("dec", KS_PAIRS, ids=str)
@pytest.mark.parametrize("in_dim", [11, 1024])
def test_keyswitch_both_arms(ks_engine, in_dim, dec, arm):
    """out_dim + 1 = 631 columns (not a multiple of the 64-column tile), counts 1, 63 and 65 (around the
    64-row tile), the worst-case digit rows in front."""
    Bk, Lk = dec
    out_dim = 630
    rng = np.random.default_rng(in_dim + 10 * Bk + Lk)
    ksk = rng.integers(0, 1 << 32, in_dim * Lk * (out_dim + 1), dtype=U32)
    x = _ks_rows(Bk, Lk, in_dim, 65, seed=in_dim + Bk)
    d = decompose32(x[:, :in_dim], Bk, Lk)
    assert d.max() == 1 << (Bk - 1) and d.min() == -(1 << (Bk - 1))  # the rows reach the largest digits
    exp = RefEngine32(B.DEFAULT_PARAMETERS).keyswitch_u32(x, ksk, in_dim, out_dim, Bk, Lk)
    ks_engine.kernel_timing(1)
    for count in (1, 63, 65):
        got = ks_engine.debug_keyswitch_u32(ksk, in_dim, out_dim, Bk, Lk, x[:count], arm=arm)
        _same(got, exp[:count], f"count {count}")
    ran = set(ks_engine.kernel_times())
    assert ran == {"keyswitch32_integer" if arm == 1 else "keyswitch32_mfma"}, ran
    ks_engine.kernel_timing(0)


def test_keyswitch_integer_arm_where_mfma_refuses(ks_engine):
    """base_log 8: the digits do not fit the int8 planes; the engine's choice is the integer kernel."""
    from tfhe_mi355 import EngineError

    in_dim, out_dim, Bk, Lk = 70, 66, 8, 3
    rng = np.random.default_rng(8)
    ksk = rng.integers(0, 1 << 32, in_dim * Lk * (out_dim + 1), dtype=U32)
    x = _ks_rows(Bk, Lk, in_dim, 9, seed=1)
    exp = RefEngine32(B.DEFAULT_PARAMETERS).keyswitch_u32(x, ksk, in_dim, out_dim, Bk, Lk)
    _same(ks_engine.debug_keyswitch_u32(ksk, in_dim, out_dim, Bk, Lk, x, arm=0), exp, "engine's choice")
    with pytest.raises(EngineError, match="int8-MFMA"):
        ks_engine.debug_keyswitch_u32(ksk, in_dim, out_dim, Bk, Lk, x, arm=2)
    with pytest.raises(EngineError, match="base_log\\*level <= 30"):
        ks_engine.debug_keyswitch_u32(np.zeros(in_dim * 4 * (out_dim + 1), dtype=U32), in_dim, out_dim, 8, 4, x, arm=0)


@pytest.mark.parametrize("name", ["DEFAULT_PARAMETERS", "TFHE_LIB_PARAMETERS"])
def test_keyswitch_through_the_context_key(name):
    """the context's own key (four byte planes repacked at upload), host and device forms, rows past
    `count` untouched."""
    import torch

    p = getattr(B, name)
    in_dim, n, Bk, Lk = p.big_lwe_dimension, p.lwe_dimension, p.ks_base_log, p.ks_level
    ksk = np.random.default_rng(n).integers(0, 1 << 32, in_dim * Lk * (n + 1), dtype=U32)
    eng, ref = _engine(p), RefEngine32(p)
    eng.upload_keyswitch_key_u32(ksk)
    ref.upload_keyswitch_key_u32(ksk)
    assert eng.ks_u32_scratch_bytes(5) > 0  # the int8-MFMA arm
    x = _ks_rows(Bk, Lk, in_dim, 65, seed=n)
    exp = ref.keyswitch_u32(x)
    for count in (1, 63, 65):
        _same(eng.keyswitch_u32(x[:count]), exp[:count], f"host form, count {count}")
    d_x = torch.from_numpy(x.view(np.int32)).cuda()
    d_out = torch.full((68, n + 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    eng.keyswitch_u32_async(d_x, d_out, 65)
    torch.cuda.current_stream().synchronize()
    got = d_out.cpu().numpy().view(U32)
    _same(got[:65], exp, "device form")
    assert (got[65:] == U32(0x5A5A5A5A)).all()
    eng.close()


# ---- 4. gates -----------------------------------------------------------------------------------------
_gate_cache = {}


def _gate_setup(name):
    """client key, GPU and reference server keys over the same key material, the shared inputs and the
    reference outputs (computed once per parameter set)."""
    if name not in _gate_cache:
        p = getattr(B, name)
        cks = B.ClientKey(p, seed=21)
        bsk, ksk = cks.server_key_material()
        eng, ref = _engine(p), RefEngine32(p)
        for e in (eng, ref):
            e.upload_bootstrap_key_u32(bsk)
            e.upload_keyswitch_key_u32(ksk)
        x = gate_inputs(cks)
        exp = run_gate_batch(B.ServerKey(ref, p), x)
        _gate_cache[name] = (p, cks, B.ServerKey(eng, p), x, exp)
    return _gate_cache[name]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("name", ["DEFAULT_PARAMETERS", "DEFAULT_PARAMETERS_KS_PBS"])
def test_gates_bit_exact_and_truth_table(name, form):
    import torch

    p, cks, sk, x, exp = _gate_setup(name)
    if form == "async":
        x = {key: B.BoolBatch(torch.from_numpy(v.data.view(np.int32)).cuda()) for key, v in x.items()}
    sk.engine.kernel_timing(1)
    got = run_gate_batch(sk, x)
    torch.cuda.synchronize()
    ran = set(sk.engine.kernel_times())
    sk.engine.kernel_timing(0)
    assert {"pbs_classic32_kernel", "keyswitch32", "boolean_ops"} <= ran and "pbs_classic_kernel" not in ran, ran
    for gate, (ct, truth) in got.items():
        assert ct.on_device == (form == "async"), gate
        _same(np.ascontiguousarray(ct.host()), exp[gate][0].data, f"{name} {gate} ({form})")
        assert np.array_equal(cks.decrypt(ct), truth), gate


@pytest.mark.parametrize("name", ["PARAMETERS_ERROR_PROB_2_POW_MINUS_165",
                                  "PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS", "TFHE_LIB_PARAMETERS"])
def test_gates_decrypt_on_the_other_sets(name):
    p = getattr(B, name)
    cks, sk = B.gen_keys(p, seed=31, device=0)
    for gate, (ct, truth) in run_gate_batch(sk, gate_inputs(cks)).items():
        assert np.array_equal(cks.decrypt(ct), truth), (name, gate)
    sk.engine.close()


# ---- 5. depth -------------------------------------------------------------------------------------------
def test_ripple_carry_adder():
    """8-bit ripple-carry adder from xor / and_ / or_ on 16 random pairs: 40 gate batches deep."""
    p, cks, sk, _, _ = _gate_setup("DEFAULT_PARAMETERS")
    rng = np.random.default_rng(17)
    a, b = rng.integers(0, 256, 16), rng.integers(0, 256, 16)
    ea = [cks.encrypt((a >> i) & 1) for i in range(8)]
    eb = [cks.encrypt((b >> i) & 1) for i in range(8)]
    carry, total = False, np.zeros(16, dtype=np.int64)
    for i in range(8):
        axb = sk.xor(ea[i], eb[i])
        s = sk.xor(axb, carry)
        carry = sk.or_(sk.and_(ea[i], eb[i]), sk.and_(axb, carry))
        total |= cks.decrypt(s).astype(np.int64) << i
    total |= cks.decrypt(carry).astype(np.int64) << 8
    assert np.array_equal(total, a + b)


# ---- 6. conversion ----------------------------------------------------------------------------------------
def test_torus32_conversion_on_the_device():
    from tfhe_mi355.engine import debug_torus32_from_fraction

    rng = np.random.default_rng(3)
    edges = conversion_edge_fractions()
    fr = np.concatenate([edges, rng.uniform(-0.5, 0.5, 100000)])
    acc0 = rng.integers(0, 1 << 32, fr.size, dtype=U32)
    acc, x = debug_torus32_from_fraction(fr, acc0)
    exp = (np.rint(fr * 4294967296.0).astype(np.int64) & 0xFFFFFFFF).astype(U32)  # fr 2^32 is exact in f64
    assert np.array_equal(exp[:edges.size], conversion_expected(edges))
    assert x[0] == x[1] == 0x80000000  # +-1/2 wrap (a saturating convert gives 0x7fffffff)
    assert np.array_equal(x, exp)
    assert np.array_equal(acc, (acc0 + exp).astype(U32))


# ---- 7. refusals ------------------------------------------------------------------------------------------
def _small_keys(p, rng):
    k, N = p.glwe_dimension, p.polynomial_size
    return (rng.integers(0, 1 << 32, p.lwe_dimension * p.pbs_level * (k + 1) * (k + 1) * N, dtype=U32),
            rng.integers(0, 1 << 32, k * N * p.ks_level * (p.lwe_dimension + 1), dtype=U32))


def test_width_mixing_is_refused():
    from tfhe_mi355 import EngineError

    p = _params(512, 2, 3, 6, 2)
    rng = np.random.default_rng(0)
    bsk32, ksk32 = _small_keys(p, rng)
    x32 = rng.integers(0, 1 << 32, (2, 3), dtype=U32)
    lut32 = rng.integers(0, 1 << 32, 3 * 512, dtype=U32)
    # a context with u64 keys refuses u32 uploads and u32 compute calls
    e64 = _engine(p)
    e64.upload_bootstrap_key(bsk32.astype(np.uint64))
    e64.upload_keyswitch_key(ksk32.astype(np.uint64))
    for call in (lambda: e64.upload_bootstrap_key_u32(bsk32), lambda: e64.upload_keyswitch_key_u32(ksk32),
                 lambda: e64.programmable_bootstrap_u32(x32, lut32),
                 lambda: e64.keyswitch_u32(np.zeros((1, 1025), dtype=U32))):
        with pytest.raises(EngineError, match="64-bit-torus keys"):
            call()
    e64.close()
    # a context with u32 keys refuses u64 uploads and u64 compute calls
    e32 = _engine(p)
    e32.upload_bootstrap_key_u32(bsk32)
    e32.upload_keyswitch_key_u32(ksk32)
    for call in (lambda: e32.upload_bootstrap_key(bsk32.astype(np.uint64)),
                 lambda: e32.upload_keyswitch_key(ksk32.astype(np.uint64)),
                 lambda: e32.programmable_bootstrap(x32.astype(np.uint64), lut32.astype(np.uint64)),
                 lambda: e32.keyswitch(np.zeros((1, 1025), dtype=np.uint64))):
        with pytest.raises(EngineError, match="32-bit-torus keys"):
            call()
    assert e32.programmable_bootstrap_u32(x32, lut32).shape == (2, 1025)  # and still serves its own width
    e32.close()


def test_multi_device_context_is_refused():
    from tfhe_mi355 import Engine, EngineError

    p = _params(512, 2, 3, 6, 2)
    bsk32, ksk32 = _small_keys(p, np.random.default_rng(1))
    eng = Engine(p, devices=[0, 0])
    for call in (lambda: eng.upload_bootstrap_key_u32(bsk32), lambda: eng.upload_keyswitch_key_u32(ksk32),
                 lambda: eng.programmable_bootstrap_u32(np.zeros((1, 3), dtype=U32), np.zeros(1536, dtype=U32)),
                 lambda: eng.boolean_gates([0], np.zeros((1, 3), dtype=U32), np.zeros((1, 3), dtype=U32), 1)):
        with pytest.raises(EngineError, match="multi-device"):
            call()
    eng.close()


def test_scratch_opcode_and_empty_batch():
    import torch

    from tfhe_mi355 import EngineError

    p = _params(512, 2, 3, 6, 2)
    rng = np.random.default_rng(2)
    bsk32, ksk32 = _small_keys(p, rng)
    eng = _engine(p)
    eng.upload_bootstrap_key_u32(bsk32)
    eng.upload_keyswitch_key_u32(ksk32)
    w = 3
    a, b = rng.integers(0, 1 << 32, (4, w), dtype=U32), rng.integers(0, 1 << 32, (4, w), dtype=U32)
    dev = lambda v: torch.from_numpy(np.array(v).view(np.int32)).cuda()  # noqa: E731
    # _async with scratch one byte short
    need = eng.boolean_gates_scratch_bytes(4, 1)
    assert need > 0
    d_out = torch.full((4, w), 7, dtype=torch.int32, device="cuda")
    d_ops = torch.zeros(4, dtype=torch.uint8, device="cuda")
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(EngineError, match="scratch too small"):
        eng.boolean_gates_async(d_ops, dev(a), dev(b), d_out, 4, 1, d_scratch=short)
    need_mux = eng.boolean_mux_scratch_bytes(4, 1)
    with pytest.raises(EngineError, match="scratch too small"):
        eng.boolean_mux_async(dev(a), dev(b), dev(a), d_out, 4, 1,
                              d_scratch=torch.empty(need_mux - 1, dtype=torch.uint8, device="cuda"))
    need_ks = eng.ks_u32_scratch_bytes(4)
    assert need_ks > 0
    with pytest.raises(EngineError, match="scratch too small"):
        eng.keyswitch_u32_async(torch.zeros((4, 1025), dtype=torch.int32, device="cuda"), d_out, 4,
                                d_scratch=torch.empty(need_ks - 1, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7).all()  # nothing ran
    # an exactly sized scratch is taken
    eng.boolean_gates_async(d_ops, dev(a), dev(b), d_out, 4, 1,
                            d_scratch=torch.empty(need, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy().view(U32), eng.boolean_gates(np.zeros(4, dtype=np.uint8), a, b, 1), "exact scratch")
    # an opcode above 5
    with pytest.raises(EngineError, match="not a gate opcode"):
        eng.boolean_gates([0, 6, 1, 2], a, b, 1)
    with pytest.raises(EngineError, match="pbs_order"):
        eng.boolean_gates([0, 1, 2, 3], a, b, 2)
    # count = 0 is a no-op
    empty = np.zeros((0, w), dtype=U32)
    assert eng.boolean_gates(np.zeros(0, dtype=np.uint8), empty, empty, 1).shape == (0, w)
    assert eng.boolean_mux(empty, empty, empty, 1).shape == (0, w)
    assert eng.programmable_bootstrap_u32(empty, np.zeros(1536, dtype=U32)).shape == (0, 1025)
    assert eng.keyswitch_u32(np.zeros((0, 1025), dtype=U32)).shape == (0, w)
    assert eng.boolean_gates_scratch_bytes(0, 1) == 0
    eng.close()
