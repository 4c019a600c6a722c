"""Guard-band tests of the device-pointer (_async) entry points of include/tfhe_mi355.h.

The parity tests pin WHAT the kernels compute; this file pins WHERE they write.  Every buffer of a call
is a region of one guarded arena (tests/guarded_arena.py): pseudo-random guard bands around every
region, every region at an address that is 16 modulo 256 (the alignment the header documents), the
scratch of exactly the size the matching *_scratch query returns.  For every case:

  1. the output region equals the synchronous host-pointer twin on the same inputs, word for word, and
     for the PBS families at most 8 sampled rows (crafted and edge rows among them) also equal the oracle
     or the restated reference;
  2. arena.check() is empty: no guard band changed, and inputs, LUTs, index and opcode arrays, Fourier
     GGSW lists and key sources are bit-identical to before;
  3. the scratch region has exactly the queried size (where the query is 0, d_scratch is None);
  4. the call runs twice with the guards, the output and the scratch refilled with another random stream
     in between (in-place operands restored): both outputs are identical;
  5. the resident keys of an engine (the _fourier / _device hand-outs) read back equal before its first
     and after its last case.

The lut-index clamp rides on the same cases: every LUT region holds lut_count = 2 LUTs followed by two
decoy LUTs of other random words, the index arrays hold 0 .. 3, and the twin is computed with the indexes
clamped to 1 -- a kernel that does not clamp reads a decoy (still inside the arena) and differs.

Keys are uniform random words (exactness needs no valid key), LWE dimensions 1 .. 3; the kernel form is
chosen by `count` alone and asserted through the engine's kernel timer; no TFHE_MI355_* variable is set.
"""
import ctypes
import dataclasses
from types import SimpleNamespace as NS

import numpy as np
import pytest

from guarded_arena import GuardedArena

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32
ONES = U64((1 << 64) - 1)
P = "tfhe_mi355_"

# entry points with no guarded case: {name: reason}
EXCLUDED = {}

CASES = []


def case(cid, engine, entries):
    """register build(E, orc) -> spec as the guarded case `cid` of engine `engine` for the entry points"""
    def deco(build):
        CASES.append(NS(id=cid, engine=engine, entries=tuple(P + e for e in entries), build=build))
        return build
    return deco


def covered_entry_points():
    out = {}
    for c in CASES:
        for e in c.entries:
            out.setdefault(e, []).append(c.id)
    return out


# ---- small helpers --------------------------------------------------------------------------------------
def _cus():
    """Compute units of device 0: the kernel-form thresholds of capi_pbs.cpp scale with it."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _rand64(seed, *shape):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=U64)


def _rand32(seed, *shape):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=U32)


def _read_device(ptr, nbytes):
    import torch

    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
    return out


def _rin(name, data, row=None):
    """a read-only region holding `data`"""
    data = np.ascontiguousarray(data)
    return NS(name=name, nbytes=data.nbytes, data=data, writable=False, row=row or data.nbytes)


def _rout(name, nbytes, row=None, data=None):
    """a writable region: the output, an in-place operand (with data) or the scratch"""
    return NS(name=name, nbytes=int(nbytes), data=None if data is None else np.ascontiguousarray(data), writable=True,
              row=row or int(nbytes))


def _spec(regions, call, twin, out, scratch, kernels, oracle=None, out_row=None):
    """regions: the arena's declaration, in address order; call(v): the async call on the views v[name];
    twin(): the expected bytes of region `out` (an array); scratch: (region name or None, the queried
    size); kernels: timer families that must have run (None: the entry point has no timer family);
    oracle(): (rows, expected [rows][words]) of the sampled rows from a reference of its own.
    A case may set spec.primary afterwards: the region holding its primary ciphertext input, where that is not
    the first read-only ciphertext region (tests/test_async_graph_gpu.py changes it between replays)."""
    return NS(regions=regions, call=call, twin=twin, out=out, scratch=scratch, kernels=kernels, oracle=oracle,
              out_row=out_row)


def _sample(count):
    return np.unique(np.clip([0, 1, 2, 3, 4, count // 2, count - 2, count - 1], 0, count - 1))


def _clamp_indexes(count):
    """lut indexes 0 .. 3 over lut_count = 2 LUTs (2 and 3 must be clamped to 1); rows 0 .. 2 of a batch
    of at least five keep LUT 0 (the crafted LUT).  Returns (device array, clamped array)."""
    idx = ((np.arange(count) + 3) % 4).astype(np.uint32)
    if count >= 5:
        idx[:3] = 0
    return idx, np.minimum(idx, 1).astype(np.uint32)


# ---- engines ----------------------------------------------------------------------------------------------
ENGINES = {}   # key -> holder, created on first use
FACTORIES = {}


def engine_factory(key):
    def deco(fn):
        FACTORIES[key] = fn
        return fn
    return deco


def _snapshot(E):
    """the resident key buffers the ABI hands out, read back; the matching _set_ready keeps the engine
    usable (a u32 context hands its Fourier key out for reading only)."""
    snap = {}
    if E.has.get("bsk"):
        snap["fourier"] = _read_device(*E.eng.fourier_bootstrap_key())
        if E.width == 64:
            E.eng.fourier_bootstrap_key_set_ready()
    if E.has.get("ksk") and E.width == 64:
        snap["ksk"] = _read_device(*E.eng.keyswitch_key_device())
        E.eng.keyswitch_key_set_ready()
    return snap


def _engine(key, orc):
    if key not in ENGINES:
        E = FACTORIES[key](orc)
        E.key = key
        E.snapshot = _snapshot(E)
        ENGINES[key] = E
    return ENGINES[key]


def _check_keys_and_close(key):
    E = ENGINES.pop(key)
    try:
        after = _snapshot(E)
        assert set(after) == set(E.snapshot)
        for part, before in E.snapshot.items():
            bad = np.flatnonzero(after[part] != before)
            assert bad.size == 0, f"engine {key}: resident {part} key changed, bytes {bad[0]} .. {bad[-1]}"
    finally:
        E.eng.close()


def _pbs_params(N, k, L, B, n, g=0, ksB=3, ksL=5):
    from tfhe_mi355.parameters import ClassicPBSParameters

    return ClassicPBSParameters(lwe_dimension=n, glwe_dimension=k, polynomial_size=N, lwe_modular_std_dev=2.0 ** -20,
                                glwe_modular_std_dev=2.0 ** -50, pbs_base_log=B, pbs_level=L, ks_base_log=ksB,
                                ks_level=ksL, message_modulus=4, carry_modulus=4, grouping_factor=g,
                                name=f"guard_N{N}_k{k}_L{L}_B{B}_n{n}_g{g}")


def _pbs_engine(orc, N, k, L, B, n, g=0, ks=False):
    """a u64 PBS engine under a bootstrapping key of random words (and a random keyswitching key)"""
    from tfhe_mi355 import Engine

    p = _pbs_params(N, k, L, B, n, g)
    words = (n // g) * (1 << g) if g else n
    bsk = _rand64(N + 31 * k + L + B + g, words * L * (k + 1) * (k + 1) * N)
    eng = Engine(p, 0)
    eng.upload_bootstrap_key(bsk)
    E = NS(eng=eng, p=p, bsk=bsk, ksk=None, has={"bsk": True}, width=64, g=g, orc=orc, _fb=None)
    if ks:
        E.ksk = _rand64(N + 7, k * N * p.ks_level * (n + 1))
        eng.upload_keyswitch_key(E.ksk)
        E.has["ksk"] = True
    return E


def _fourier_oracle(E):
    if E._fb is None:
        p, O = E.p, E.orc
        args = (E.bsk, p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.pbs_base_log, p.pbs_level)
        E._fb = O.MultiBitFourierBsk(*args, E.g) if E.g else O.FourierBsk(*args)
    return E._fb


PBS_ENGINES = {
    # key: (N, k, L, B, n, g, ks)
    "c2048": (2048, 1, 1, 23, 2, 0, True),
    "c1024": (1024, 1, 2, 15, 2, 0, False),
    "c256": (256, 5, 1, 15, 2, 0, False),
    "c512": (512, 3, 1, 18, 2, 0, False),
    "mb3": (2048, 1, 1, 21, 3, 3, False),
    "mb2": (2048, 1, 1, 22, 2, 2, False),
    "mb512": (512, 3, 1, 18, 2, 2, False),
    "mb8192": (8192, 1, 2, 14, 3, 3, False),
    "l4096": (4096, 1, 1, 22, 2, 0, True),
    "l8192": (8192, 1, 2, 15, 2, 0, False),
    "l16384": (16384, 1, 3, 15, 1, 0, False),
    "l32768": (32768, 1, 2, 15, 1, 0, False),
}
for _key, _a in PBS_ENGINES.items():
    FACTORIES[_key] = (lambda a: lambda orc: _pbs_engine(orc, a[0], a[1], a[2], a[3], a[4], a[5], a[6]))(_a)


# ---- the u64 PBS families ---------------------------------------------------------------------------------
def _pbs_inputs(E, form, count, seed):
    """(rows, the four LUTs: two live, two decoys): the crafted triple in front under the crafted LUT (the
    edge LUT for multi-bit, whose external products take the accumulator itself), an all-zero mask, an
    all-ones body; KS -> PBS rows are keyswitched first, so they are random and edge words only."""
    from pbs_edge_inputs import crafted_case, pbs_edge_words, unit_mask

    p = E.p
    N, k, n, B, L = p.polynomial_size, p.glwe_dimension, p.lwe_dimension, p.pbs_base_log, p.pbs_level
    w_in = (k * N if form == "kspbs" else n) + 1
    cts = _rand64(seed, count, w_in)
    luts = _rand64(seed + 1, 4, (k + 1) * N)
    if E.g:
        luts[0] = np.concatenate([pbs_edge_words(B, L, N, seed=seed + r) for r in range(k + 1)])
        cts[:3, -1] = [0, 1 << 63, (1 << 64) - 1][:min(count, 3)]
    elif form != "kspbs":
        luts[0] = crafted_case(B, L, N, k, seed=seed)[1]
        cts[:3, 0] = unit_mask(N)
        cts[:3, -1] = [0, 1 << 63, (1 << 64) - 1][:min(count, 3)]
    if count > 3:
        cts[3, :-1] = 0
    if count > 4:
        cts[4, -1] = ONES
    return cts, luts


def _pbs_case(form, count, kernels, scratch_cts=None, seed=1):
    """form: pbs | rot | kspbs | pbsks.  scratch_cts (N >= 4096): scratch for that many ciphertexts,
    pbs_scratch_bytes(1) each, the documented "less scratch runs smaller passes" contract."""
    def build(E, orc):
        eng, p = E.eng, E.p
        N, k, n = p.polynomial_size, p.glwe_dimension, p.lwe_dimension
        cnt = count(_cus()) if callable(count) else count
        cts, luts = _pbs_inputs(E, form, cnt, seed + cnt)
        idx, idxc = _clamp_indexes(cnt)
        w_out = {"pbs": k * N + 1, "rot": (k + 1) * N, "kspbs": k * N + 1, "pbsks": n + 1}[form]
        if form == "rot":
            need = 0
        elif scratch_cts is not None:
            m = scratch_cts(_cus()) if callable(scratch_cts) else scratch_cts
            need = eng.pbs_scratch_bytes(1) * m
            assert m >= cnt or need < eng.pbs_scratch_bytes(cnt), "the case means to give less than the query"
        else:
            need = {"pbs": eng.pbs_scratch_bytes, "kspbs": eng.ks_pbs_scratch_bytes,
                    "pbsks": eng.pbs_ks_scratch_bytes}[form](cnt)
        regions = [_rin("lwe_in", cts, row=cts.shape[1] * 8), _rin("lut_indexes", idx, row=4),
                   _rout("out", cnt * w_out * 8, row=w_out * 8), _rin("luts", luts, row=luts.shape[1] * 8)]
        if need:
            regions.insert(3, _rout("scratch", need, row=min(need, max(256, need // max(cnt, 1)))))

        def call(v):
            s = v.get("scratch")
            if form == "pbs":
                eng.programmable_bootstrap_async(v["lwe_in"], v["out"], v["luts"], 2, cnt, v["lut_indexes"], d_scratch=s)
            elif form == "rot":
                eng.blind_rotate_async(v["lwe_in"], v["out"], v["luts"], 2, cnt, v["lut_indexes"])
            elif form == "kspbs":
                eng.keyswitch_programmable_bootstrap_async(v["lwe_in"], v["out"], v["luts"], 2, cnt, d_scratch=s,
                                                           d_lut_indexes=v["lut_indexes"])
            else:
                eng.programmable_bootstrap_keyswitch_async(v["lwe_in"], v["out"], v["luts"], 2, cnt, d_scratch=s,
                                                           d_lut_indexes=v["lut_indexes"])

        host = {"pbs": eng.programmable_bootstrap, "rot": eng.blind_rotate,
                "kspbs": eng.keyswitch_programmable_bootstrap, "pbsks": eng.programmable_bootstrap_keyswitch}[form]

        def oracle():
            rows = _sample(cnt)
            fb = _fourier_oracle(E)
            x = cts[rows]
            ks = lambda a: orc.keyswitch(E.ksk, k * N, n, p.ks_base_log, p.ks_level, a)  # noqa: E731
            if form == "kspbs":
                x = ks(x)
            run = fb.blind_rotate if form == "rot" and not E.g else fb.pbs
            y = run(x, luts[:2], idxc[rows], threads=8)
            return rows, ks(y) if form == "pbsks" else y

        spec = _spec(regions, call, lambda: host(cts, luts[:2], idxc), "out", ("scratch" if need else None, need),
                     kernels, oracle, out_row=w_out * 8)
        if form == "rot" and E.g:  # the oracle has no multi-bit blind rotation: its PBS is the extracted sample
            from ggsw_reference import Ref

            spec.oracle_post = lambda got: Ref(None, k, N, 0, 0).sample_extract(got.view(U64))
        return spec
    return build


def _lat(cus):
    return 3 * cus  # capi_pbs.cpp latency_max, classic


# classic N <= 2048: programmable_bootstrap_async and blind_rotate_async
for _form, _entry in (("pbs", "programmable_bootstrap_async"), ("rot", "blind_rotate_async")):
    for _cnt, _kern, _tag in ((1, "pbs_latency_kernel", "1"), (5, "pbs_latency_kernel", "5"),
                              (lambda cus: _lat(cus) + 77, "pbs_classic_kernel", "lat+77")):
        case(f"classic-2048_1_1-{_form}-{_tag}", "c2048", [_entry])(_pbs_case(_form, _cnt, {_kern}))
    for _key, _counts in (("c1024", (1, 19, 1100)), ("c256", (1, 19, 1100)), ("c512", (1, 19))):
        for _cnt in _counts:
            case(f"classic-{_key[1:]}-{_form}-{_cnt}", _key, [_entry])(_pbs_case(_form, _cnt, {"pbs_classic_kernel"}))

# multi-bit
for _cnt, _kern, _tag in ((1, "pbs_mb_latency_kernel", "1"), (5, "pbs_mb_latency_kernel", "5"),
                          (lambda cus: 2 * cus + 13, "pbs_multibit", "2cus+13")):
    case(f"multibit-2048-g3-pbs-{_tag}", "mb3", ["programmable_bootstrap_async"])(_pbs_case("pbs", _cnt, {_kern}))
case("multibit-2048-g3-rot-5", "mb3", ["blind_rotate_async"])(_pbs_case("rot", 5, {"pbs_mb_latency_kernel"}))
case("multibit-2048-g2-pbs-19", "mb2", ["programmable_bootstrap_async"])(_pbs_case("pbs", 19, {"pbs_mb_latency_kernel"}))
for _cnt in (1, 19):
    case(f"multibit-512_3-g2-pbs-{_cnt}", "mb512", ["programmable_bootstrap_async"])(
        _pbs_case("pbs", _cnt, {"pbs_multibit"}))
case("multibit-8192-g3-pbs-3-scratch2", "mb8192", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 3, {"large_mb_pair2_kernel"}, scratch_cts=2))


def _quad(cus):
    return cus // 2   # capi_pbs.cpp quad_max at N = 4096


def _onchip(cus):
    return cus * 5 // 8  # capi_pbs.cpp onchip_min at N = 4096


# classic N >= 4096: scratch = pbs_scratch_bytes(1) x m
case("large-4096-quad-1-scratch7", "l4096", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 1, {"quad_cmux_kernel"}, scratch_cts=7))
case("large-4096-quad-7-scratch7", "l4096", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 7, {"quad_cmux_kernel"}, scratch_cts=7))
case("large-4096-split-Q+5", "l4096", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", lambda cus: _quad(cus) + 5, {"large_sub_kernel"}, scratch_cts=lambda cus: _quad(cus) + 5))
case("large-4096-onchip-O+3", "l4096", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", lambda cus: _onchip(cus) + 3, {"onchip_cmux_kernel"}))
case("large-8192-5-scratch2", "l8192", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 5, {"quad_cmux_kernel"}, scratch_cts=2))
case("large-16384-3-scratch2", "l16384", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 3, {"large_sub_kernel"}, scratch_cts=2))
case("large-32768-7-scratch3", "l32768", ["programmable_bootstrap_async"])(
    _pbs_case("pbs", 7, {"large_group_cmux_kernel"}, scratch_cts=3))

# KS -> PBS and PBS -> KS
for _form, _entry in (("kspbs", "keyswitch_programmable_bootstrap_async"),
                      ("pbsks", "programmable_bootstrap_keyswitch_async")):
    for _cnt in (1, 67):
        case(f"{_form}-2048-{_cnt}", "c2048", [_entry])(_pbs_case(_form, _cnt, {"keyswitch", "pbs_latency_kernel"}))
    case(f"{_form}-4096-3", "l4096", [_entry])(_pbs_case(_form, 3, {"keyswitch", "quad_cmux_kernel"}))


# ---- keyswitch, packing keyswitch, GLWE x polynomial products (N = 512, k = 1) ------------------------
@engine_factory("ks512")
def _ks512(orc):
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P22

    N, k, n, B, L = 512, 1, 63, 3, 5
    p = P22.with_(glwe_dimension=k, polynomial_size=N, lwe_dimension=n, ks_base_log=B, ks_level=L, pbs_level=1,
                  name="guard_ks512")
    eng = Engine(p, 0)
    E = NS(eng=eng, p=p, has={"ksk": True}, width=64, ksk=_rand64(11, k * N * L * (n + 1)))
    eng.upload_keyswitch_key(E.ksk)
    eng.upload_packing_keyswitch_key(_rand64(12, k * N * L * (k + 1) * N), B, L)
    eng.upload_relinearization_key(_rand64(13, 1, 4, (k + 1) * N), 6, 4)
    E.key_mfma = eng.keyswitch_key(_rand64(14, 512 * 5 * 130), 512, 129, 3, 5)   # the int8-MFMA arm
    E.key_wide = eng.keyswitch_key(_rand64(15, 512 * 3 * 71), 512, 70, 9, 3)    # base_log > 7: the wide scalar arm
    return E


def _ks_rows(count, words, B, L, seed):
    from test_keyswitch_reference import HEAVY_NEG, edge_rows

    x = edge_rows(B, L, words, count, seed=seed)
    return np.ascontiguousarray(x[HEAVY_NEG:HEAVY_NEG + 1] if count == 1 else x[:count])  # one row: a heavy one


def _simple(eng_call, host, ins, out_words, count, need, kernels, dtype=U64, inplace=None):
    """a case with read-only inputs `ins` [(name, array, row bytes)], one output of count x out_words and an
    optional scratch"""
    item = np.dtype(dtype).itemsize
    regions = [_rin(name, a, row) for name, a, row in ins]
    regions.append(_rout("out", count * out_words * item, row=out_words * item, data=inplace))
    if need:
        regions.append(_rout("scratch", need))
    return _spec(regions, eng_call, host, "out", ("scratch" if need else None, need), kernels, out_row=out_words * item)


for _cnt in (1, 67):
    @case(f"keyswitch-512-{_cnt}", "ks512", ["keyswitch_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        x = _ks_rows(cnt, 513, 3, 5, seed=cnt)
        need = eng.ks_scratch_bytes(cnt)
        assert need > 0  # the int8-MFMA arm
        return _simple(lambda v: eng.keyswitch_async(v["lwe_in"], v["out"], cnt, d_scratch=v["scratch"]),
                       lambda: eng.keyswitch(x), [("lwe_in", x, 513 * 8)], 64, cnt, need, {"keyswitch"})

    for _which in ("mfma", "wide"):
        @case(f"keyswitch_with_key-{_which}-{_cnt}", "ks512", ["keyswitch_with_key_async"])
        def _b(E, orc, cnt=_cnt, which=_which):
            eng, key = E.eng, getattr(E, "key_" + which)
            x = _ks_rows(cnt, key.in_dim + 1, key.base_log, key.level, seed=cnt + 2)
            need = eng.keyswitch_with_key_scratch_bytes(key, cnt)
            assert (need > 0) == (which == "mfma")
            return _simple(lambda v: eng.keyswitch_with_key_async(key, v["lwe_in"], v["out"], cnt,
                                                                  d_scratch=v.get("scratch")),
                           lambda: eng.keyswitch_with_key(key, x), [("lwe_in", x, (key.in_dim + 1) * 8)],
                           key.out_dim + 1, cnt, need, {"keyswitch"})

    @case(f"packing_keyswitch-512-{_cnt}", "ks512", ["packing_keyswitch_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        x = _ks_rows(cnt, 513, 3, 5, seed=cnt + 4)
        need = eng.pks_scratch_bytes(cnt)
        assert need > 0
        return _simple(lambda v: eng.packing_keyswitch_async(v["lwe_in"], v["out"], cnt, d_scratch=v["scratch"]),
                       lambda: eng.packing_keyswitch(x), [("lwe_in", x, 513 * 8)], 1024, cnt, need, None)

    for _extract in (False, True):
        @case(f"glwe_poly_mul-512-{'extract' if _extract else 'glwe'}-{_cnt if _cnt == 1 else 5}", "ks512",
              ["glwe_poly_mul_async"])
        def _b(E, orc, cnt=1 if _cnt == 1 else 5, extract=_extract):
            eng = E.eng
            g, v_ = _rand64(20 + cnt, cnt, 2, 1024), _rand64(21 + cnt, 3, 2, 512)  # dense polynomials
            w = 513 if extract else 1024
            spec = _simple(lambda v: eng.glwe_poly_mul_async(v["glwe_in"], 2, v["polys"], 3, cnt, extract, v["out"]),
                           lambda: eng.glwe_poly_mul(g, v_, extract),
                           [("glwe_in", g, 1024 * 8), ("polys", v_, 512 * 8)], 3 * w, cnt, 0, None)
            spec.out_row = w * 8
            return spec

    @case(f"lwe_mult-512-{_cnt if _cnt == 1 else 5}", "ks512", ["lwe_mult_async"])
    def _b(E, orc, cnt=1 if _cnt == 1 else 5):
        eng = E.eng
        lhs, rhs = _mult_rows(cnt, 513, 30 + cnt)
        need = eng.lwe_mult_scratch_bytes(cnt)
        return _simple(lambda v: eng.lwe_mult_async(v["lhs"], v["rhs"], 4, v["out"], cnt, d_scratch=v["scratch"]),
                       lambda: eng.lwe_mult(lhs, rhs, 4), [("lhs", lhs, 513 * 8), ("rhs", rhs, 513 * 8)], 513, cnt, need,
                       {"packing_keyswitch", "glwe_tensor", "glwe_relin"})


def _mult_rows(count, words, seed):
    """random; lhs all zero; both all ones; both 1 << 63; all ones times random"""
    lhs, rhs = np.random.default_rng(seed).integers(0, 1 << 64, (2, max(count, 5), words), dtype=U64)
    if count > 1:
        lhs[1] = 0
        lhs[2] = rhs[2] = ONES
        lhs[3] = rhs[3] = U64(1 << 63)
        lhs[4] = ONES
    return np.ascontiguousarray(lhs[:count]), np.ascontiguousarray(rhs[:count])


@engine_factory("mult1024")
def _mult1024(orc):
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P22

    eng = Engine(P22.with_(glwe_dimension=1, polynomial_size=1024, pbs_level=1, name="guard_mult1024"), 0)
    eng.upload_relinearization_key(_rand64(41, 1, 4, 2048), 6, 4)
    return NS(eng=eng, has={}, width=64)


for _cnt in (1, 5):
    for _extract in (False, True):
        @case(f"glwe_mult-1024-{'extract' if _extract else 'glwe'}-{_cnt}", "mult1024", ["glwe_mult_async"])
        def _b(E, orc, cnt=_cnt, extract=_extract):
            eng = E.eng
            lhs, rhs = _mult_rows(cnt, 2048, 50 + cnt)
            need = eng.glwe_mult_scratch_bytes(cnt)
            return _simple(lambda v: eng.glwe_mult_async(v["lhs"], v["rhs"], 4, extract, v["out"], cnt,
                                                         d_scratch=v["scratch"]),
                           lambda: eng.glwe_mult(lhs, rhs, 4, extract), [("lhs", lhs, 2048 * 8), ("rhs", rhs, 2048 * 8)],
                           1025 if extract else 2048, cnt, need, {"glwe_tensor", "glwe_relin"})


# ---- GGSW layer at (2048, 1, 5, 3) ------------------------------------------------------------------------
GG = NS(N=2048, k=1, B=5, L=3, glwe=4096)
GG_IDX = np.array([4, 2, 2, 0, 3], dtype=np.uint32)  # permuted, repeating


@engine_factory("ggsw")
def _ggsw(orc):
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P22

    eng = Engine(P22.with_(glwe_dimension=GG.k, polynomial_size=GG.N, pbs_level=1, name="guard_ggsw"), 0)
    return NS(eng=eng, has={}, width=64, fourier={})


def _ggsw_std(count, seed):
    return _rand64(seed, count, GG.L * (GG.k + 1) * GG.glwe)


def _fourier_unguarded(E, g):
    """the Fourier list of g from a plain torch allocation (the twin of ggsw_list_convert_async, which
    has no host-pointer form; the host-pointer GGSW calls convert inside the library)"""
    import torch

    d_std = torch.from_numpy(g.view(np.int64)).cuda()
    d_f = torch.empty(E.eng.ggsw_list_fourier_bytes(g.shape[0], GG.L), dtype=torch.uint8, device="cuda")
    E.eng.ggsw_list_convert_async(d_std, g.shape[0], GG.L, d_f)
    torch.cuda.synchronize()
    return d_f.cpu().numpy()


for _cnt in (1, 5):
    @case(f"ggsw_list_convert-{_cnt}", "ggsw", ["ggsw_list_convert_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        g = _ggsw_std(cnt, 60 + cnt)
        nbytes = eng.ggsw_list_fourier_bytes(cnt, GG.L)
        assert nbytes == cnt * GG.L * (GG.k + 1) ** 2 * (GG.N // 2) * 16
        regions = [_rin("ggsw", g, g.shape[1] * 8), _rout("out", nbytes, row=nbytes // cnt)]
        return _spec(regions, lambda v: eng.ggsw_list_convert_async(v["ggsw"], cnt, GG.L, v["out"]),
                     lambda: _fourier_unguarded(E, g), "out", (None, 0), {"ggsw_to_fourier"}, out_row=nbytes // cnt)

    @case(f"ggsw_external_product-{_cnt}", "ggsw", ["ggsw_external_product_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        g = _ggsw_std(5, 65)
        idx = GG_IDX[:cnt].copy()
        d, inout = _rand64(66 + cnt, cnt, GG.glwe), _rand64(67 + cnt, cnt, GG.glwe)
        if cnt > 1:
            d[0] = 0
            d[1] = ONES
        regions = [_rin("fourier", _fourier_unguarded(E, g), row=g.shape[1] * 8), _rin("indexes", idx, row=4),
                   _rin("glwe_in", d, GG.glwe * 8), _rout("out", inout.nbytes, row=GG.glwe * 8, data=inout)]
        return _spec(regions, lambda v: eng.ggsw_external_product_async(v["fourier"], 5, GG.B, GG.L, v["glwe_in"],
                                                                        v["out"], cnt, v["indexes"]),
                     lambda: eng.ggsw_external_product(g, GG.B, GG.L, d, inout.copy(), idx), "out", (None, 0),
                     {"ggsw_external_product"}, out_row=GG.glwe * 8)

    @case(f"ggsw_cmux-{_cnt}", "ggsw", ["ggsw_cmux_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        g = _ggsw_std(5, 65)
        idx = GG_IDX[:cnt].copy()
        ct0, ct1 = _rand64(68 + cnt, cnt, GG.glwe), _rand64(69 + cnt, cnt, GG.glwe)
        if cnt > 1:
            ct1[0] = ct0[0]
            ct0[1], ct1[1] = 0, ONES
        regions = [_rin("fourier", _fourier_unguarded(E, g), row=g.shape[1] * 8), _rin("indexes", idx, row=4),
                   _rin("ct0", ct0, GG.glwe * 8), _rin("ct1", ct1, GG.glwe * 8),
                   _rout("out", ct0.nbytes, row=GG.glwe * 8)]
        return _spec(regions, lambda v: eng.ggsw_cmux_async(v["fourier"], 5, GG.B, GG.L, v["ct0"], v["ct1"], v["out"],
                                                            cnt, v["indexes"]),
                     lambda: eng.ggsw_cmux(g, GG.B, GG.L, ct0, ct1, idx), "out", (None, 0), {"ggsw_cmux"},
                     out_row=GG.glwe * 8)

    @case(f"vertical_packing-{min(_cnt, 3)}", "ggsw", ["vertical_packing_async"])
    def _b(E, orc, cnt=min(_cnt, 3)):
        """three tree bits, two rotation bits; lut_count = 2 with two decoys behind, indexes up to 3"""
        eng = E.eng
        nbits, npoly = 5, 8
        g = _ggsw_std(cnt * nbits, 70 + cnt).reshape(cnt, nbits, -1)
        luts = _rand64(71 + cnt, 4, npoly, GG.N)
        idx = np.array([3, 0, 2], dtype=np.uint32)[:cnt]
        idxc = np.minimum(idx, 1).astype(np.uint32)
        need = eng.vertical_packing_scratch_bytes(npoly, cnt)
        w = GG.k * GG.N + 1
        regions = [_rin("fourier", _fourier_unguarded(E, g.reshape(cnt * nbits, -1)), row=g.shape[2] * 8),
                   _rin("luts", luts, row=npoly * GG.N * 8), _rin("lut_indexes", idx, row=4),
                   _rout("out", cnt * w * 8, row=w * 8), _rout("scratch", need, row=GG.glwe * 8)]
        return _spec(regions, lambda v: eng.vertical_packing_async(v["fourier"], GG.B, GG.L, nbits, v["luts"], 2, npoly,
                                                                   cnt, v["out"], v["lut_indexes"], d_scratch=v["scratch"]),
                     lambda: eng.vertical_packing(g, GG.B, GG.L, luts[:2], idxc), "out", ("scratch", need),
                     {"ggsw_cmux_tree", "ggsw_rotate_chain"}, out_row=w * 8)


# ---- WoP-PBS at the smallest pfpks shape (512, 1, 7, 6), n = 3 --------------------------------------------
WOP = NS(N=512, k=1, n=3, B=10, L=2, ksB=3, ksL=5, pfB=7, pfL=6, cbsB=5, cbsL=3, glwe=1024, big=512)


@engine_factory("wop512")
def _wop512(orc):
    E = _pbs_engine(orc, WOP.N, WOP.k, WOP.L, WOP.B, WOP.n, ks=True)
    E.eng.upload_pfpksk_list(_rand64(81, (WOP.k + 1) * (WOP.big + 1) * WOP.pfL * WOP.glwe), WOP.pfB, WOP.pfL)
    return E


for _cnt in (1, 3):
    @case(f"pfpks-512-{_cnt}", "wop512", ["private_functional_packing_keyswitch_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        x = _ks_rows(cnt, WOP.big + 1, WOP.pfB, WOP.pfL, seed=cnt + 6)
        need = eng.pfpks_scratch_bytes(cnt)
        assert need > 0
        return _simple(lambda v: eng.private_functional_packing_keyswitch_async(v["lwe_in"], v["out"], cnt,
                                                                               d_scratch=v["scratch"]),
                       lambda: eng.private_functional_packing_keyswitch(x), [("lwe_in", x, (WOP.big + 1) * 8)],
                       (WOP.k + 1) * WOP.glwe, cnt, need, {"pfpks_mfma"})

    @case(f"extract_bits-512-{_cnt}", "wop512", ["extract_bits_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        x = _rand64(82 + cnt, cnt, WOP.big + 1)
        need = eng.extract_bits_scratch_bytes(cnt)
        return _simple(lambda v: eng.extract_bits_async(v["lwe_in"], 60, 4, v["out"], cnt, d_scratch=v["scratch"]),
                       lambda: eng.extract_bits(x, 60, 4), [("lwe_in", x, (WOP.big + 1) * 8)], 4 * (WOP.n + 1), cnt, need,
                       {"pbs_classic_kernel", "keyswitch", "wop_glue"})

    @case(f"circuit_bootstrap-512-{_cnt}", "wop512", ["circuit_bootstrap_async"])
    def _b(E, orc, cnt=_cnt):
        eng = E.eng
        x = _rand64(84 + cnt, cnt, WOP.n + 1)
        need = eng.circuit_bootstrap_scratch_bytes(WOP.cbsL, cnt)
        return _simple(lambda v: eng.circuit_bootstrap_async(v["lwe_in"], 60, WOP.cbsB, WOP.cbsL, v["out"], cnt,
                                                             d_scratch=v["scratch"]),
                       lambda: eng.circuit_bootstrap(x, 60, WOP.cbsB, WOP.cbsL), [("lwe_in", x, (WOP.n + 1) * 8)],
                       WOP.cbsL * (WOP.k + 1) * WOP.glwe, cnt, need, {"pbs_classic_kernel", "pfpks_mfma", "wop_glue"})

    @case(f"circuit_bootstrap_vertical_packing-512-{_cnt}", "wop512", ["circuit_bootstrap_vertical_packing_async"])
    def _b(E, orc, cnt=_cnt):
        """the composed call: scratch = [standard GGSWs | Fourier GGSWs | max(cbs, vertical packing)]; one
        tree bit and three rotation bits, two outputs, lut_count = 2 with two decoys behind"""
        eng = E.eng
        nbits, nout, npoly = 4, 2, 2
        x = _rand64(86 + cnt, cnt, nbits, WOP.n + 1)
        luts = _rand64(87 + cnt, 4, nout, npoly, WOP.N)
        idx = np.array([3, 0, 2], dtype=np.uint32)[:cnt]
        idxc = np.minimum(idx, 1).astype(np.uint32)
        need = eng.circuit_bootstrap_vertical_packing_scratch_bytes(nbits, WOP.cbsL, 2, nout, npoly, cnt)
        w = WOP.big + 1
        regions = [_rin("lwe_in", x, row=(WOP.n + 1) * 8), _rin("luts", luts, row=nout * npoly * WOP.N * 8),
                   _rin("lut_indexes", idx, row=4), _rout("out", cnt * nout * w * 8, row=w * 8),
                   _rout("scratch", need, row=WOP.glwe * 8)]
        return _spec(regions, lambda v: eng.circuit_bootstrap_vertical_packing_async(
            v["lwe_in"], nbits, WOP.cbsB, WOP.cbsL, v["luts"], 2, nout, npoly, cnt, v["out"], v["lut_indexes"],
            d_scratch=v["scratch"]),
            lambda: eng.circuit_bootstrap_vertical_packing(x, WOP.cbsB, WOP.cbsL, luts[:2], idxc), "out",
            ("scratch", need), {"pbs_classic_kernel", "pfpks_mfma", "ggsw_to_fourier", "ggsw_cmux_tree",
                                "ggsw_rotate_chain"}, out_row=w * 8)


# ---- 32-bit torus: the two Boolean shapes with n = 3 ----------------------------------------------------
BOOL_SHAPES = {"bool512": (512, 2, 3, 6, 3, 4), "bool1024": (1024, 1, 3, 7, 2, 8)}  # N, k, L, B, ks B, ks L


def _bool_engine(orc, N, k, L, B, ksB, ksL):
    from boolean_reference import RefEngine32
    from tfhe_mi355 import Engine
    from tfhe_mi355 import boolean as Bm

    n = 3
    p = dataclasses.replace(Bm.DEFAULT_PARAMETERS, lwe_dimension=n, glwe_dimension=k, polynomial_size=N, pbs_base_log=B,
                            pbs_level=L, ks_base_log=ksB, ks_level=ksL, name=f"guard_bool_{N}_{k}")
    bsk = _rand32(N + k, n * L * (k + 1) * (k + 1) * N)
    ksk = _rand32(N + k + 1, k * N * ksL * (n + 1))
    eng, ref = Engine(p, 0), RefEngine32(p)
    for e in (eng, ref):
        e.upload_bootstrap_key_u32(bsk)
        e.upload_keyswitch_key_u32(ksk)
    return NS(eng=eng, p=p, ref=ref, has={"bsk": True, "ksk": True}, width=32)


for _key, _a in BOOL_SHAPES.items():
    FACTORIES[_key] = (lambda a: lambda orc: _bool_engine(orc, *a))(_a)


def _pbs32_case(glwe_out, count):
    def build(E, orc):
        from pbs_edge_inputs32 import crafted_case32, unit_mask32

        eng, p = E.eng, E.p
        N, k, n = p.polynomial_size, p.glwe_dimension, p.lwe_dimension
        cnt = count(eng) if callable(count) else count
        x = _rand32(90 + cnt, cnt, n + 1)
        luts = _rand32(91 + cnt, 4, (k + 1) * N)
        luts[0] = crafted_case32(p.pbs_base_log, p.pbs_level, N, k, seed=7)[1]
        x[:3, 0] = unit_mask32(N)
        x[:3, -1] = [0, 1 << 31, (1 << 32) - 1][:min(cnt, 3)]
        if cnt > 4:
            x[3, :-1] = 0
            x[4, -1] = (1 << 32) - 1
        idx, idxc = _clamp_indexes(cnt)
        w = (k + 1) * N if glwe_out else k * N + 1
        need = (eng.blind_rotate_u32_scratch_bytes if glwe_out else eng.pbs_u32_scratch_bytes)(cnt)
        fn = eng.blind_rotate_u32_async if glwe_out else eng.programmable_bootstrap_u32_async
        host, ref = ((eng.blind_rotate_u32, E.ref.blind_rotate_u32) if glwe_out
                     else (eng.programmable_bootstrap_u32, E.ref.programmable_bootstrap_u32))
        regions = [_rin("lwe_in", x, row=(n + 1) * 4), _rin("lut_indexes", idx, row=4), _rout("out", cnt * w * 4, row=w * 4),
                   _rin("luts", luts, row=luts.shape[1] * 4)]
        if need:
            regions.append(_rout("scratch", need))

        def oracle():
            rows = _sample(cnt)
            return rows, ref(x[rows], luts[:2], idxc[rows])

        return _spec(regions, lambda v: fn(v["lwe_in"], v["out"], v["luts"], 2, cnt, v["lut_indexes"],
                                           d_scratch=v.get("scratch")),
                     lambda: host(x, luts[:2], idxc), "out", ("scratch" if need else None, need),
                     {"pbs_classic32_kernel"}, oracle, out_row=w * 4)
    return build


def _gate_rows(E, count, pbs_order, seed):
    """three operands of `count` rows"""
    return _rand32(seed, 3, count, E.eng.gate_words(pbs_order))


for _key in BOOL_SHAPES:
    for _glwe, _entry in ((False, "programmable_bootstrap_u32_async"), (True, "blind_rotate_u32_async")):
        case(f"{_key}-{'rot' if _glwe else 'pbs'}-1", _key, [_entry])(_pbs32_case(_glwe, 1))
        case(f"{_key}-{'rot' if _glwe else 'pbs'}-resident+1", _key, [_entry])(
            _pbs32_case(_glwe, lambda eng: eng.pbs_u32_resident() + 1))
    for _cnt in (1, 67):
        @case(f"{_key}-keyswitch-{_cnt}", _key, ["keyswitch_u32_async"])
        def _b(E, orc, cnt=_cnt):
            eng, p = E.eng, E.p
            big = p.glwe_dimension * p.polynomial_size
            x = (_ks_rows(cnt, big + 1, p.ks_base_log, p.ks_level, seed=cnt + 8) >> U64(32)).astype(U32)
            need = eng.ks_u32_scratch_bytes(cnt)
            return _simple(lambda v: eng.keyswitch_u32_async(v["lwe_in"], v["out"], cnt, d_scratch=v.get("scratch")),
                           lambda: eng.keyswitch_u32(x), [("lwe_in", x, (big + 1) * 4)], p.lwe_dimension + 1, cnt, need,
                           {"keyswitch32"}, dtype=U32)
    for _order in (0, 1):
        for _cnt in (1, 6):
            @case(f"{_key}-gates-order{_order}-{_cnt}", _key, ["boolean_gates_async"])
            def _b(E, orc, cnt=_cnt, order=_order):
                eng = E.eng
                w = eng.gate_words(order)
                a, b, _ = _gate_rows(E, cnt, order, 100 + cnt + order)
                ops = (np.arange(cnt) % 6).astype(np.uint8) if cnt > 1 else np.array([4], dtype=np.uint8)
                need = eng.boolean_gates_scratch_bytes(cnt, order)
                spec = _simple(lambda v: eng.boolean_gates_async(v["ops"], v["lhs"], v["rhs"], v["out"], cnt, order,
                                                                 d_scratch=v.get("scratch")),
                               lambda: eng.boolean_gates(ops, a, b, order),
                               [("ops", ops, 1), ("lhs", a, w * 4), ("rhs", b, w * 4)], w, cnt, need,
                               {"pbs_classic32_kernel", "keyswitch32", "boolean_ops"}, dtype=U32)
                spec.oracle = lambda: (np.arange(cnt), E.ref.boolean_gates(ops, a, b, order))
                return spec

            @case(f"{_key}-mux-order{_order}-{_cnt}", _key, ["boolean_mux_async"])
            def _b(E, orc, cnt=_cnt, order=_order):
                eng = E.eng
                w = eng.gate_words(order)
                c, t, e = _gate_rows(E, cnt, order, 110 + cnt + order)
                need = eng.boolean_mux_scratch_bytes(cnt, order)
                spec = _simple(lambda v: eng.boolean_mux_async(v["cond"], v["then"], v["else"], v["out"], cnt, order,
                                                               d_scratch=v.get("scratch")),
                               lambda: eng.boolean_mux(c, t, e, order),
                               [("cond", c, w * 4), ("then", t, w * 4), ("else", e, w * 4)], w, cnt, need,
                               {"pbs_classic32_kernel", "keyswitch32", "boolean_ops"}, dtype=U32)
                spec.oracle = lambda: (np.arange(cnt), E.ref.boolean_mux(c, t, e, order))
                return spec

    @case(f"{_key}-not", _key, ["boolean_not_async"])
    def _b(E, orc):
        eng = E.eng
        w = eng.gate_words(1)
        x = _rand32(120, 6, w)
        x[0] = 0
        return _simple(lambda v: eng.boolean_not_async(v["in"], v["out"], 6 * w), lambda: (U32(0) - x).astype(U32),
                       [("in", x, w * 4)], w, 6, 0, {"boolean_ops"}, dtype=U32)


# ---- 128-bit torus ------------------------------------------------------------------------------------------
U128_SHAPES = {"u128-256": (256, 1, 1, 7), "u128-2048": (2048, 1, 1, 23)}  # the second: (k + 1) N = 4096


def _u128_engine(orc, N, k, L, B):
    import pbs128_cases as C
    import pbs128_reference as R
    from tfhe_mi355 import Engine

    n = 2
    p = C.params(n, N, k, L, B)
    bsk = R.uniform(N + k, n * L * (k + 1) * (k + 1) * N).reshape(n, L, k + 1, k + 1, N, 2)
    eng = Engine.for_u128(p, 0)
    eng.upload_bootstrap_key_u128(bsk)
    ref = R.RefEngine128(p)
    ref.upload_bootstrap_key_u128(bsk)
    # no resident-key read-back: the _fourier hand-out describes the 64-bit layout of the context's buffer
    return NS(eng=eng, p=p, ref=ref, has={}, width=128)


for _key, _a in U128_SHAPES.items():
    FACTORIES[_key] = (lambda a: lambda orc: _u128_engine(orc, *a))(_a)


def _pbs128_case(glwe_out, count):
    def build(E, orc):
        import pbs128_cases as C
        import pbs128_reference as R

        eng, p = E.eng, E.p
        N, k, n = p.polynomial_size, p.glwe_dimension, p.lwe_dimension
        cnt = count(eng) if callable(count) else count
        x = R.uniform(130 + cnt, cnt * (n + 1)).reshape(cnt, n + 1, 2)
        for row, rot in enumerate((0, N, 2 * N)):  # bodies switching to 0, N and 2N
            if row < cnt:
                x[row, n] = R.to_words([C.mask_for_rotation(rot, N) - (1 if rot == 2 * N else 0)])[0]
        if cnt > 3:
            x[3, :n] = 0
        luts = R.uniform(131 + cnt, 4 * (k + 1) * N).reshape(4, (k + 1) * N, 2)
        idx, idxc = _clamp_indexes(cnt)
        w = (k + 1) * N if glwe_out else k * N + 1
        need = (eng.blind_rotate_u128_scratch_bytes if glwe_out else eng.pbs_u128_scratch_bytes)(cnt)
        fn = eng.blind_rotate_u128_async if glwe_out else eng.programmable_bootstrap_u128_async
        host, ref = ((eng.blind_rotate_u128, E.ref.blind_rotate_u128) if glwe_out
                     else (eng.programmable_bootstrap_u128, E.ref.programmable_bootstrap_u128))
        regions = [_rin("lwe_in", x, row=(n + 1) * 16), _rin("lut_indexes", idx, row=4),
                   _rout("out", cnt * w * 16, row=w * 16), _rin("luts", luts, row=(k + 1) * N * 16)]
        if need:
            regions.append(_rout("scratch", need))

        def oracle():
            rows = _sample(cnt)
            return rows, ref(x[rows], luts[:2], idxc[rows])

        return _spec(regions, lambda v: fn(v["lwe_in"], v["out"], v["luts"], 2, cnt, d_lut_indexes=v["lut_indexes"],
                                           d_scratch=v.get("scratch")),
                     lambda: host(x, luts[:2], idxc), "out", ("scratch" if need else None, need), {"pbs_f128_kernel"},
                     oracle, out_row=w * 16)
    return build


for _glwe, _entry in ((False, "programmable_bootstrap_u128_async"), (True, "blind_rotate_u128_async")):
    _t = "rot" if _glwe else "pbs"
    case(f"u128-256-{_t}-1", "u128-256", [_entry])(_pbs128_case(_glwe, 1))
    case(f"u128-256-{_t}-resident+1", "u128-256", [_entry])(_pbs128_case(_glwe, lambda eng: eng.pbs_u128_resident() + 1))
    case(f"u128-2048-{_t}-1", "u128-2048", [_entry])(_pbs128_case(_glwe, 1))
    case(f"u128-2048-{_t}-5", "u128-2048", [_entry])(_pbs128_case(_glwe, 5))


# ---- key ingestion: only the source is in the arena, and it must stay as it was ---------------------------
@engine_factory("ingest")
def _ingest(orc):
    from tfhe_mi355 import Engine

    a = PBS_ENGINES["c2048"]
    return NS(eng=Engine(_pbs_params(a[0], a[1], a[2], a[3], a[4]), 0), has={}, width=64)


@case("bootstrap_key_convert", "ingest", ["bootstrap_key_convert_async"])
def _b(E, orc):
    """the Fourier key converted from the guarded source equals the one the host-pointer upload of the same
    words made (engine c2048)"""
    eng, ref = E.eng, _engine("c2048", orc)

    def converted():
        return _read_device(*eng.fourier_bootstrap_key())

    regions = [_rin("bsk", ref.bsk, row=2 * 2048 * 8)]
    spec = _spec(regions, lambda v: eng.convert_bootstrap_key_device(v["bsk"], ref.bsk.size), lambda: ref.snapshot["fourier"],
                 None, (None, 0), None)
    spec.result = converted
    return spec


@case("keyswitch_key_upload", "ingest", ["keyswitch_key_upload_async"])
def _b(E, orc):
    eng, ref = E.eng, _engine("c2048", orc)
    regions = [_rin("ksk", ref.ksk, row=3 * 8)]
    spec = _spec(regions, lambda v: eng.upload_keyswitch_key_device(v["ksk"], ref.ksk.size),
                 lambda: ref.ksk.view(np.uint8), None, (None, 0), None)
    spec.result = lambda: _read_device(*eng.keyswitch_key_device())
    return spec


# ---- the integer layer's glue: sentinel tests exist (test_lwe_ops_gpu.py); here the weak alignment and
# ---- the refill pass ----------------------------------------------------------------------------------------
WORDS = 743


for _scalar in (3, 2 ** 64 - 1):
    for _src in ("other", "own", None):
        @case(f"lwe_scalar_mul_add-{_scalar % 1000}-{_src}", "c2048", ["lwe_scalar_mul_add_async"])
        def _b(E, orc, scalar=_scalar, src=_src):
            """y = block 3 of [3 rows][5 blocks][743 words]; x = block 1 of a [3][4][743] tensor, block 0 of y's
            own tensor, or none; every other word of y's tensor stays"""
            eng = E.eng
            Y, X = _rand64(140, 3, 5, WORDS), _rand64(141, 3, 4, WORDS)
            exp = Y.copy()
            exp[:, 3] = Y[:, 3] * U64(scalar) + (X[:, 1] if src == "other" else Y[:, 0] if src == "own" else U64(0))

            def call(v):
                y = v["out"].data_ptr()
                xp, xs = {"other": (v["x"].data_ptr() + 8 * WORDS, 4 * WORDS), "own": (y, 5 * WORDS), None: (None, 0)}[src]
                eng.lwe_scalar_mul_add_async(y + 8 * 3 * WORDS, xp, scalar, 3, WORDS, 5 * WORDS, xs)

            regions = [_rin("x", X, row=WORDS * 8), _rout("out", Y.nbytes, row=WORDS * 8, data=Y)]
            spec = _spec(regions, call, lambda: exp, "out", (None, 0), None, out_row=5 * WORDS * 8)
            if src != "other":  # x is not read here: the ciphertext input is y's own tensor
                spec.primary = "out"
            return spec


@case("trivial_pbs-257", "c2048", ["trivial_pbs_async"])
def _b(E, orc):
    """bodies v delta, v delta + delta - 1 and 2^64 - 1 cycled over 257 rows of stride 750 > 743"""
    eng, p = E.eng, E.p
    N, k = p.polynomial_size, p.glwe_dimension
    msup, delta = p.message_modulus * p.carry_modulus, p.delta
    f = lambda m: (5 * m + 3) % msup  # noqa: E731
    lut = orc.fill_accumulator(N, k, p.message_modulus, p.carry_modulus, f)
    vs = list(range(2 * msup))
    bodies = [v * delta for v in vs] + [v * delta + delta - 1 for v in vs] + [2 ** 64 - 1]
    values = vs + vs + [2 * msup - 1]
    rows, stride = 257, 750
    pick = np.arange(rows) % len(bodies)
    buf = _rand64(150, rows, stride)
    buf[:, :WORDS - 1] = 0
    buf[:, WORDS - 1] = np.array(bodies, dtype=U64)[pick]
    exp = buf.copy()
    want = [(f(v % msup) * delta * (-1 if v >= msup else 1)) % 2 ** 64 for v in values]
    exp[:, WORDS - 1] = np.array(want, dtype=U64)[pick]
    regions = [_rin("lut", lut, row=lut.nbytes), _rout("out", buf.nbytes, row=stride * 8, data=buf)]
    return _spec(regions, lambda v: eng.trivial_pbs_async(v["out"].data_ptr() + 8 * (WORDS - 1), rows, stride, v["lut"]),
                 lambda: exp, "out", (None, 0), None, out_row=stride * 8)


# ---- the runner ---------------------------------------------------------------------------------------------
CASES.sort(key=lambda c: list(FACTORIES).index(c.engine) if c.engine in FACTORIES else 99)  # stable: engine by engine
_LAST_OF_ENGINE = {c.engine: c.id for c in CASES}


def _first_difference(got, exp, row):
    bad = np.flatnonzero(got != exp)
    return f"{bad.size} bytes differ, first in row {bad[0] // row} (byte {bad[0]}), last in row {bad[-1] // row}"


def _run_call(spec, arena, views):
    import torch

    spec.call(views)
    torch.cuda.synchronize()
    changed = arena.check()
    out = None if spec.out is None else arena.view(spec.out).cpu().numpy().copy()
    return out, changed


def build_arena(spec):
    """(arena, views) of a case: every region of the spec at 16 modulo 256, the scratch of exactly the queried
    size (test_async_graph_gpu.py replays the cases from arenas built here)"""
    # 3. the scratch: exactly the queried size, or none where the query says 0
    sname, need = spec.scratch
    names = [r.name for r in spec.regions]
    if need == 0:
        assert sname is None and "scratch" not in names
    else:
        assert [r.nbytes for r in spec.regions if r.name == sname] == [need]
    arena = GuardedArena("cuda:0", seed=1)
    for r in spec.regions:
        arena.region(r.name, r.nbytes, align=16, data=r.data, writable=r.writable, row=r.row)
    arena.allocate()
    views = {r.name: arena.view(r.name) for r in spec.regions}
    for v in views.values():
        assert v.data_ptr() % 256 == 16
    return arena, views


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_guarded_call(orc, c):
    E = _engine(c.engine, orc)
    try:
        spec = c.build(E, orc)
        eng = E.eng
        expected = np.ascontiguousarray(spec.twin()).view(np.uint8).reshape(-1)
        need = spec.scratch[1]
        arena, views = build_arena(spec)
        # first call, under the kernel timer
        eng.kernel_timing(1)
        out1, changed1 = _run_call(spec, arena, views)
        ran = set(eng.kernel_times())
        eng.kernel_timing(0)
        print(f"{c.id}: kernel families {sorted(ran)}, regions "
              f"{[(r.name, r.nbytes) for r in spec.regions]}, scratch query {need}")
        if spec.kernels is not None:
            assert spec.kernels <= ran, f"expected kernel families {spec.kernels}, ran {ran}"
        # 2. nothing outside the output and the scratch changed
        assert changed1 == [], f"first call wrote outside its output and scratch: {changed1}"
        # 4. again, from other garbage in the guards, the output and the scratch
        arena.refill(2)
        arena.restore()
        out2, changed2 = _run_call(spec, arena, views)
        assert changed2 == [], f"second call wrote outside its output and scratch: {changed2}"
        if spec.out is None:  # key ingestion: the result is the resident key
            got = spec.result()
            assert got.size == expected.size and np.array_equal(got, expected), "resident key differs from the twin's"
            return
        row = spec.out_row
        # 1. the twin, word for word
        assert out1.size == expected.size, (out1.size, expected.size)
        assert np.array_equal(out1, expected), "output differs from the host-pointer form: " + _first_difference(
            out1, expected, row)
        assert np.array_equal(out2, out1), "output depends on what the output or scratch held before: " + \
            _first_difference(out2, out1, row)
        if spec.oracle is not None:  # and a reference of its own on the sampled rows
            rows, want = spec.oracle()
            assert len(rows) <= 8
            got = np.ascontiguousarray(out1.reshape(-1, row)[rows])
            if getattr(spec, "oracle_post", None):
                got = np.ascontiguousarray(spec.oracle_post(got)).view(np.uint8).reshape(len(rows), -1)
            want = np.ascontiguousarray(want).view(np.uint8).reshape(len(rows), -1)
            bad = [int(r) for r, g, w in zip(rows, got, want) if not np.array_equal(g, w)]
            assert not bad, f"sampled rows {bad} differ from the reference"
    finally:
        if _LAST_OF_ENGINE[c.engine] == c.id and c.engine in ENGINES and not _needed_later(c):
            _check_keys_and_close(c.engine)  # 5. once per engine, after its last case


def _needed_later(c):
    """c2048 also serves as the twin of the key-ingestion cases, which run after its own"""
    return c.engine == "c2048"


def test_resident_keys_unchanged_at_the_end():
    """engines still open (c2048, and any whose last case was deselected): the same read-back"""
    errors = []
    for key in list(ENGINES):
        try:
            _check_keys_and_close(key)
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, errors


def test_device_arena_reports_a_stray_byte_and_decoys_change_the_output(orc):
    """The two things the cases above lean on, shown on the device: a byte written one past a region is
    reported, with its band and offset; and the decoy LUTs are live data -- the same call with lut_count = 4
    (indexes 2 and 3 then legitimately read the decoys) gives other rows exactly where the index exceeds 1,
    so an unclamped kernel could not pass a case."""
    import torch

    E = _engine("c2048", orc)
    eng, cnt = E.eng, 5
    cts, luts = _pbs_inputs(E, "pbs", cnt, 3)
    idx, idxc = _clamp_indexes(cnt)
    assert sorted(set(idx.tolist())) == [0, 2, 3]
    arena = GuardedArena("cuda:0", seed=7)
    for r in (_rin("lwe_in", cts, 24), _rin("lut_indexes", idx, 4), _rout("out", cnt * 2049 * 8, row=2049 * 8),
              _rout("scratch", eng.pbs_scratch_bytes(cnt)), _rin("luts", luts, 4096 * 8)):
        arena.region(r.name, r.nbytes, data=r.data, writable=r.writable, row=r.row)
    arena.allocate()
    v = {r.name: r.view for r in arena.regions}
    eng.programmable_bootstrap_async(v["lwe_in"], v["out"], v["luts"], 4, cnt, v["lut_indexes"], d_scratch=v["scratch"])
    torch.cuda.synchronize()
    assert arena.check() == []
    got = v["out"].cpu().numpy().view(U64).reshape(cnt, -1)
    clamped = eng.programmable_bootstrap(cts, luts[:2], idxc)
    differs = (got != clamped).any(axis=1)
    assert differs.tolist() == (idx > 1).tolist(), differs
    assert np.array_equal(got, eng.programmable_bootstrap(cts, luts, idx))
    out = next(r for r in arena.regions if r.name == "out")
    arena.buf[out.offset + out.nbytes] ^= 0x40      # one byte past the output
    arena.buf[out.offset - 1] ^= 0x40               # one byte before it
    v["luts"][5] ^= 1                               # and one inside an input
    names = [s[0] for s in arena.segments]
    before, after = names[names.index("out") - 1], names[names.index("out") + 1]
    glen = arena.segments[names.index(before)][2] - arena.segments[names.index(before)][1]
    assert arena.check() == [(before, glen - 1, glen - 1), (after, 0, 0), ("luts", 5, 5)]


def test_case_table_names_every_form():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert all(c.engine in FACTORIES for c in CASES)
