"""The radix integer DAG (tfhe_mi355/integer.py) on the host path, oracle engine, at lwe_dimension = 8:
which parameter sets the carry-propagating entry points serve and which they refuse, the shared case list
of integer_dag_cases.py checked against plain Python integers, and the device layer-table caches driven
with CPU tensors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import integer_dag_cases as C
from conftest import OracleEngine

# The rule (integer.propagation_refusal / mul_refusal), written out: a change of the rule is a change here.
SUPPORTED = ["PARAM_MESSAGE_2_CARRY_2_KS_PBS"]
REJECTED = [
    "PARAM_MESSAGE_1_CARRY_0_KS_PBS", "PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_2_CARRY_0_KS_PBS",
    "PARAM_MESSAGE_1_CARRY_2_KS_PBS", "PARAM_MESSAGE_2_CARRY_1_KS_PBS", "PARAM_MESSAGE_3_CARRY_0_KS_PBS",
    "PARAM_MESSAGE_1_CARRY_3_KS_PBS", "PARAM_MESSAGE_3_CARRY_1_KS_PBS", "PARAM_MESSAGE_4_CARRY_0_KS_PBS",
]
# N > 2048: decided by the rule.  (message bits, carry bits) the whole layer serves, and the pairs where the
# propagation and the sum are served and the multiply is refused (its bivariate product needs
# carry_modulus >= message_modulus); every other pair of SHORTINT_ALL is refused outright.
RULE_SUPPORTED = [(2, 2), (3, 3), (4, 4)]
RULE_ADD_ONLY = [(3, 2), (4, 2), (4, 3), (5, 2), (5, 3), (6, 2)]
# Sets above N = 2048 that are cheap enough at lwe_dimension = 8 to run as well (N = 4096 and 8192)
LARGE_SUPPORTED = ["PARAM_MESSAGE_3_CARRY_3_KS_PBS"]
LARGE_ADD_ONLY = ["PARAM_MESSAGE_3_CARRY_2_KS_PBS", "PARAM_MESSAGE_4_CARRY_2_KS_PBS"]
LARGE_REJECTED = ["PARAM_MESSAGE_2_CARRY_3_KS_PBS"]       # carry_modulus > message_modulus


def _sweep(name):
    """One set in a child process under a time limit: a DAG that stops shrinking fails here instead of
    hanging the run."""
    r = subprocess.run([sys.executable, os.path.abspath(C.__file__), name], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_pinned_lists_cover_every_small_set():
    from tfhe_mi355.parameters import SHORTINT_ALL

    small = [n for n, p in SHORTINT_ALL.items() if n.endswith("_KS_PBS") and p.polynomial_size <= 2048]
    assert sorted(small) == sorted(SUPPORTED + REJECTED)


@pytest.mark.parametrize("name", SUPPORTED + LARGE_SUPPORTED)
def test_sweep_supported_set_passes_every_case(name):
    res = _sweep(name)
    assert {op: r["verdict"] for op, r in res.items()} == {op: "ok" for op in C.SWEEP_OPS}


@pytest.mark.parametrize("name", REJECTED + LARGE_REJECTED)
def test_sweep_rejected_set_is_refused_before_any_pbs(name):
    res = _sweep(name)
    for op in C.SWEEP_OPS:
        v = res[op]["verdict"]
        assert v.startswith("NotImplementedError") and name in v and "not supported: " in v, (op, v)
        assert res[op]["pbs_count"] == 0 and res[op]["seconds"] < 0.5, res[op]


@pytest.mark.parametrize("name", LARGE_ADD_ONLY)
def test_sweep_add_only_set(name):
    """carry_modulus < message_modulus with room for the carry states: the additions pass, the multiply is
    refused before its first PBS."""
    res = _sweep(name)
    mul = res.pop("mul_parallelized")
    assert mul["verdict"].startswith("NotImplementedError") and name in mul["verdict"] and mul["pbs_count"] == 0
    assert {op: r["verdict"] for op, r in res.items()} == {"add_assign_parallelized": "ok", "dirty_add": "ok"}


def test_rule_on_every_shortint_set():
    from tfhe_mi355.integer import mul_refusal, propagation_refusal
    from tfhe_mi355.parameters import SHORTINT_ALL

    full, add_only = [], []
    for name, p in SHORTINT_ALL.items():
        if not name.endswith("_KS_PBS"):
            continue
        bits = (p.message_modulus.bit_length() - 1, p.carry_modulus.bit_length() - 1)
        if propagation_refusal(p.message_modulus, p.carry_modulus) is None:
            (full if mul_refusal(p.message_modulus, p.carry_modulus) is None else add_only).append(bits)
    assert sorted(full) == RULE_SUPPORTED and sorted(add_only) == RULE_ADD_ONLY


class _NoEngine:
    def upload_bootstrap_key(self, bsk):
        pass

    def upload_keyswitch_key(self, ksk):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached on a refused parameter set")


@pytest.mark.parametrize("name", ["PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_2_CARRY_3_KS_PBS",
                                  "PARAM_MESSAGE_2_CARRY_1_KS_PBS", "PARAM_MESSAGE_3_CARRY_1_KS_PBS",
                                  "PARAM_MESSAGE_4_CARRY_4_KS_PBS"])
def test_every_entry_point_refuses_or_accepts_by_the_rule(name):
    """The key is built for every set; on a refused one each carry-propagating entry point raises
    NotImplementedError naming the set, without touching the engine or its operands' data."""
    from tfhe_mi355 import integer, shortint
    from tfhe_mi355.parameters import SHORTINT_ALL

    P = SHORTINT_ALL[name]
    sks = integer.ServerKey(shortint.ServerKey(None, engine=_NoEngine(), parameters=P))
    if name == "PARAM_MESSAGE_4_CARRY_4_KS_PBS":
        assert sks.propagation_refusal is None and sks.mul_refusal is None
        return
    sks.lwe_size = 3
    x, y = sks.create_trivial_zero(2, 3), sks.create_trivial_zero(2, 3)
    x.degree = y.degree = [P.message_modulus - 1] * 3
    x.noise = y.noise = [1] * 3
    for call in (lambda: sks.full_propagate(x), lambda: sks.add_assign_parallelized(x, y),
                 lambda: sks.unchecked_sum_ciphertexts_vec([x, y, x]), lambda: sks.unchecked_sum_ciphertexts_vec([]),
                 lambda: sks.unchecked_mul(x, y), lambda: sks.mul_parallelized(x, y)):
        with pytest.raises(NotImplementedError, match=f"{name} .*is not supported: "):
            call()
    assert sks.pbs_count == 0 and sks.launches == 0 and not x.data.any()


# ---- the shared case list on the host path -----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_key():
    return C.keys(OracleEngine(C.params(), threads=4))


def test_case_list_is_complete():
    assert [c.id for c in C.CASES] == list(C.EXPECTED)
    assert {c.nb for c in C.CASES} == set(C.BLOCKS)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_host_dag_case(host_key, case):
    ck, sks = host_key
    enc = C.encrypt(ck, case)
    before = [e.data.copy() for e in enc]
    out = sks.to_host(C.run(case, sks, enc))
    assert (sks.pbs_count, sks.launches) == C.EXPECTED[case.id]
    assert np.array_equal(C.decrypt(ck, case, out), C.expected(case))
    assert out.block_carries_are_empty(C.MSG) and out.num_blocks == case.nb
    assert all(np.array_equal(e.data, b) for e, b in zip(enc, before))


def test_boolean_valued_operand_is_refused(host_key):
    ck, sks = host_key
    case = C.CASES[0]
    a = C.encrypt(ck, case)[0]
    with pytest.raises(NotImplementedError, match="boolean-valued operand"):
        sks.mul_parallelized(a, sks.create_trivial_zero(C.K, case.nb))


# ---- the device layer-table caches, on CPU tensors -----------------------------------------------------------
def _cpu_device_ops(cap, capturing):
    """_DeviceOps with its tensors on the CPU: the cache logic of lut() and _layer_tables() runs as on the
    GPU (same keys, same identity checks, same eviction), only the uploads land in host memory."""
    import torch

    from tfhe_mi355.integer import _BoundedCache, _DeviceOps

    ops = object.__new__(_DeviceOps)
    ops.torch, ops.device = torch, torch.device("cpu")
    ops._lut_dev = _BoundedCache(cap, lambda: capturing[0])
    ops._stacks = _BoundedCache(cap, lambda: capturing[0])
    return ops


class _Rows:
    def __init__(self, count):
        self.count = count


def _lut(value):
    from tfhe_mi355.shortint import LookupTable

    return LookupTable(np.full(16, value, dtype=np.uint64), 3)


def _check_tables(ops, K, luts, lis):
    todo = [(_Rows(K), 0, li) for li in lis]
    d_luts, idx = ops._layer_tables(todo, luts)
    assert np.array_equal(d_luts.numpy().view(np.uint64), np.stack([lut.acc for lut in luts]))
    if len(luts) > 1:
        assert np.array_equal(idx.numpy(), np.repeat(np.asarray(lis, dtype=np.int32), K))
    else:
        assert idx is None
    for lut in luts:
        assert np.array_equal(ops.lut(lut).numpy().view(np.uint64), lut.acc)


def test_layer_tables_follow_recreated_luts_and_batch_sizes():
    """A LUT created, used, dropped and recreated in a loop (its id() is likely to come back), two batch
    sizes, a cache of 2 entries: every lookup returns the tables of the LUT objects it was given."""
    ops = _cpu_device_ops(2, [False])
    keep = [_lut(1000), _lut(2000)]
    for i in range(40):
        fresh = _lut(i)
        for K in (1, 3):
            _check_tables(ops, K, [fresh], [0, 0])
            _check_tables(ops, K, [keep[0], fresh], [0, 1, 1])
            _check_tables(ops, K, [fresh, keep[i % 2]], [1, 0])
            assert len(ops._stacks) <= 2 and len(ops._lut_dev) <= 2
        del fresh


def test_layer_tables_reject_a_stale_entry_under_a_reused_id():
    """A cached entry keeps its LUT objects alive, so a live entry's ids cannot be reused; the identity
    check in _layer_tables and lut() is the second line behind that.  Planting an entry whose LUTs are not
    the ones asked for (what a reused id would look like) must give a fresh upload, not the stale table."""
    ops = _cpu_device_ops(4, [False])
    old, new = _lut(7), _lut(9)
    todo = [(_Rows(3), 0, 0)]
    stale = ops._layer_tables(todo, [old])[0]
    key = (3, (id(new),), ())
    ops._stacks.put(key, ([old], stale, None))
    ops._lut_dev.put(id(new), (old, stale[0]))
    assert np.array_equal(ops._layer_tables(todo, [new])[0].numpy().view(np.uint64), new.acc[None])
    assert np.array_equal(ops.lut(new).numpy().view(np.uint64), new.acc)


def test_layer_tables_touched_during_capture_stay_pinned():
    """What a captured graph reads must outlive eviction: tables looked up (hit or miss) while capturing are
    the same tensor objects after the cache has been flooded, and do not count against the cap's eviction."""
    capturing = [False]
    ops = _cpu_device_ops(2, capturing)
    warm, cold = _lut(1), _lut(2)
    todo = [(_Rows(3), 0, 0)]
    t_warm = ops._layer_tables(todo, [warm])[0]           # eager warm-up: cached, not pinned
    capturing[0] = True
    assert ops._layer_tables(todo, [warm])[0] is t_warm   # hit during capture
    t_cold = ops._layer_tables(todo, [cold])[0]           # miss during capture
    l_warm = ops.lut(warm)
    capturing[0] = False
    pinned = dict(ops._stacks._pinned)
    assert len(pinned) == 2 and len(ops._lut_dev._pinned) == 1
    for i in range(10):                                   # flood both caches
        _check_tables(ops, 3, [_lut(100 + i)], [0])
    assert set(ops._stacks._pinned) == set(pinned) and len(ops._stacks._d) <= 2
    assert ops._layer_tables(todo, [warm])[0] is t_warm and ops._layer_tables(todo, [cold])[0] is t_cold
    assert ops.lut(warm) is l_warm
