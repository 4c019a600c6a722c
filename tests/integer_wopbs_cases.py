"""Shared by test_integer_wopbs.py (CPU) and test_integer_wopbs_gpu.py: a CPU stand-in of the engine for
the integer WoP-PBS layer, built on the oracle and tests/wopbs_reference.WopRef, and the parameter sets
and keys of the cases (WoP 2_2 and 1_2 and PBS 2_2, lwe_dimension cut to 96 as in test_wopbs_gpu.py).

The stand-in offers exactly the calls integer.WopbsKey and shortint.WopbsKey make on an engine:
extract_bits, circuit_bootstrap_vertical_packing, keyswitch_key / keyswitch_with_key, keyswitch and the
PBS calls (the last three from oracle.OracleEngine), plus the key uploads.  Every keyswitch_with_key is
recorded in `ks_calls` as (in_dim, out_dim, base_log, level, rows).
"""
from types import SimpleNamespace

import numpy as np

from oracle.oracle import OracleEngine
from wopbs_reference import wop_ref_for

U64 = np.uint64
_cache = {}


class StandInEngine(OracleEngine):
    def __init__(self, params):
        super().__init__(params)
        self.bsk = self.pfpksk = self._ref = None
        self.ks_calls = []

    def upload_bootstrap_key(self, bsk):
        super().upload_bootstrap_key(bsk)
        self.bsk = bsk

    def upload_pfpksk_list(self, pfpksk, base_log, level):
        assert (base_log, level) == (self.p.pfks_base_log, self.p.pfks_level)
        self.pfpksk = pfpksk

    @property
    def ref(self):
        if self._ref is None:
            self._ref = wop_ref_for(self.O, self.p, self.bsk, self.ksk, self.pfpksk)
        return self._ref

    def extract_bits(self, lwe_in, delta_log, nbits):
        return self.ref.extract_bits(lwe_in, delta_log, nbits)

    def circuit_bootstrap_vertical_packing(self, lwe_in, cbs_base_log, cbs_level, luts, lut_indexes=None):
        return self.ref.circuit_bootstrap_vertical_packing(lwe_in, cbs_base_log, cbs_level, luts, lut_indexes)

    def keyswitch_key(self, ksk, in_dim, out_dim, base_log, level):
        ksk = np.ascontiguousarray(ksk, dtype=U64).ravel()
        assert ksk.size == in_dim * level * (out_dim + 1)
        return SimpleNamespace(ksk=ksk, in_dim=in_dim, out_dim=out_dim, base_log=base_log, level=level)

    def keyswitch_with_key(self, key, lwe_in):
        x = np.ascontiguousarray(lwe_in, dtype=U64).reshape(-1, key.in_dim + 1)
        self.ks_calls.append((key.in_dim, key.out_dim, key.base_log, key.level, x.shape[0]))
        return self.O.keyswitch(key.ksk, key.in_dim, key.out_dim, key.base_log, key.level, x)


def params(name):
    from tfhe_mi355 import parameters as P

    return {"wop_2_2": P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS, "wop_1_2": P.WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS,
            "pbs_2_2": P.PARAM_MESSAGE_2_CARRY_2_KS_PBS}[name].with_(lwe_dimension=96)


def client_key(name, seed):
    from tfhe_mi355.shortint import ClientKey

    if ("cks", name, seed) not in _cache:
        _cache[("cks", name, seed)] = ClientKey(params(name), seed)
    return _cache[("cks", name, seed)]


def standin_only_for_wopbs(name, seed=61):
    """(shortint client key, integer.WopbsKey on the stand-in) of one WoP set, its keys from `seed`."""
    if ("only", name, seed) in _cache:
        return _cache[("only", name, seed)]
    from tfhe_mi355 import integer
    from tfhe_mi355.shortint import ServerKey

    cks = client_key(name, seed)
    eng = StandInEngine(cks.parameters)
    sks = ServerKey(cks, engine=eng)
    _cache[("only", name, seed)] = (cks, integer.WopbsKey.new_wopbs_key_only_for_wopbs(cks, sks))
    return _cache[("only", name, seed)]


def standin_cross(seed=67):
    """(PBS 2_2 client key, its stand-in server key, integer.WopbsKey.new_wopbs_key on stand-ins)."""
    if ("cross", seed) in _cache:
        return _cache[("cross", seed)]
    from tfhe_mi355 import integer
    from tfhe_mi355.shortint import ServerKey

    cks = client_key("pbs_2_2", seed)
    sks = ServerKey(cks, engine=StandInEngine(cks.parameters))
    wk = integer.WopbsKey.new_wopbs_key(cks, sks, params("wop_2_2"), engine=StandInEngine(params("wop_2_2")))
    _cache[("cross", seed)] = (cks, sks, wk)
    return _cache[("cross", seed)]


def hand_bits(ref, data, nbits, delta_log):
    """The bits integer.WopbsKey must hand to the composed call, assembled block by block: blocks most
    significant first, block j's nbits[j] bits most significant first; data [K][blocks][kN+1]."""
    parts = [ref.extract_bits(data[:, j, :], delta_log, nbits[j]) for j in range(data.shape[1] - 1, -1, -1) if nbits[j]]
    return np.concatenate(parts, axis=1)
