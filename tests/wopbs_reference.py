"""CPU reference of the bootstrapped half of WoP-PBS (private functional packing keyswitch, bit
extraction, circuit bootstrap, and their composition with vertical packing), built from the oracle
alone (oracle/ stays as it is); shared by test_wopbs.py and test_wopbs_gpu.py.

pfpks.  The oracle's packing keyswitch computes out = (body at the GLWE body's constant term) -
sum_i sum_lvl digit_lvl(in_i) * key[i][lvl] over in_dim mask words, key levels stored L..1.  Called
with in_dim = kN + 1 on the input with one zero word appended, the appended word is the body it adds
(zero) and the real body is one more decomposed row: exactly the pfpks, once key g's level axis is
flipped from the reference's 1..L order.

Bit extraction and circuit bootstrap follow wop_pbs/mod.rs:158-224 and :320-343, 369-444 step for
step on O.keyswitch, FourierBsk.pbs and that pfpks.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ggsw_reference import Ref

U64 = np.uint64


def pfpksk_shape(k, N, level):
    return (k + 1, k * N + 1, level, (k + 1) * N)


def pfpks(O, key_list, k, N, base_log, level, lwe_in):
    """[count][kN+1] -> [count][k+1][(k+1)N] under the key list [k+1][kN+1][level][(k+1)N], level 1 first."""
    keys = np.ascontiguousarray(key_list, dtype=U64).reshape(pfpksk_shape(k, N, level))
    x = np.ascontiguousarray(lwe_in, dtype=U64).reshape(-1, k * N + 1)
    xz = np.concatenate([x, np.zeros((x.shape[0], 1), dtype=U64)], axis=1)

    flipped = [np.ascontiguousarray(keys[g][:, ::-1]) for g in range(k + 1)]
    out = np.zeros((x.shape[0], k + 1, (k + 1) * N), dtype=U64)
    step = max(1, -(-x.shape[0] // 8))

    def one(job):
        g, a = job
        out[a:a + step, g] = O.packing_keyswitch(flipped[g], k * N + 1, k, N, base_log, level, xz[a:a + step])

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, [(g, a) for g in range(k + 1) for a in range(0, x.shape[0], step)]))
    return out


class WopRef:
    """Keys of one WoP-PBS setting: fbsk an oracle FourierBsk, ksk [kN][ks_level][n+1] (levels L..1),
    pfpksk in the reference's order."""

    def __init__(self, O, n, k, N, ks, pfks, fbsk, ksk, pfpksk):
        self.O, self.n, self.k, self.N = O, n, k, N
        self.ks, self.pfks = ks, pfks
        self.fbsk, self.ksk, self.pfpksk = fbsk, ksk, pfpksk
        self.glwe = (k + 1) * N

    def _const_lut(self, value):
        lut = np.zeros(self.glwe, dtype=U64)
        lut[self.k * self.N:] = U64((-value) % (1 << 64))
        return lut

    def pfpks(self, lwe_in):
        return pfpks(self.O, self.pfpksk, self.k, self.N, self.pfks[0], self.pfks[1], lwe_in)

    def extract_bits(self, lwe_in, delta_log, nbits):
        """wop_pbs/mod.rs:158-224: [count][kN+1] -> [count][nbits][n+1], most significant bit first."""
        kN = self.k * self.N
        cur = np.array(lwe_in, dtype=U64).reshape(-1, kN + 1)
        out = np.zeros((cur.shape[0], nbits, self.n + 1), dtype=U64)
        for b in range(nbits):
            shifted = cur << U64(64 - delta_log - b - 1)
            ks = self.O.keyswitch(self.ksk, kN, self.n, self.ks[0], self.ks[1], shifted)
            out[:, nbits - 1 - b] = ks
            if b == nbits - 1:
                break
            ks[:, -1] += U64(1 << 62)
            pbs = self.fbsk.pbs(ks, self._const_lut(1 << (delta_log - 1 + b)))
            pbs[:, -1] += U64(1 << (delta_log + b - 1))
            cur -= pbs
        return out

    def circuit_bootstrap(self, lwe_in, delta_log, cbs_base_log, cbs_level):
        """wop_pbs/mod.rs:243-444: [count][n+1] -> [count][cbs_level][k+1][(k+1)N]."""
        x = np.ascontiguousarray(lwe_in, dtype=U64).reshape(-1, self.n + 1)
        out = np.zeros((x.shape[0], cbs_level, self.k + 1, self.glwe), dtype=U64)
        shifted = x * U64(1 << (63 - delta_log))
        shifted[:, -1] += U64(1 << 62)
        for lvl in range(1, cbs_level + 1):
            alpha = 1 << (63 - cbs_base_log * lvl)
            pbs = self.fbsk.pbs(shifted, self._const_lut(alpha))
            pbs[:, -1] += U64(alpha)
            out[:, lvl - 1] = self.pfpks(pbs)
        return out

    def circuit_bootstrap_vertical_packing(self, lwe_in, cbs_base_log, cbs_level, luts, lut_indexes=None):
        """wop_pbs/mod.rs:647-746: lwe_in [count][nbits][n+1] bits at q/2, luts [lut_count][nout][npoly][N]
        -> [count][nout][kN+1]."""
        x = np.ascontiguousarray(lwe_in, dtype=U64)
        count, nbits = x.shape[0], x.shape[1]
        luts = np.ascontiguousarray(luts, dtype=U64)
        ggsw = self.circuit_bootstrap(x.reshape(count * nbits, -1), 63, cbs_base_log, cbs_level)
        ggsw = ggsw.reshape(count, nbits, -1)
        ref = Ref(self.O, self.k, self.N, cbs_base_log, cbs_level)
        out = np.zeros((count, luts.shape[1], self.k * self.N + 1), dtype=U64)
        for c in range(count):
            lut = luts[0 if lut_indexes is None else int(lut_indexes[c])]
            for o in range(luts.shape[1]):
                out[c, o] = ref.vertical_packing(ggsw[c], lut[o])
        return out


# ---- the decryption case shared by test_wopbs.py (CPU) and test_wopbs_gpu.py ---------------------------
DECRYPT_SEED = 21
_decrypt_case = {}


def wop_keys(cks):
    """The key material ServerKey(cks) and WopbsKey.new_wopbs_key_only_for_wopbs(cks, sks) generate, as
    arrays (the same seeds): standard BSK, KSK, pfpksk list."""
    from tfhe_mi355 import client

    p, s = cks.parameters, cks.seed
    bsk = client.gen_bootstrap_key(s * 7 + 3, cks.small_lwe_secret_key, cks.glwe_secret_key, p.glwe_dimension,
                                   p.polynomial_size, p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev)
    ksk = client.gen_keyswitch_key(s * 7 + 4, cks.large_lwe_secret_key, cks.small_lwe_secret_key, p.ks_base_log,
                                   p.ks_level, p.lwe_modular_std_dev)
    pfpksk = client.gen_pfpksk_list(s * 7 + 5, cks.large_lwe_secret_key, cks.glwe_secret_key, p.glwe_dimension,
                                    p.polynomial_size, p.pfks_base_log, p.pfks_level, p.pfks_modular_std_dev)
    return bsk, ksk, pfpksk


def wop_ref_for(O, p, bsk, ksk, pfpksk):
    fb = O.FourierBsk(bsk, p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.pbs_base_log, p.pbs_level)
    return WopRef(O, p.lwe_dimension, p.glwe_dimension, p.polynomial_size, (p.ks_base_log, p.ks_level),
                  (p.pfks_base_log, p.pfks_level), fb, ksk, pfpksk)


def decrypt_case(O):
    """WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS with its real keys, fixed seeds and inputs, and the
    reference's outputs, computed once per process:
      a: all 16 messages without padding, one batch, through the 4-bit LUT i -> lut_value(i mod 4) << 60;
      b: two items of three 4-bit blocks each, as one 12-bit index (1 tree bit, 11 rotation bits) into
         vp_lut(2, N, 11, 2^60)."""
    if _decrypt_case:
        return _decrypt_case
    from ggsw_reference import lut_value, vp_lut
    from tfhe_mi355.parameters import WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS as P
    from tfhe_mi355.shortint import ClientKey

    cks = ClientKey(P, DECRYPT_SEED)
    bsk, ksk, pfpksk = wop_keys(cks)
    ref = wop_ref_for(O, P, bsk, ksk, pfpksk)
    N = P.polynomial_size
    msgs_a = np.arange(16, dtype=U64)
    cts_a = cks.encrypt_without_padding_many(msgs_a)
    lut_a = np.zeros(N, dtype=U64)
    for i in range(16):
        lut_a[i] = U64(lut_value(i % 4) << 60)
    x_a = np.stack([c.ct for c in cts_a])
    bits_a = ref.extract_bits(x_a, 60, 4)
    out_a = ref.circuit_bootstrap_vertical_packing(bits_a, P.cbs_base_log, P.cbs_level, lut_a.reshape(1, 1, 1, N))
    blocks_b = np.array([[0xA, 0x3, 0x5], [0x0, 0xF, 0xC]], dtype=U64)  # most significant block first
    cts_b = cks.encrypt_without_padding_many(blocks_b.ravel())
    x_b = np.stack([c.ct for c in cts_b])
    bits_b = ref.extract_bits(x_b, 60, 4)                               # [6][4][n+1]
    lut_b = vp_lut(2, N, 11, 1 << 60).reshape(1, 1, 2, N)
    out_b = ref.circuit_bootstrap_vertical_packing(bits_b.reshape(2, 12, -1), P.cbs_base_log, P.cbs_level, lut_b)
    index_b = [(int(r[0]) << 8) | (int(r[1]) << 4) | int(r[2]) for r in blocks_b]
    _decrypt_case.update(P=P, cks=cks, bsk=bsk, ksk=ksk, pfpksk=pfpksk, ref=ref, msgs_a=msgs_a, cts_a=cts_a, x_a=x_a,
                         lut_a=lut_a, bits_a=bits_a, out_a=out_a, blocks_b=blocks_b, x_b=x_b, bits_b=bits_b,
                         lut_b=lut_b, out_b=out_b, index_b=index_b)
    return _decrypt_case
