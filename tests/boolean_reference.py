"""RefEngine32: the engine's 32-bit-torus methods computed on the CPU (test infrastructure).

Shares no code with libtfhe_mi355.  The PBS is tests/boolean_ref32.c (compiled here on first use) over
the ORACLE's FFT: the helper is handed the oracle library's orc_fft_forward_integer and
orc_fft_complex as function pointers and the oracle's twist table (orc_mono_spectrum at frequency 0
returns twist[d]), and the Fourier key is the oracle's FourierBsk of the key widened to u64.  A
different FFT would differ from the GPU by +-1 in about a tenth of the u32 outputs (the rounding grain
is 2^-32, the f64 error of these products about 2^-35), so bit-exact parity needs the same DAG.

The keyswitch and the gate algebra are exact integer numpy.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T, F = 1 << 29, 7 << 29  # boolean/mod.rs:77-80
u32p = ctypes.POINTER(ctypes.c_uint32)
f64p = ctypes.POINTER(ctypes.c_double)
_helper = None


def helper():
    """ctypes handle of boolean_ref32.c, compiled once per source version into the temp directory."""
    global _helper
    if _helper is not None:
        return _helper
    src = os.path.join(HERE, "boolean_ref32.c")
    tag = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
    so = os.path.join(tempfile.gettempdir(), f"boolean_ref32_{os.getuid()}_{tag}.so")
    if not os.path.exists(so):
        tmp = f"{so}.{os.getpid()}"
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fopenmp", "-o", tmp,
                        src, "-lm"], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    L.ref32_from_fraction.restype = ctypes.c_uint32
    L.ref32_from_fraction.argtypes = [ctypes.c_double]
    L.ref32_external_product.argtypes = [ctypes.c_void_p, ctypes.c_void_p, f64p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, f64p, u32p, u32p]
    L.ref32_pbs_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, f64p, f64p, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p, u32p, u32p, u32p, ctypes.c_long,
                                  ctypes.c_int]
    _helper = L
    return L


def _oracle():
    from oracle import oracle as O

    O.build()
    return O


def _fn(O, name):
    return ctypes.cast(getattr(O.lib(), name), ctypes.c_void_p)


_twists = {}


def twist_table(N: int) -> np.ndarray:
    """The oracle's twist[d] = exp(i pi d / N), d < N/2: the spectrum of X^d at the position of frequency 0."""
    if N not in _twists:
        O = _oracle()
        p0 = int(np.nonzero(O.pos_freq(N) == 0)[0][0])
        _twists[N] = np.array([O.mono_spectrum(N, d)[p0] for d in range(N // 2)], dtype=np.complex128)
    return _twists[N]


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def widen(a) -> np.ndarray:
    return _u32(a).astype(np.uint64) << np.uint64(32)


def from_fraction(fr) -> np.ndarray:
    """X = rint_half_even(fr 2^32) mod 2^32 (the reference formula of the backward conversion)."""
    h = helper()
    return np.array([h.ref32_from_fraction(float(x)) for x in np.asarray(fr, dtype=np.float64).ravel()],
                    dtype=np.uint32)


def conversion_edge_fractions() -> np.ndarray:
    """+-1/2, +-(1/2 - 2^-53), 0 and ties (j + 1/2) 2^-32."""
    j = np.array([0, 1, 2, 3, 12345, (1 << 31) - 2, -1, -2, -3, -(1 << 31) + 1], dtype=np.float64)
    return np.concatenate([[0.5, -0.5, 0.5 - 2.0 ** -53, -(0.5 - 2.0 ** -53), 0.0], (j + 0.5) * 2.0 ** -32])


def conversion_expected(fr) -> np.ndarray:
    """rint_half_even(fr 2^32) mod 2^32 in exact integer arithmetic (fr 2^32 is an exact f64)."""
    out = []
    for x in np.asarray(fr, dtype=np.float64):
        num, den = (float(x) * 4294967296.0).as_integer_ratio()
        q, r = divmod(num, den)
        if 2 * r > den or (2 * r == den and q & 1):
            q += 1
        out.append(q % (1 << 32))
    return np.array(out, dtype=np.uint32)


def decompose32(words, base_log: int, level: int) -> np.ndarray:
    """Signed digits [..., level] of u32 words, level L first (decomposer.rs:99-153, iter.rs:134-141)."""
    x = _u32(words).astype(np.int64)
    bits = base_log * level
    state = ((x >> (31 - bits)) + 1) >> 1
    state &= (1 << bits) - 1  # closest_representable wraps
    out = np.empty(x.shape + (level,), dtype=np.int64)
    mask = (1 << base_log) - 1
    for lv in range(level):
        res = state & mask
        state >>= base_log
        carry = (((res - 1) | state) & res) >> (base_log - 1)
        state += carry
        out[..., lv] = res - (carry << base_log)
    return out


class RefEngine32:
    """The u32 methods of tfhe_mi355.Engine on the CPU, for one BooleanParameters set."""

    def __init__(self, parameters):
        self.params = parameters
        self.O = _oracle()
        self._fourier = None
        self._ksk = None

    @property
    def n(self):
        return self.params.lwe_dimension

    @property
    def big_dim(self):
        return self.params.glwe_dimension * self.params.polynomial_size

    @property
    def glwe_len(self):
        return (self.params.glwe_dimension + 1) * self.params.polynomial_size

    # -- keys ------------------------------------------------------------------------------------
    def upload_bootstrap_key_u32(self, bsk32) -> None:
        p = self.params
        fb = self.O.FourierBsk(widen(bsk32).ravel(), p.lwe_dimension, p.glwe_dimension, p.polynomial_size,
                               p.pbs_base_log, p.pbs_level)
        self._fourier = np.ascontiguousarray(fb.fourier())

    def upload_keyswitch_key_u32(self, ksk32) -> None:
        p = self.params
        self._ksk = _u32(ksk32).reshape(self.big_dim * p.ks_level, p.lwe_dimension + 1)

    # -- PBS ---------------------------------------------------------------------------------------
    def _pbs(self, lwe_in, luts, lut_indexes, glwe_out: bool) -> np.ndarray:
        p, n = self.params, self.n
        x = _u32(lwe_in).reshape(-1, n + 1)
        L = _u32(luts).reshape(-1, self.glwe_len)
        idx = None if lut_indexes is None else np.ascontiguousarray(lut_indexes, dtype=np.uint32)
        out = np.zeros((x.shape[0], self.glwe_len if glwe_out else self.big_dim + 1), dtype=np.uint32)
        tw = twist_table(p.polynomial_size)
        helper().ref32_pbs_batch(_fn(self.O, "orc_fft_complex"), _fn(self.O, "orc_fft_forward_integer"),
                                 tw.ctypes.data_as(f64p), self._fourier.ctypes.data_as(f64p), n, p.glwe_dimension,
                                 p.polynomial_size, p.pbs_base_log, p.pbs_level, x.ctypes.data_as(u32p),
                                 out.ctypes.data_as(u32p), L.ctypes.data_as(u32p),
                                 None if idx is None else idx.ctypes.data_as(u32p), x.shape[0], int(glwe_out))
        return out

    def programmable_bootstrap_u32(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        return self._pbs(lwe_in, luts, lut_indexes, False)

    def blind_rotate_u32(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        return self._pbs(lwe_in, luts, lut_indexes, True)

    def external_product(self, ggsw_fourier, acc, glwe) -> np.ndarray:
        """acc + ggsw (x) glwe on u32 GLWEs: one CMUX's add_external_product_assign."""
        p = self.params
        out = _u32(acc).copy().ravel()
        g = _u32(glwe).ravel()
        gf = np.ascontiguousarray(ggsw_fourier, dtype=np.complex128)
        tw = twist_table(p.polynomial_size)
        helper().ref32_external_product(_fn(self.O, "orc_fft_complex"), _fn(self.O, "orc_fft_forward_integer"),
                                        tw.ctypes.data_as(f64p), p.glwe_dimension, p.polynomial_size,
                                        p.pbs_base_log, p.pbs_level, gf.ctypes.data_as(f64p),
                                        out.ctypes.data_as(u32p), g.ctypes.data_as(u32p))
        return out

    # -- keyswitch: exact integers -------------------------------------------------------------------
    def keyswitch_u32(self, lwe_in, ksk=None, in_dim=None, out_dim=None, base_log=None, level=None) -> np.ndarray:
        p = self.params
        in_dim = self.big_dim if in_dim is None else in_dim
        out_dim = self.n if out_dim is None else out_dim
        base_log, level = base_log or p.ks_base_log, level or p.ks_level
        K = self._ksk if ksk is None else _u32(ksk).reshape(in_dim * level, out_dim + 1)
        x = _u32(lwe_in).reshape(-1, in_dim + 1)
        D = decompose32(x[:, :in_dim], base_log, level).reshape(x.shape[0], in_dim * level)
        # D K mod 2^32 through two exact f64 products on the 16-bit halves of the key
        assert (1 << (base_log - 1)) * 65536 * in_dim * level < 2 ** 53
        Df = D.astype(np.float64)
        lo = (Df @ (K & np.uint32(0xFFFF)).astype(np.float64)).astype(np.int64)
        hi = (Df @ (K >> np.uint32(16)).astype(np.float64)).astype(np.int64)
        acc = (lo + (hi << 16)) & 0xFFFFFFFF
        out = (-acc) & 0xFFFFFFFF
        out[:, out_dim] = (out[:, out_dim] + x[:, in_dim].astype(np.int64)) & 0xFFFFFFFF
        return out.astype(np.uint32)

    # -- gates ---------------------------------------------------------------------------------------
    def _lut_true(self) -> np.ndarray:
        lut = np.zeros(self.glwe_len, dtype=np.uint32)
        lut[self.big_dim:] = T
        return lut

    def _bootstrap_pattern(self, rows, pbs_order: int) -> np.ndarray:
        if pbs_order:
            return self.keyswitch_u32(self.programmable_bootstrap_u32(rows, self._lut_true()))
        return self.programmable_bootstrap_u32(self.keyswitch_u32(rows), self._lut_true())

    def boolean_gates(self, ops, lhs, rhs, pbs_order: int) -> np.ndarray:
        w = (self.n if pbs_order else self.big_dim) + 1
        a, b = _u32(lhs).reshape(-1, w).astype(np.int64), _u32(rhs).reshape(-1, w).astype(np.int64)
        ops = np.asarray(ops, dtype=np.int64).ravel()
        if ops.size and (ops.min() < 0 or ops.max() > 5):
            raise ValueError("opcode above 5")
        s = np.array([1, -1, -1, 1, 2, -2], dtype=np.int64)[ops]
        c = np.array([F, T, F, T, 2 * T, -2 * T], dtype=np.int64)[ops]
        rows = s[:, None] * (a + b)
        rows[:, -1] += c
        return self._bootstrap_pattern((rows & 0xFFFFFFFF).astype(np.uint32), pbs_order)

    def boolean_mux(self, cond, then_ct, else_ct, pbs_order: int) -> np.ndarray:
        w = (self.n if pbs_order else self.big_dim) + 1
        c, t, e = (_u32(x).reshape(-1, w).astype(np.int64) for x in (cond, then_ct, else_ct))
        rows = np.empty((2 * c.shape[0], w), dtype=np.int64)
        rows[0::2] = c + t
        rows[1::2] = e - c
        rows[:, -1] += F
        rows = (rows & 0xFFFFFFFF).astype(np.uint32)
        lut = self._lut_true()
        if pbs_order:
            b = self.programmable_bootstrap_u32(rows, lut).astype(np.int64)
            s = b[0::2] + b[1::2]
            s[:, -1] += T
            return self.keyswitch_u32((s & 0xFFFFFFFF).astype(np.uint32))
        b = self.programmable_bootstrap_u32(self.keyswitch_u32(rows), lut).astype(np.int64)
        s = b[0::2] + b[1::2]
        s[:, -1] += T
        return (s & 0xFFFFFFFF).astype(np.uint32)

    def boolean_not(self, ct) -> np.ndarray:
        return ((-_u32(ct).astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
