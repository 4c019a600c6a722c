"""RefEngine128: the engine's 128-bit-torus methods computed on the CPU (test infrastructure).

Shares no code with libtfhe_mi355 and reads nothing outside the repository.  The arithmetic is
tests/pbs_ref128.c (compiled here on first use), which restates DESIGN.md 3b operation for operation; the
twist and twiddle tables are computed HERE with big-integer fixed-point Taylor series at 320 bits and handed
to the C code as data.  Every table entry is canonical (hi = RN(x), lo = RN(x - hi) of the exact real x), so
this independent computation gives the engine's tables bit for bit.

u128 words are uint64 pairs (low, high): arrays of shape [..., 2].
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
i64p = ctypes.POINTER(ctypes.c_int64)
f64p = ctypes.POINTER(ctypes.c_double)
MASK128 = (1 << 128) - 1
_helper = None


def helper():
    """ctypes handle of pbs_ref128.c, compiled once per source version into the temp directory."""
    global _helper
    if _helper is not None:
        return _helper
    src = os.path.join(HERE, "pbs_ref128.c")
    tag = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
    so = os.path.join(tempfile.gettempdir(), f"pbs_ref128_{os.getuid()}_{tag}.so")
    if not os.path.exists(so):
        tmp = f"{so}.{os.getpid()}"
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-fopenmp",
                        "-o", tmp, src, "-lm"], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    c_int, c_long, c_u64, c_dbl = ctypes.c_int, ctypes.c_long, ctypes.c_uint64, ctypes.c_double
    for name, args in {
        "ref128_to_signed_dd": [u64p, f64p, f64p, c_long],
        "ref128_torus_from_f128": [f64p, f64p, u64p, u64p, c_long],
        "ref128_decompose": [u64p, c_long, c_int, c_int, i64p, u64p],
        "ref128_roundtrip": [u64p, c_int, f64p, f64p, u64p],
        "ref128_fft_product": [u64p, i64p, c_int, f64p, f64p, u64p],
        "ref128_exact_product": [u64p, i64p, c_int, u64p],
        "ref128_bsk_to_fourier": [u64p, c_long, c_int, f64p, f64p, f64p],
        "ref128_pbs_batch": [f64p, f64p, f64p, c_int, c_int, c_int, c_int, c_int, c_int, u64p, u64p, c_long, u32p,
                             u64p, c_long, c_int, c_int],
        "ref128_exact_cmux": [u64p, u64p, ctypes.c_uint32, c_int, c_int, c_int, c_int],
        "ref128_uniform": [c_u64, u64p, c_long],
        "ref128_binary_key": [c_u64, u64p, c_long],
        "ref128_gen_ggsw": [c_u64, c_u64, u64p, c_int, c_int, c_int, c_int, c_dbl, u64p],
        "ref128_gen_bsk": [c_u64, u64p, c_int, u64p, c_int, c_int, c_int, c_int, c_dbl, u64p, c_int],
        "ref128_lwe_encrypt": [c_u64, u64p, c_int, u64p, c_long, c_dbl, u64p],
        "ref128_lwe_decrypt": [u64p, c_int, u64p, c_long, u64p],
    }.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = None
    _helper = L
    return L


def _p(a, t=u64p):
    return a.ctypes.data_as(t)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


# ---- u128 <-> Python integers -------------------------------------------------------------------------
def to_words(values) -> np.ndarray:
    """Python integers (taken mod 2^128) -> uint64 [len, 2] (low, high)."""
    v = [int(x) & MASK128 for x in values]
    out = np.empty((len(v), 2), dtype=np.uint64)
    out[:, 0] = [x & 0xFFFFFFFFFFFFFFFF for x in v]
    out[:, 1] = [x >> 64 for x in v]
    return out


def to_ints(words) -> list:
    w = _u64(words).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in w.tolist()]


# ---- canonical tables: big-integer fixed point --------------------------------------------------------
PREC = 320
_ONE = 1 << PREC


def _atan_inv(q: int) -> int:  # atan(1/q) in fixed point
    total, term, q2, k = 0, _ONE // q, q * q, 0
    while term:
        total += term // (2 * k + 1) if k % 2 == 0 else -(term // (2 * k + 1))
        term //= q2
        k += 1
    return total


_PI = 16 * _atan_inv(5) - 4 * _atan_inv(239)  # Machin


def _cos_sin(x: int):
    """cos and sin of the fixed-point x in [0, pi/4]."""
    x2 = x * x >> PREC
    c, term, k = 0, _ONE, 0
    while term:
        c += term if k % 2 == 0 else -term
        k += 1
        term = (term * x2 >> PREC) // ((2 * k - 1) * (2 * k))
    s, term, k = 0, x, 0
    while term:
        s += term if k % 2 == 0 else -term
        k += 1
        term = (term * x2 >> PREC) // ((2 * k) * (2 * k + 1))
    return c, s


def _to_dd(v: int):
    """hi = RN(v / 2^PREC), lo = RN(v / 2^PREC - hi): CPython's int / int is correctly rounded."""
    hi = v / _ONE
    a, b = hi.as_integer_ratio()
    r = v - a * _ONE // b
    assert (a * _ONE) % b == 0
    return hi, r / _ONE


def unit_root(u: int, N: int):
    """((cos.hi, cos.lo), (sin.hi, sin.lo)) of pi u / N, 0 <= u <= N."""
    cneg = swap = False
    if u > N // 2:
        u, cneg = N - u, True
    if u > N // 4:
        u, swap = N // 2 - u, True
    c, s = _cos_sin(_PI * u // N)
    if swap:
        c, s = s, c
    return _to_dd(-c if cneg else c), _to_dd(s)


_tables = {}


def tables(N: int):
    """(twist [4, N/2], twiddles [4, N/4]) float64 planes: re.hi, re.lo, im.hi, im.lo."""
    if N not in _tables:
        M, Q = N // 2, N // 4
        tw, w = np.empty((4, M)), np.empty((4, Q))
        for j in range(M):
            (tw[0, j], tw[1, j]), (tw[2, j], tw[3, j]) = unit_root(j, N)
        for t in range(Q):
            (w[0, t], w[1, t]), (sh, sl) = unit_root(4 * t, N)
            w[2, t], w[3, t] = -sh, -sl
        tw.setflags(write=False)
        w.setflags(write=False)
        _tables[N] = (tw, w)
    return _tables[N]


# ---- exact arithmetic on Python integers (the big-integer side of the conversion tests) ---------------
def exact_signed_dd(x: int):
    """hi = RN(signed x), lo = RN(x - hi) of a u128 word, by correctly rounded integer division."""
    s = x - (1 << 128) if x >> 127 else x
    hi = s / 1
    return hi, (s - int(hi)) / 1


def exact_torus_from_dd(hi: float, lo: float) -> int:
    """floor((x - floor x) 2^128 + 1/2) mod 2^128 of x = hi + lo, in rational arithmetic."""
    from fractions import Fraction

    x = Fraction(hi) + Fraction(lo)
    x -= x.__floor__()
    return (x * (1 << 128) + Fraction(1, 2)).__floor__() & MASK128


def closest_representable(x: int, base_log: int, level: int) -> int:
    sh = 128 - base_log * level
    return (((x + (1 << (sh - 1))) >> sh) << sh) & MASK128


def mod_distance(a: int, b: int) -> int:
    d = (a - b) & MASK128
    return min(d, (1 << 128) - d)


# ---- C-backed pieces ------------------------------------------------------------------------------------
def to_signed_dd(words):
    w = _u64(words).reshape(-1, 2)
    hi, lo = np.empty(len(w)), np.empty(len(w))
    helper().ref128_to_signed_dd(_p(w), _p(hi, f64p), _p(lo, f64p), len(w))
    return hi, lo


def torus_from_f128(hi, lo, acc=None) -> np.ndarray:
    h, l = np.ascontiguousarray(hi, dtype=np.float64).ravel(), np.ascontiguousarray(lo, dtype=np.float64).ravel()
    a = None if acc is None else _u64(acc).reshape(-1, 2)
    out = np.empty((h.size, 2), dtype=np.uint64)
    helper().ref128_torus_from_f128(_p(h, f64p), _p(l, f64p), None if a is None else _p(a), _p(out), h.size)
    return out


def decompose(words, base_log: int, level: int):
    """(digits [level, n] int64, level L first; closest_representable words [n, 2])."""
    w = _u64(words).reshape(-1, 2)
    digits, closest = np.empty((level, len(w)), dtype=np.int64), np.empty_like(w)
    helper().ref128_decompose(_p(w), len(w), base_log, level, _p(digits, i64p), _p(closest))
    return digits, closest


def roundtrip(poly) -> np.ndarray:
    w = _u64(poly).reshape(-1, 2)
    tw, tab = tables(len(w))
    out = np.empty_like(w)
    helper().ref128_roundtrip(_p(w), len(w), _p(tw, f64p), _p(tab, f64p), _p(out))
    return out


def fft_product(torus, integer) -> np.ndarray:
    w, g = _u64(torus).reshape(-1, 2), np.ascontiguousarray(integer, dtype=np.int64)
    tw, tab = tables(len(w))
    out = np.empty_like(w)
    helper().ref128_fft_product(_p(w), _p(g, i64p), len(w), _p(tw, f64p), _p(tab, f64p), _p(out))
    return out


def exact_product(torus, integer) -> np.ndarray:
    w, g = _u64(torus).reshape(-1, 2), np.ascontiguousarray(integer, dtype=np.int64)
    out = np.empty_like(w)
    helper().ref128_exact_product(_p(w), _p(g, i64p), len(w), _p(out))
    return out


def exact_cmux(acc, ggsw, at: int, N: int, k: int, base_log: int, level: int) -> np.ndarray:
    """acc + GGSW [] (X^at acc - acc) with exact products, from the standard-domain GGSW [level, k+1, k+1, N, 2]."""
    a = _u64(acc).reshape((k + 1) * N, 2).copy()
    g = _u64(ggsw).reshape(level * (k + 1) * (k + 1) * N, 2)
    helper().ref128_exact_cmux(_p(a), _p(g), at, N, k, base_log, level)
    return a


def uniform(seed: int, n: int) -> np.ndarray:
    out = np.empty((n, 2), dtype=np.uint64)
    helper().ref128_uniform(seed, _p(out), n)
    return out


def binary_key(seed: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint64)
    helper().ref128_binary_key(seed, _p(out), n)
    return out


def gen_ggsw(seed: int, bit: int, glwe_sk, k: int, N: int, base_log: int, level: int, std: float) -> np.ndarray:
    out = np.empty((level, k + 1, k + 1, N, 2), dtype=np.uint64)
    sk = _u64(glwe_sk)
    helper().ref128_gen_ggsw(seed, bit, _p(sk), k, N, base_log, level, std, _p(out))
    return out


def gen_bsk(seed: int, lwe_sk, glwe_sk, k: int, N: int, base_log: int, level: int, std: float,
            threads: int = 8) -> np.ndarray:
    ls, gs = _u64(lwe_sk), _u64(glwe_sk)
    out = np.empty((len(ls), level, k + 1, k + 1, N, 2), dtype=np.uint64)
    helper().ref128_gen_bsk(seed, _p(ls), len(ls), _p(gs), k, N, base_log, level, std, _p(out), threads)
    return out


def lwe_encrypt(seed: int, sk, plaintexts, std: float) -> np.ndarray:
    s, pt = _u64(sk), _u64(plaintexts).reshape(-1, 2)
    out = np.empty((len(pt), len(s) + 1, 2), dtype=np.uint64)
    helper().ref128_lwe_encrypt(seed, _p(s), len(s), _p(pt), len(pt), std, _p(out))
    return out


def lwe_decrypt(sk, cts) -> np.ndarray:
    s = _u64(sk)
    c = _u64(cts).reshape(-1, len(s) + 1, 2)
    out = np.empty((len(c), 2), dtype=np.uint64)
    helper().ref128_lwe_decrypt(_p(s), len(s), _p(c), len(c), _p(out))
    return out


def decode(plain_words, bits: int, modulus_log: int = 128) -> list:
    """Messages of `bits` bits under one bit of padding, rounded, from decrypted u128 words."""
    shift = modulus_log - bits - 1
    return [(((x >> (128 - modulus_log)) + (1 << (shift - 1))) >> shift) % (1 << bits) for x in to_ints(plain_words)]


def identity_accumulator(N: int, k: int, bits: int, f=lambda m: m, modulus_log: int = 128) -> np.ndarray:
    """Trivial GLWE [(k+1)N, 2] of the usual half-box-rotated LUT of f on `bits`-bit messages with padding."""
    box = N >> bits
    delta = 1 << (modulus_log - bits - 1)
    body = [(f(j // box) % (1 << bits)) * delta << (128 - modulus_log) for j in range(N)]
    body = body[box // 2:] + [-v for v in body[:box // 2]]  # negacyclic rotation by half a box
    return to_words([0] * (k * N) + body)


class RefEngine128:
    """The u128 methods of tfhe_mi355.Engine on the CPU (same signatures, same array shapes)."""

    def __init__(self, params, threads: int = 16):
        self.params = params
        self.threads = threads
        self.fbsk = None

    n = property(lambda self: self.params.lwe_dimension)
    big_dim = property(lambda self: self.params.glwe_dimension * self.params.polynomial_size)
    glwe_len = property(lambda self: (self.params.glwe_dimension + 1) * self.params.polynomial_size)

    def upload_bootstrap_key_u128(self, standard_bsk) -> None:
        p = self.params
        N = p.polynomial_size
        b = _u64(standard_bsk).reshape(-1, N, 2)
        expect = p.lwe_dimension * p.pbs_level * (p.glwe_dimension + 1) ** 2
        if len(b) != expect:
            raise ValueError(f"bootstrapping key has {len(b)} polynomials, expected {expect}")
        tw, tab = tables(N)
        self.fbsk = np.empty((len(b), 4, N // 2), dtype=np.float64)
        helper().ref128_bsk_to_fourier(_p(b), len(b), N, _p(tw, f64p), _p(tab, f64p), _p(self.fbsk, f64p))

    def _run(self, lwe_in, luts, lut_indexes, modulus_log, glwe_out):
        p = self.params
        N, k = p.polynomial_size, p.glwe_dimension
        x = _u64(lwe_in).reshape(-1, self.n + 1, 2)
        L = _u64(luts).reshape(-1, self.glwe_len, 2)
        idx = None if lut_indexes is None else np.ascontiguousarray(lut_indexes, dtype=np.uint32)
        out = np.empty((len(x), self.glwe_len if glwe_out else self.big_dim + 1, 2), dtype=np.uint64)
        tw, tab = tables(N)
        helper().ref128_pbs_batch(_p(self.fbsk, f64p), _p(tw, f64p), _p(tab, f64p), self.n, N, k, p.pbs_base_log,
                                  p.pbs_level, modulus_log, _p(x), _p(L), len(L), None if idx is None else _p(idx, u32p),
                                  _p(out), len(x), int(glwe_out), self.threads)
        return out

    def programmable_bootstrap_u128(self, lwe_in, luts, lut_indexes=None, ciphertext_modulus_log: int = 128):
        return self._run(lwe_in, luts, lut_indexes, ciphertext_modulus_log, False)

    def blind_rotate_u128(self, lwe_in, luts, lut_indexes=None, ciphertext_modulus_log: int = 128):
        return self._run(lwe_in, luts, lut_indexes, ciphertext_modulus_log, True)
