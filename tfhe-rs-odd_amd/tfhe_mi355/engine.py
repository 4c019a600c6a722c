"""Engine = one C-ABI context on one GPU (include/tfhe_mi355.h), numpy in/out or torch device
tensors in/out.  This is the object a reference `ShortintBootstrappingKey::Gpu{handle}` arm would
hold (SURVEY.md 8b seam 1).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import TfheMi355LweSource, TfheMi355Parameters, sz, u32p, u64p, vp
from .parameters import ClassicPBSParameters


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(u64p)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr32(a: np.ndarray):
    return a.ctypes.data_as(u32p)


def _dev_ptr(t) -> int:
    """Device pointer of a torch tensor (or a raw int)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    if not t.is_contiguous():
        raise ValueError("device tensors must be contiguous")
    return t.data_ptr()


def _stream_ptr(stream) -> int:
    if stream is None:
        import torch

        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def c_params(p: ClassicPBSParameters) -> TfheMi355Parameters:
    return TfheMi355Parameters(p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.pbs_base_log,
                               p.pbs_level, p.ks_base_log, p.ks_level, p.message_modulus,
                               p.carry_modulus, p.grouping_factor)


def _free_host(ptr: int) -> None:
    try:
        _lib.load().tfhe_mi355_host_free(vp(ptr))
    except Exception:  # interpreter shutdown
        pass


def pinned_empty(shape, dtype=np.uint64) -> np.ndarray:
    """An uninitialised numpy array in page-locked host memory (tfhe_mi355_host_alloc), freed with
    the array.  Batches passed to the host-pointer entry points in such arrays are DMA'd directly."""
    import weakref

    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = vp()
    _lib.call("tfhe_mi355_host_alloc", max(n, 1), ctypes.byref(p))
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
    weakref.finalize(buf, _free_host, p.value)
    return np.frombuffer(buf, dtype=np.uint8, count=n).view(dtype).reshape(shape)


class LweSource:
    """Where LWE rows come from (TfheMi355LweSource): kind "rows" ([count][n+1] expanded rows), "compact"
    (the container of an LweCompactCiphertextList), "seeded_list" (bodies + one 128-bit seed) or "seeded_rows"
    (bodies + one seed per row).  data and seeds are numpy arrays (host-pointer calls) or torch device tensors
    (async calls); seeds as Python ints are packed into {lo, hi} words."""
    KINDS = {"rows": 0, "compact": 1, "seeded_list": 2, "seeded_rows": 3}

    def __init__(self, kind, lwe_dimension: int, data, seeds=None, count=None):
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self.lwe_dimension = int(lwe_dimension)
        host = not hasattr(data, "data_ptr")
        self.data = _u64(data).ravel() if host else data
        if seeds is not None and not hasattr(seeds, "data_ptr"):
            if isinstance(seeds, np.ndarray) and seeds.dtype == np.uint64:  # {lo, hi} words already
                seeds = np.ascontiguousarray(seeds).ravel()
            else:
                ints = [seeds] if isinstance(seeds, (int, np.integer)) else list(seeds)
                seeds = np.array([[int(x) & 0xFFFFFFFFFFFFFFFF, (int(x) >> 64) & 0xFFFFFFFFFFFFFFFF] for x in ints],
                                 dtype=np.uint64).ravel()
        self.seeds = seeds
        n = self.lwe_dimension
        if count is None:
            size = self.data.size if host else self.data.numel()
            if self.kind == 0:
                count = size // (n + 1)
            elif self.kind == 1:
                raise ValueError("a compact source needs its ciphertext count")
            else:
                count = size
        self.count = int(count)
        if host:
            need = {0: self.count * (n + 1), 1: -(-self.count // n) * n + self.count}.get(self.kind, self.count)
            if self.data.size != need:
                raise ValueError(f"source data has {self.data.size} words, expected {need}")
            if self.kind in (2, 3) and (self.seeds is None or self.seeds.size != (2 if self.kind == 2 else 2 * self.count)):
                raise ValueError("seeded source: one {lo, hi} seed for a list, one per row for rows")

    def _c(self) -> TfheMi355LweSource:
        def p(a):
            if a is None:
                return None
            return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
        return TfheMi355LweSource(self.kind, self.lwe_dimension, p(self.data), p(self.seeds))


def device_count() -> int:
    n = ctypes.c_int(0)
    _lib.call("tfhe_mi355_device_count", ctypes.byref(n))
    return n.value


class Engine:
    """MI355X PBS engine context bound to `device`, or -- `devices` = a list of device ordinals
    (repeats allowed; [] = every visible GPU) -- one context over several GPUs of this process
    (tfhe_mi355_context_create_devices): keys replicated from the first device, batched calls split
    over the devices, small calls and submits spread round robin; device-tensor (async) calls run on
    the first device."""

    def __init__(self, params: ClassicPBSParameters, device: int = 0, devices=None):
        self.params = params
        self._cp = c_params(params)
        h = vp()
        if devices is None:
            self.device = device
            _lib.call("tfhe_mi355_context_create", ctypes.byref(self._cp), device, ctypes.byref(h))
        else:
            arr = (ctypes.c_int * max(len(devices), 1))(*devices)
            _lib.call("tfhe_mi355_context_create_devices", ctypes.byref(self._cp), arr, len(devices),
                      ctypes.byref(h))
        self._h = h
        self.devices = self.device_ordinals() if devices is not None else [device]
        self.device = self.devices[0]

    @property
    def multi_device(self) -> bool:
        """True for a context over several shards (tfhe_mi355_context_create_devices with > 1 entry)."""
        return len(self.devices) > 1

    def device_ordinals(self) -> list:
        """Device ordinal of each shard (one entry for a single-device context)."""
        n = sz()
        _lib.call("tfhe_mi355_context_devices", self._h, ctypes.byref(n))
        out = []
        for i in range(n.value):
            sub, dev = vp(), ctypes.c_int()
            _lib.call("tfhe_mi355_context_device_context", self._h, i, ctypes.byref(sub), ctypes.byref(dev))
            out.append(dev.value)
        return out

    REPLICATION = {0: "none", 1: "rccl", 2: "peer_copy", 3: "device_copy"}

    def replication(self):
        """How the last key replication ran ('none' | 'rccl' | 'peer_copy' | 'device_copy') and why auto
        mode did not use RCCL ('' when it did or had no need)."""
        mode, note = ctypes.c_int(), ctypes.c_char_p()
        _lib.call("tfhe_mi355_context_replication", self._h, ctypes.byref(mode), ctypes.byref(note))
        return self.REPLICATION.get(mode.value, str(mode.value)), (note.value or b"").decode()

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.call("tfhe_mi355_context_destroy", self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- sizes --------------------------------------------------------------------------
    @property
    def n(self):
        return self.params.lwe_dimension

    @property
    def big_dim(self):
        return self.params.glwe_dimension * self.params.polynomial_size

    @property
    def glwe_len(self):
        return (self.params.glwe_dimension + 1) * self.params.polynomial_size

    # -- keys ---------------------------------------------------------------------------
    def upload_bootstrap_key(self, standard_bsk: np.ndarray) -> None:
        b = _u64(standard_bsk).ravel()
        _lib.call("tfhe_mi355_bootstrap_key_upload", self._h, _ptr(b), b.size)

    def convert_bootstrap_key_device(self, d_standard_bsk, numel: int, stream=None) -> None:
        _lib.call("tfhe_mi355_bootstrap_key_convert_async", self._h, _dev_ptr(d_standard_bsk), numel,
                  _stream_ptr(stream))

    def fourier_bootstrap_key(self):
        """(device pointer, bytes) of the Fourier BSK buffer (for RCCL broadcast)."""
        p, b = vp(), ctypes.c_size_t()
        _lib.call("tfhe_mi355_bootstrap_key_fourier", self._h, ctypes.byref(p), ctypes.byref(b))
        return p.value, b.value

    def fourier_bootstrap_key_set_ready(self):
        _lib.call("tfhe_mi355_bootstrap_key_fourier_set_ready", self._h)

    def upload_keyswitch_key(self, ksk: np.ndarray) -> None:
        k = _u64(ksk).ravel()
        _lib.call("tfhe_mi355_keyswitch_key_upload", self._h, _ptr(k), k.size)

    def upload_keyswitch_key_device(self, d_ksk, numel: int, stream=None) -> None:
        _lib.call("tfhe_mi355_keyswitch_key_upload_async", self._h, _dev_ptr(d_ksk), numel, _stream_ptr(stream))

    def keyswitch_key_device(self):
        p, b = vp(), ctypes.c_size_t()
        _lib.call("tfhe_mi355_keyswitch_key_device", self._h, ctypes.byref(p), ctypes.byref(b))
        return p.value, b.value

    def keyswitch_key_set_ready(self):
        _lib.call("tfhe_mi355_keyswitch_key_set_ready", self._h)

    # -- profiling -----------------------------------------------------------------------
    def kernel_timing(self, every: int) -> None:
        """Time every `every`-th launch of each kernel family with HIP events on its stream
        (0 = off); clears the totals."""
        _lib.call("tfhe_mi355_kernel_timing_enable", self._h, int(every))

    def kernel_times(self) -> dict:
        """{kernel family: (average ms per timed launch, timed launches)}; waits for the events."""
        out = {}
        name = ctypes.create_string_buffer(128)
        tot, cnt = ctypes.c_double(), ctypes.c_uint64()
        lib = _lib.load()
        i = 0
        while lib.tfhe_mi355_kernel_timing_entry(self._h, i, name, 128, ctypes.byref(tot), ctypes.byref(cnt)) == 0:
            out[name.value.decode()] = (tot.value / max(cnt.value, 1), cnt.value)
            i += 1
        return out

    def coalesce_stats(self, reset: bool = False) -> dict:
        """Request-coalescing counters: batches, ciphertexts, most batches in flight, batch wall
        seconds (summed); `reset` clears them after reading."""
        b, r, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        t = ctypes.c_double()
        _lib.call("tfhe_mi355_coalesce_stats", self._h, int(bool(reset)), ctypes.byref(b), ctypes.byref(r),
                  ctypes.byref(m), ctypes.byref(t))
        return {"batches": b.value, "rows": r.value, "max_in_flight": m.value, "batch_seconds": t.value,
                "mean_batch_rows": r.value / b.value if b.value else None,
                "mean_batch_ms": 1e3 * t.value / b.value if b.value else None}

    # -- host (numpy) batched ops ---------------------------------------------------------
    def _luts(self, luts):
        luts = _u64(luts)
        if luts.ndim == 1:
            luts = luts.reshape(1, -1)
        if luts.shape[1] != self.glwe_len:
            raise ValueError(f"lookup table has {luts.shape[1]} words, expected {self.glwe_len}")
        return luts

    @staticmethod
    def _idx(lut_indexes, count, lut_count):
        if lut_indexes is None:
            return None, None
        idx = np.ascontiguousarray(lut_indexes, dtype=np.uint32)
        if idx.shape != (count,):
            raise ValueError("lut_indexes must have one entry per ciphertext")
        return idx, idx.ctypes.data_as(u32p)

    @staticmethod
    def _out(out, shape):
        if out is None:
            return np.empty(shape, dtype=np.uint64)
        if out.dtype != np.uint64 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint64 array of shape {shape}")
        return out

    def programmable_bootstrap(self, lwe_in, luts, lut_indexes=None, out=None) -> np.ndarray:
        """`out` (optional): the caller's output array; in and out arrays from `pinned_empty` are
        DMA'd directly by the ABI (no staging copies)."""
        x = _u64(lwe_in).reshape(-1, self.n + 1)
        L = self._luts(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = self._out(out, (x.shape[0], self.big_dim + 1))
        _lib.call("tfhe_mi355_programmable_bootstrap", self._h, _ptr(x), _ptr(out), _ptr(L), L.shape[0],
                  idxp, x.shape[0])
        return out

    def blind_rotate(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        """bootstrap_without_sample_extract (fork, fft64/crypto/bootstrap.rs:383-412): the rotated
        accumulators, [count][(k+1)N]."""
        x = _u64(lwe_in).reshape(-1, self.n + 1)
        L = self._luts(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_blind_rotate", self._h, _ptr(x), _ptr(out), _ptr(L), L.shape[0], idxp, x.shape[0])
        return out

    def keyswitch(self, lwe_in) -> np.ndarray:
        x = _u64(lwe_in).reshape(-1, self.big_dim + 1)
        out = np.empty((x.shape[0], self.n + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_keyswitch", self._h, _ptr(x), _ptr(out), x.shape[0])
        return out

    # -- keyswitching keys as objects (the keyswitches between two parameter sets) ---------------
    def keyswitch_key(self, ksk, in_dim: int, out_dim: int, base_log: int, level: int) -> "KeyswitchKey":
        """A keyswitching key [in_dim][level][out_dim+1] (levels L..1, as upload_keyswitch_key takes it) of
        its own dimensions and decomposition, on every device of the engine."""
        k = _u64(ksk).ravel()
        h = vp()
        _lib.call("tfhe_mi355_lwe_keyswitch_key_create", self._h, _ptr(k), k.size, in_dim, out_dim, base_log, level,
                  ctypes.byref(h))
        return KeyswitchKey(self, h, in_dim, out_dim, base_log, level)

    def keyswitch_with_key(self, key: "KeyswitchKey", lwe_in) -> np.ndarray:
        """keyswitch_lwe_ciphertext under `key`, batched: [count][in_dim+1] -> [count][out_dim+1]."""
        x = _u64(lwe_in).reshape(-1, key.in_dim + 1)
        out = np.empty((x.shape[0], key.out_dim + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_keyswitch_with_key", self._h, key._handle(self), _ptr(x), _ptr(out), x.shape[0])
        return out

    def keyswitch_with_key_scratch_bytes(self, key: "KeyswitchKey", count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_keyswitch_with_key_scratch", self._h, key._handle(self), count, ctypes.byref(b))
        return b.value

    def keyswitch_with_key_async(self, key: "KeyswitchKey", d_in, d_out, count: int, stream=None,
                                 d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.keyswitch_with_key_scratch_bytes(key, count), stream)
        _lib.call("tfhe_mi355_keyswitch_with_key_async", self._h, key._handle(self), _dev_ptr(d_in), _dev_ptr(d_out),
                  count, sp, sb, _stream_ptr(stream))

    def keyswitch_programmable_bootstrap(self, lwe_in, luts, lut_indexes=None, out=None) -> np.ndarray:
        x = _u64(lwe_in).reshape(-1, self.big_dim + 1)
        L = self._luts(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = self._out(out, (x.shape[0], self.big_dim + 1))
        _lib.call("tfhe_mi355_keyswitch_programmable_bootstrap", self._h, _ptr(x), _ptr(out), _ptr(L),
                  L.shape[0], idxp, x.shape[0])
        return out

    # -- asynchronous small calls (tfhe_mi355_submit / _wait, the coalescer's queue) ----------
    OPS = {"pbs": (0, "n", "big"), "ks_pbs": (1, "big", "big"), "pbs_ks": (2, "n", "n"), "ks": (3, "big", "n")}

    def submit(self, op: str, lwe_in, luts=None, lut_indexes=None) -> "Request":
        """Enqueue 1..1024 ciphertexts of `op` ("pbs", "ks_pbs", "pbs_ks", "ks") and return at once;
        `Request.wait()` returns the outputs (every request must be waited on)."""
        code, din, dout = self.OPS[op]
        w_in = (self.n if din == "n" else self.big_dim) + 1
        w_out = (self.n if dout == "n" else self.big_dim) + 1
        x = np.ascontiguousarray(_u64(lwe_in).reshape(-1, w_in))
        if code == 3:
            L, idx, idxp = np.zeros((1, 1), dtype=np.uint64), None, None
        else:
            L = self._luts(luts)
            idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], w_out), dtype=np.uint64)
        h = ctypes.c_void_p()
        _lib.call("tfhe_mi355_submit", self._h, code, _ptr(x), _ptr(out), _ptr(L), 0 if code == 3 else L.shape[0],
                  idxp, x.shape[0], ctypes.byref(h))
        return Request(h, (x, L, idx, out))

    def programmable_bootstrap_keyswitch(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        x = _u64(lwe_in).reshape(-1, self.n + 1)
        L = self._luts(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], self.n + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_programmable_bootstrap_keyswitch", self._h, _ptr(x), _ptr(out), _ptr(L),
                  L.shape[0], idxp, x.shape[0])
        return out

    def upload_compressed_server_key(self, data: bytes) -> None:
        """Both keys of a bincode-serialized shortint CompressedServerKey (serialization.py)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.call("tfhe_mi355_compressed_server_key_upload", self._h,
                  buf.ctypes.data_as(_lib.u8p), buf.size)

    def upload_server_key(self, data: bytes) -> None:
        """Both keys of a bincode-serialized shortint ServerKey (Fourier BSK, serialization.py)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.call("tfhe_mi355_server_key_upload", self._h, buf.ctypes.data_as(_lib.u8p), buf.size)

    def upload_seeded_bootstrap_key(self, bodies: np.ndarray, compression_seed: int) -> None:
        """decompress_seeded_lwe_bootstrap_key on the GPU + Fourier conversion."""
        b = _u64(bodies)
        _lib.call("tfhe_mi355_bootstrap_key_upload_seeded", self._h, _ptr(b), b.size,
                  compression_seed & 0xFFFFFFFFFFFFFFFF, (compression_seed >> 64) & 0xFFFFFFFFFFFFFFFF)

    def upload_seeded_keyswitch_key(self, bodies: np.ndarray, compression_seed: int) -> None:
        """decompress_seeded_lwe_keyswitch_key on the GPU."""
        b = _u64(bodies)
        _lib.call("tfhe_mi355_keyswitch_key_upload_seeded", self._h, _ptr(b), b.size,
                  compression_seed & 0xFFFFFFFFFFFFFFFF, (compression_seed >> 64) & 0xFFFFFFFFFFFFFFFF)

    def csprng_mask_words(self, compression_seed: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=np.uint64)
        _lib.call("tfhe_mi355_csprng_mask_words", self._h, compression_seed & 0xFFFFFFFFFFFFFFFF,
                  (compression_seed >> 64) & 0xFFFFFFFFFFFFFFFF, _ptr(out), count)
        return out

    def upload_packing_keyswitch_key(self, pksk: np.ndarray, base_log: int, level: int) -> None:
        k = _u64(pksk)
        _lib.call("tfhe_mi355_packing_keyswitch_key_upload", self._h, _ptr(k), k.size, base_log, level)

    def packing_keyswitch(self, lwe_in) -> np.ndarray:
        """keyswitch_lwe_ciphertext_into_glwe_ciphertext (lwe_packing_keyswitch.rs:102-186), batched."""
        x = _u64(lwe_in).reshape(-1, self.big_dim + 1)
        out = np.empty((x.shape[0], self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_packing_keyswitch", self._h, _ptr(x), _ptr(out), x.shape[0])
        return out

    def glwe_poly_mul(self, glwe_in, polys, extract: bool = False) -> np.ndarray:
        """out[c][i] = sum_j glwe_in[c][j] * polys[i][j] (negacyclic, wrapping), optionally sample-
        extracted: glwe_in [count][J][(k+1)N], polys [npoly][J][N]."""
        N = self.params.polynomial_size
        g = _u64(glwe_in)
        if g.ndim == 2:
            g = g.reshape(g.shape[0], 1, -1)
        v = _u64(polys)
        if v.ndim == 2:
            v = v.reshape(v.shape[0], 1, -1)
        count, J = g.shape[0], g.shape[1]
        if g.shape[2] != self.glwe_len or v.shape[1] != J or v.shape[2] != N:
            raise ValueError("glwe_poly_mul: shape mismatch")
        out = np.empty((count, v.shape[0], self.big_dim + 1 if extract else self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_glwe_poly_mul", self._h, _ptr(g), J, _ptr(v), v.shape[0], count, int(extract), _ptr(out))
        return out

    # -- GLWE x GLWE product with relinearisation (the gadget layer's lwe_mult) ------------------
    def upload_relinearization_key(self, rlk: np.ndarray, base_log: int, level: int) -> None:
        """RelinearizationKey [k(k+1)/2][level][(k+1)N], level L first (the reference's memory as it is);
        its decomposition belongs to the key."""
        k = _u64(rlk)
        _lib.call("tfhe_mi355_relinearization_key_upload", self._h, _ptr(k), k.size, base_log, level)

    def glwe_mult(self, lhs, rhs, log_p: int, extract: bool = False) -> np.ndarray:
        """glwe_mult (custom_glwe_glwe_product.rs:13-64), batched: both [count][(k+1)N] GLWEs shifted right
        by 32 - log_p/2, tensored and relinearised; with extract the degree-0 sample, [count][kN+1]."""
        a = _u64(lhs).reshape(-1, self.glwe_len)
        b = _u64(rhs).reshape(-1, self.glwe_len)
        if a.shape != b.shape:
            raise ValueError("glwe_mult: lhs and rhs differ in shape")
        out = np.empty((a.shape[0], self.big_dim + 1 if extract else self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_glwe_mult", self._h, _ptr(a), _ptr(b), log_p, int(extract), _ptr(out), a.shape[0])
        return out

    def lwe_mult(self, lhs, rhs, log_p: int) -> np.ndarray:
        """The ciphertext half of lwe_mult (gadget/engine/mod.rs:680-751), batched: both [count][kN+1] LWEs
        packed by one packing-keyswitch launch, multiplied, sample-extracted."""
        a = _u64(lhs).reshape(-1, self.big_dim + 1)
        b = _u64(rhs).reshape(-1, self.big_dim + 1)
        if a.shape != b.shape:
            raise ValueError("lwe_mult: lhs and rhs differ in shape")
        out = np.empty_like(a)
        _lib.call("tfhe_mi355_lwe_mult", self._h, _ptr(a), _ptr(b), log_p, _ptr(out), a.shape[0])
        return out

    def glwe_mult_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_glwe_mult_scratch", count)

    def lwe_mult_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_lwe_mult_scratch", count)

    def glwe_mult_async(self, d_lhs, d_rhs, log_p: int, extract: bool, d_out, count: int, stream=None,
                        d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.glwe_mult_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_glwe_mult_async", self._h, _dev_ptr(d_lhs), _dev_ptr(d_rhs), log_p, int(extract),
                  _dev_ptr(d_out), count, sp, sb, _stream_ptr(stream))

    def lwe_mult_async(self, d_lhs, d_rhs, log_p: int, d_out, count: int, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.lwe_mult_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_lwe_mult_async", self._h, _dev_ptr(d_lhs), _dev_ptr(d_rhs), log_p, _dev_ptr(d_out),
                  count, sp, sb, _stream_ptr(stream))

    # -- GGSW operations: per-item GGSW ciphertexts, decomposition chosen per call -----------
    def ggsw_words(self, level: int) -> int:
        """u64 words of one standard-domain GGSW: [level][k+1][(k+1)N]."""
        k1 = self.params.glwe_dimension + 1
        return level * k1 * k1 * self.params.polynomial_size

    def _ggsw_list(self, ggsw_list, level: int) -> np.ndarray:
        g = _u64(ggsw_list)
        if g.size == 0 or g.size % self.ggsw_words(level):
            raise ValueError(f"GGSW list of {g.size} words is no multiple of {self.ggsw_words(level)}")
        return g.reshape(-1, self.ggsw_words(level))

    def ggsw_external_product(self, ggsw_list, base_log: int, level: int, glwe_in, glwe_inout,
                              ggsw_indexes=None) -> np.ndarray:
        """glwe_inout[i] += ggsw[i] (x) glwe_in[i] (add_external_product_assign, fft64/crypto/ggsw.rs:
        477-598), batched; returns the accumulated array (glwe_inout itself when it is a C-contiguous
        uint64 array).  ggsw_indexes picks each item's GGSW (None: item i uses GGSW i)."""
        g = self._ggsw_list(ggsw_list, level)
        x = _u64(glwe_in).reshape(-1, self.glwe_len)
        out = _u64(glwe_inout).reshape(-1, self.glwe_len)
        if out.shape != x.shape:
            raise ValueError("ggsw_external_product: glwe_in and glwe_inout differ in shape")
        idx, idxp = self._idx(ggsw_indexes, x.shape[0], g.shape[0])
        _lib.call("tfhe_mi355_ggsw_external_product", self._h, _ptr(g), g.shape[0], base_log, level, idxp, _ptr(x),
                  _ptr(out), x.shape[0])
        return out

    def ggsw_cmux(self, ggsw_list, base_log: int, level: int, ct0, ct1, ggsw_indexes=None, out=None) -> np.ndarray:
        """out[i] = ct0[i] + ggsw[i] (x) (ct1[i] - ct0[i]) (cmux, fft64/crypto/ggsw.rs:766-777), batched;
        `out` may be ct0 itself."""
        g = self._ggsw_list(ggsw_list, level)
        a = _u64(ct0).reshape(-1, self.glwe_len)
        b = _u64(ct1).reshape(-1, self.glwe_len)
        if a.shape != b.shape:
            raise ValueError("ggsw_cmux: ct0 and ct1 differ in shape")
        idx, idxp = self._idx(ggsw_indexes, a.shape[0], g.shape[0])
        out = self._out(out, a.shape)
        _lib.call("tfhe_mi355_ggsw_cmux", self._h, _ptr(g), g.shape[0], base_log, level, idxp, _ptr(a), _ptr(b),
                  _ptr(out), a.shape[0])
        return out

    def vertical_packing(self, ggsw_list, base_log: int, level: int, luts, lut_indexes=None) -> np.ndarray:
        """vertical_packing (fft64/crypto/wop_pbs/mod.rs:785-853), batched: ggsw_list [count][nbits]
        GGSWs (index bits, most significant first), luts [lut_count][npoly][N] (or [npoly][N]);
        returns [count][kN+1]."""
        N = self.params.polynomial_size
        g = _u64(ggsw_list)
        if g.ndim < 2:
            raise ValueError("vertical_packing: ggsw_list must be [count][nbits] GGSWs")
        count = g.shape[0]
        g = g.reshape(count, -1)
        if g.shape[1] == 0 or g.shape[1] % self.ggsw_words(level):
            raise ValueError(f"vertical_packing: {g.shape[1]} words per item is no multiple of one GGSW")
        nbits = g.shape[1] // self.ggsw_words(level)
        L = _u64(luts)
        if L.ndim == 2:
            L = L.reshape(1, *L.shape)
        if L.ndim != 3 or L.shape[2] != N:
            raise ValueError("vertical_packing: luts must be [lut_count][npoly][N]")
        idx, idxp = self._idx(lut_indexes, count, L.shape[0])
        out = np.empty((count, self.big_dim + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_vertical_packing", self._h, _ptr(g), base_log, level, nbits, _ptr(L), L.shape[0],
                  L.shape[1], idxp, count, _ptr(out))
        return out

    # -- WoP-PBS, the bootstrapped half: pfpks, bit extraction, circuit bootstrap -------------
    def upload_pfpksk_list(self, pfpksk: np.ndarray, base_log: int, level: int) -> None:
        """LwePrivateFunctionalPackingKeyswitchKeyList [k+1][kN+1][level][(k+1)N], level 1 first (the
        reference's memory as it is); its decomposition belongs to the key."""
        k = _u64(pfpksk)
        _lib.call("tfhe_mi355_pfpksk_list_upload", self._h, _ptr(k), k.size, base_log, level)

    def private_functional_packing_keyswitch(self, lwe_in) -> np.ndarray:
        """private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext under every key of the
        list, batched: [count][kN+1] -> [count][k+1][(k+1)N]."""
        x = _u64(lwe_in).reshape(-1, self.big_dim + 1)
        out = np.empty((x.shape[0], self.params.glwe_dimension + 1, self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_private_functional_packing_keyswitch", self._h, _ptr(x), _ptr(out), x.shape[0])
        return out

    def extract_bits(self, lwe_in, delta_log: int, nbits: int) -> np.ndarray:
        """extract_bits (wop_pbs/mod.rs:66-225), batched: [count][kN+1] -> [count][nbits][n+1], most
        significant bit first, each at q/2."""
        if nbits <= 0 or delta_log < 0 or delta_log + nbits > 64 or (delta_log == 0 and nbits > 1):
            raise ValueError(f"extract_bits: delta_log {delta_log}, nbits {nbits} out of range")
        x = _u64(lwe_in).reshape(-1, self.big_dim + 1)
        out = np.empty((x.shape[0], nbits, self.n + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_extract_bits", self._h, _ptr(x), delta_log, nbits, _ptr(out), x.shape[0])
        return out

    def circuit_bootstrap(self, lwe_in, delta_log: int, cbs_base_log: int, cbs_level: int) -> np.ndarray:
        """circuit_bootstrap_boolean (wop_pbs/mod.rs:243-444), batched: [count][n+1] ->
        [count][cbs_level][k+1][(k+1)N] standard-domain GGSWs."""
        if not 0 <= delta_log <= 63:
            raise ValueError(f"circuit_bootstrap: delta_log {delta_log} out of range")
        x = _u64(lwe_in).reshape(-1, self.n + 1)
        out = np.empty((x.shape[0], cbs_level, self.params.glwe_dimension + 1, self.glwe_len), dtype=np.uint64)
        _lib.call("tfhe_mi355_circuit_bootstrap", self._h, _ptr(x), delta_log, cbs_base_log, cbs_level, _ptr(out),
                  x.shape[0])
        return out

    def _wop_luts(self, luts) -> np.ndarray:
        N = self.params.polynomial_size
        L = _u64(luts)
        if L.ndim == 2:
            L = L.reshape(1, 1, *L.shape)
        elif L.ndim == 3:
            L = L.reshape(1, *L.shape)
        if L.ndim != 4 or L.shape[3] != N:
            raise ValueError("luts must be [lut_count][nout][npoly][N]")
        return L

    def circuit_bootstrap_vertical_packing(self, lwe_in, cbs_base_log: int, cbs_level: int, luts,
                                           lut_indexes=None) -> np.ndarray:
        """circuit_bootstrap_boolean_vertical_packing (wop_pbs/mod.rs:647-746), batched: lwe_in
        [count][nbits][n+1] (bits at q/2, most significant first), luts [lut_count][nout][npoly][N] (or
        [nout][npoly][N], [npoly][N]); returns [count][nout][kN+1]."""
        x = _u64(lwe_in)
        if x.ndim != 3 or x.shape[2] != self.n + 1 or x.shape[1] == 0:
            raise ValueError("circuit_bootstrap_vertical_packing: lwe_in must be [count][nbits][n+1]")
        L = self._wop_luts(luts)
        count, nbits = x.shape[0], x.shape[1]
        idx, idxp = self._idx(lut_indexes, count, L.shape[0])
        out = np.empty((count, L.shape[1], self.big_dim + 1), dtype=np.uint64)
        _lib.call("tfhe_mi355_circuit_bootstrap_vertical_packing", self._h, _ptr(x), nbits, cbs_base_log, cbs_level,
                  _ptr(L), L.shape[0], L.shape[1], L.shape[2], idxp, count, _ptr(out))
        return out

    def pfpks_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_private_functional_packing_keyswitch_scratch", count)

    def extract_bits_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_extract_bits_scratch", count)

    def circuit_bootstrap_scratch_bytes(self, cbs_level: int, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_circuit_bootstrap_scratch", self._h, cbs_level, count, ctypes.byref(b))
        return b.value

    def circuit_bootstrap_vertical_packing_scratch_bytes(self, nbits: int, cbs_level: int, lut_count: int, nout: int,
                                                         npoly: int, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_circuit_bootstrap_vertical_packing_scratch", self._h, nbits, cbs_level, lut_count, nout,
                  npoly, count, ctypes.byref(b))
        return b.value

    def private_functional_packing_keyswitch_async(self, d_in, d_out, count: int, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pfpks_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_private_functional_packing_keyswitch_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out),
                  count, sp, sb, _stream_ptr(stream))

    def extract_bits_async(self, d_in, delta_log: int, nbits: int, d_out, count: int, stream=None,
                           d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.extract_bits_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_extract_bits_async", self._h, _dev_ptr(d_in), delta_log, nbits, _dev_ptr(d_out), count,
                  sp, sb, _stream_ptr(stream))

    def circuit_bootstrap_async(self, d_in, delta_log: int, cbs_base_log: int, cbs_level: int, d_ggsw_out, count: int,
                                stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.circuit_bootstrap_scratch_bytes(cbs_level, count), stream)
        _lib.call("tfhe_mi355_circuit_bootstrap_async", self._h, _dev_ptr(d_in), delta_log, cbs_base_log, cbs_level,
                  _dev_ptr(d_ggsw_out), count, sp, sb, _stream_ptr(stream))

    def circuit_bootstrap_vertical_packing_async(self, d_in, nbits: int, cbs_base_log: int, cbs_level: int, d_luts,
                                                 lut_count: int, nout: int, npoly: int, count: int, d_out,
                                                 d_lut_indexes=None, stream=None, d_scratch=None) -> None:
        need = self.circuit_bootstrap_vertical_packing_scratch_bytes(nbits, cbs_level, lut_count, nout, npoly, count)
        sp, sb, _keep = self._scratch(d_scratch, need, stream)
        _lib.call("tfhe_mi355_circuit_bootstrap_vertical_packing_async", self._h, _dev_ptr(d_in), nbits, cbs_base_log,
                  cbs_level, _dev_ptr(d_luts), lut_count, nout, npoly, _dev_ptr(d_lut_indexes), count, _dev_ptr(d_out),
                  sp, sb, _stream_ptr(stream))

    # -- device (torch) async ops -------------------------------------------------------
    # Every device scratch the C ABI needs comes from the caller (include/tfhe_mi355.h): pass
    # d_scratch (>= the matching *_scratch_bytes), or let these wrappers allocate it from torch's
    # caching allocator for the call.
    # -- 32-bit torus (the reference's boolean module; include/tfhe_mi355.h "32-bit torus") ------------
    # Host arrays are uint32; device tensors are torch.int32 (same bits).  A context holds keys of one
    # torus width; these calls are single-device.
    def upload_bootstrap_key_u32(self, standard_bsk) -> None:
        b = _u32(standard_bsk).ravel()
        _lib.call("tfhe_mi355_bootstrap_key_upload_u32", self._h, _ptr32(b), b.size)

    def upload_keyswitch_key_u32(self, ksk) -> None:
        k = _u32(ksk).ravel()
        _lib.call("tfhe_mi355_keyswitch_key_upload_u32", self._h, _ptr32(k), k.size)

    def _luts32(self, luts):
        luts = _u32(luts)
        if luts.ndim == 1:
            luts = luts.reshape(1, -1)
        if luts.shape[1] != self.glwe_len:
            raise ValueError(f"lookup table has {luts.shape[1]} words, expected {self.glwe_len}")
        return luts

    def programmable_bootstrap_u32(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        x = _u32(lwe_in).reshape(-1, self.n + 1)
        L = self._luts32(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], self.big_dim + 1), dtype=np.uint32)
        _lib.call("tfhe_mi355_programmable_bootstrap_u32", self._h, _ptr32(x), _ptr32(out), _ptr32(L), L.shape[0],
                  idxp, x.shape[0])
        return out

    def blind_rotate_u32(self, lwe_in, luts, lut_indexes=None) -> np.ndarray:
        x = _u32(lwe_in).reshape(-1, self.n + 1)
        L = self._luts32(luts)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], self.glwe_len), dtype=np.uint32)
        _lib.call("tfhe_mi355_blind_rotate_u32", self._h, _ptr32(x), _ptr32(out), _ptr32(L), L.shape[0], idxp,
                  x.shape[0])
        return out

    def keyswitch_u32(self, lwe_in) -> np.ndarray:
        x = _u32(lwe_in).reshape(-1, self.big_dim + 1)
        out = np.empty((x.shape[0], self.n + 1), dtype=np.uint32)
        _lib.call("tfhe_mi355_keyswitch_u32", self._h, _ptr32(x), _ptr32(out), x.shape[0])
        return out

    def gate_words(self, pbs_order: int) -> int:
        """Words per ciphertext row of a gate call: n+1 for pbs_order 1 (BootstrapKeyswitch), kN+1 for 0."""
        return (self.n if pbs_order else self.big_dim) + 1

    def boolean_gates(self, ops, lhs, rhs, pbs_order: int) -> np.ndarray:
        """A mixed batch of binary gates (opcodes 0 AND, 1 NAND, 2 NOR, 3 OR, 4 XOR, 5 XNOR)."""
        w = self.gate_words(pbs_order)
        a, b = _u32(lhs).reshape(-1, w), _u32(rhs).reshape(-1, w)
        o = np.ascontiguousarray(ops, dtype=np.uint8).ravel()
        if a.shape != b.shape or o.size != a.shape[0]:
            raise ValueError("ops, lhs and rhs must have one entry per gate")
        out = np.empty_like(a)
        _lib.call("tfhe_mi355_boolean_gates", self._h, o.ctypes.data_as(_lib.u8p), _ptr32(a), _ptr32(b), _ptr32(out),
                  a.shape[0], int(pbs_order))
        return out

    def boolean_mux(self, cond, then_ct, else_ct, pbs_order: int) -> np.ndarray:
        w = self.gate_words(pbs_order)
        c, t, e = (_u32(x).reshape(-1, w) for x in (cond, then_ct, else_ct))
        if not (c.shape == t.shape == e.shape):
            raise ValueError("cond, then and else must have the same shape")
        out = np.empty_like(c)
        _lib.call("tfhe_mi355_boolean_mux", self._h, _ptr32(c), _ptr32(t), _ptr32(e), _ptr32(out), c.shape[0],
                  int(pbs_order))
        return out

    def boolean_not(self, ct) -> np.ndarray:
        """NOT negates every word (boolean/engine/mod.rs:377-398); host arrays need no kernel."""
        return (np.uint32(0) - _u32(ct)).astype(np.uint32)

    def _scratch_query_order(self, fn: str, count: int, pbs_order: int) -> int:
        b = ctypes.c_size_t()
        _lib.call(fn, self._h, count, int(pbs_order), ctypes.byref(b))
        return b.value

    def pbs_u32_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_programmable_bootstrap_u32_scratch", count)

    def ks_u32_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_keyswitch_u32_scratch", count)

    def boolean_gates_scratch_bytes(self, count: int, pbs_order: int) -> int:
        return self._scratch_query_order("tfhe_mi355_boolean_gates_scratch", count, pbs_order)

    def boolean_mux_scratch_bytes(self, count: int, pbs_order: int) -> int:
        return self._scratch_query_order("tfhe_mi355_boolean_mux_scratch", count, pbs_order)

    def programmable_bootstrap_u32_async(self, d_in, d_out, d_luts, lut_count: int, count: int, d_lut_indexes=None,
                                         stream=None, d_scratch=None, glwe_out: bool = False) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pbs_u32_scratch_bytes(count), stream)
        fn = "tfhe_mi355_blind_rotate_u32_async" if glwe_out else "tfhe_mi355_programmable_bootstrap_u32_async"
        _lib.call(fn, self._h, _dev_ptr(d_in), _dev_ptr(d_out), _dev_ptr(d_luts), lut_count,
                  _dev_ptr(d_lut_indexes), count, sp, sb, _stream_ptr(stream))

    def blind_rotate_u32_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_blind_rotate_u32_scratch", count)

    def blind_rotate_u32_async(self, d_in, d_glwe_out, d_luts, lut_count: int, count: int, d_lut_indexes=None,
                               stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.blind_rotate_u32_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_blind_rotate_u32_async", self._h, _dev_ptr(d_in), _dev_ptr(d_glwe_out), _dev_ptr(d_luts),
                  lut_count, _dev_ptr(d_lut_indexes), count, sp, sb, _stream_ptr(stream))

    def keyswitch_u32_async(self, d_in, d_out, count: int, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.ks_u32_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_keyswitch_u32_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out), count, sp, sb,
                  _stream_ptr(stream))

    def boolean_gates_async(self, d_ops, d_lhs, d_rhs, d_out, count: int, pbs_order: int, stream=None,
                            d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.boolean_gates_scratch_bytes(count, pbs_order), stream)
        _lib.call("tfhe_mi355_boolean_gates_async", self._h, _dev_ptr(d_ops), _dev_ptr(d_lhs), _dev_ptr(d_rhs),
                  _dev_ptr(d_out), count, int(pbs_order), sp, sb, _stream_ptr(stream))

    def boolean_mux_async(self, d_cond, d_then, d_else, d_out, count: int, pbs_order: int, stream=None,
                          d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.boolean_mux_scratch_bytes(count, pbs_order), stream)
        _lib.call("tfhe_mi355_boolean_mux_async", self._h, _dev_ptr(d_cond), _dev_ptr(d_then), _dev_ptr(d_else),
                  _dev_ptr(d_out), count, int(pbs_order), sp, sb, _stream_ptr(stream))

    def boolean_not_async(self, d_in, d_out, words: int, stream=None) -> None:
        _lib.call("tfhe_mi355_boolean_not_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out), words,
                  _stream_ptr(stream))

    def debug_keyswitch_u32(self, ksk, in_dim: int, out_dim: int, base_log: int, level: int, lwe_in,
                            arm: int = 0) -> np.ndarray:
        """One u32 keyswitch under `ksk` [in_dim][level][out_dim+1] through kernel `arm` (0 the engine's choice,
        1 integer, 2 int8 MFMA); a test hook, the context's keys are not touched."""
        k = _u32(ksk).ravel()
        if k.size != in_dim * level * (out_dim + 1):
            raise ValueError("keyswitching key size")
        x = _u32(lwe_in).reshape(-1, in_dim + 1)
        out = np.empty((x.shape[0], out_dim + 1), dtype=np.uint32)
        _lib.call("tfhe_mi355_debug_keyswitch_u32", self._h, _ptr32(k), in_dim, out_dim, base_log, level, arm,
                  _ptr32(x), _ptr32(out), x.shape[0])
        return out

    def pbs_u32_resident(self) -> int:
        """Ciphertexts (= workgroups) of the u32 PBS kernel resident at once on the device."""
        n = sz()
        _lib.call("tfhe_mi355_debug_pbs_u32_resident", self._h, ctypes.byref(n))
        return n.value

    # -- 128-bit torus (the reference's fft128 path; include/tfhe_mi355.h "128-bit torus") -------------
    # A u128 word is two uint64 (low, high): host arrays are uint64 of shape [..., words, 2], device
    # tensors torch.int64 of the same shape.  A context holds keys of one torus width; single-device.
    @classmethod
    def for_u128(cls, params, device: int = 0) -> "Engine":
        """A context validated against the f128 kernel's limits (tfhe_mi355_context_create_u128) instead of
        the u64 kernels'; it serves the _u128 calls only."""
        self = cls.__new__(cls)
        self.params = params
        self._cp = c_params(params)
        h = vp()
        _lib.call("tfhe_mi355_context_create_u128", ctypes.byref(self._cp), device, ctypes.byref(h))
        self._h = h
        self.devices = [device]
        self.device = device
        return self

    @staticmethod
    def _u128(a, words: int) -> np.ndarray:
        a = _u64(a)
        if a.ndim < 1 or a.shape[-1] != 2:
            raise ValueError("u128 arrays are uint64 of shape [..., 2] (low, high)")
        return a.reshape(-1, words, 2)

    def upload_bootstrap_key_u128(self, standard_bsk) -> None:
        b = _u64(standard_bsk)
        if b.ndim < 1 or b.shape[-1] != 2:
            raise ValueError("u128 arrays are uint64 of shape [..., 2] (low, high)")
        b = b.ravel()
        _lib.call("tfhe_mi355_bootstrap_key_upload_u128", self._h, _ptr(b), b.size // 2)

    def _call_u128(self, fn: str, lwe_in, luts, lut_indexes, ciphertext_modulus_log: int, out_words: int):
        x = self._u128(lwe_in, self.n + 1)
        L = _u64(luts)
        if L.ndim < 2 or L.shape[-1] != 2 or L.shape[-2] != self.glwe_len:
            raise ValueError(f"lookup tables are uint64 of shape [..., {self.glwe_len}, 2]")
        L = L.reshape(-1, self.glwe_len, 2)
        idx, idxp = self._idx(lut_indexes, x.shape[0], L.shape[0])
        out = np.empty((x.shape[0], out_words, 2), dtype=np.uint64)
        _lib.call(fn, self._h, _ptr(x), _ptr(out), _ptr(L), L.shape[0], idxp, x.shape[0],
                  int(ciphertext_modulus_log))
        return out

    def programmable_bootstrap_u128(self, lwe_in, luts, lut_indexes=None, ciphertext_modulus_log: int = 128):
        """[count, n+1, 2] -> [count, kN+1, 2]; luts [lut_count, (k+1)N, 2] general GLWE accumulators."""
        return self._call_u128("tfhe_mi355_programmable_bootstrap_u128", lwe_in, luts, lut_indexes,
                               ciphertext_modulus_log, self.big_dim + 1)

    def blind_rotate_u128(self, lwe_in, luts, lut_indexes=None, ciphertext_modulus_log: int = 128):
        """The blind rotation without the sample extraction: [count, (k+1)N, 2]."""
        return self._call_u128("tfhe_mi355_blind_rotate_u128", lwe_in, luts, lut_indexes, ciphertext_modulus_log,
                               self.glwe_len)

    def pbs_u128_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_programmable_bootstrap_u128_scratch", count)

    def blind_rotate_u128_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_blind_rotate_u128_scratch", count)

    def programmable_bootstrap_u128_async(self, d_in, d_out, d_luts, lut_count: int, count: int, d_lut_indexes=None,
                                          ciphertext_modulus_log: int = 128, stream=None, d_scratch=None,
                                          glwe_out: bool = False) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pbs_u128_scratch_bytes(count), stream)
        fn = "tfhe_mi355_blind_rotate_u128_async" if glwe_out else "tfhe_mi355_programmable_bootstrap_u128_async"
        _lib.call(fn, self._h, _dev_ptr(d_in), _dev_ptr(d_out), _dev_ptr(d_luts), lut_count,
                  _dev_ptr(d_lut_indexes), count, int(ciphertext_modulus_log), sp, sb, _stream_ptr(stream))

    def blind_rotate_u128_async(self, d_in, d_out, d_luts, lut_count: int, count: int, **kw) -> None:
        self.programmable_bootstrap_u128_async(d_in, d_out, d_luts, lut_count, count, glwe_out=True, **kw)

    def pbs_u128_resident(self) -> int:
        """Ciphertexts (= workgroups) of the f128 PBS kernel resident at once on the device."""
        n = sz()
        _lib.call("tfhe_mi355_debug_pbs_u128_resident", self._h, ctypes.byref(n))
        return n.value

    def _scratch_query(self, fn: str, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call(fn, self._h, count, ctypes.byref(b))
        return b.value

    def pbs_resident(self) -> int:
        """Workgroups of the classic u64 PBS kernel resident at once on the device: its persistent grid
        (0: the shape has none)."""
        n = sz()
        _lib.call("tfhe_mi355_debug_pbs_resident", self._h, ctypes.byref(n))
        return n.value

    def pbs_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_programmable_bootstrap_scratch", count)

    def ks_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_keyswitch_scratch", count)

    def pks_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_packing_keyswitch_scratch", count)

    def ks_pbs_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_keyswitch_programmable_bootstrap_scratch", count)

    def pbs_ks_scratch_bytes(self, count: int) -> int:
        return self._scratch_query("tfhe_mi355_programmable_bootstrap_keyswitch_scratch", count)

    def _scratch(self, d_scratch, need: int, stream):
        """(pointer, bytes, keep-alive) of the scratch for one async call."""
        if d_scratch is not None:
            nbytes = d_scratch.numel() * d_scratch.element_size() if hasattr(d_scratch, "numel") else need
            return _dev_ptr(d_scratch), nbytes, d_scratch
        if need == 0:
            return None, 0, None
        import torch

        t = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self.device))
        # The tensor is freed when the wrapper returns, while the kernel may still run: tell the
        # caching allocator which stream uses the block so it is not handed out before that
        # stream reaches this point (raw int handles are wrapped as an ExternalStream).
        if isinstance(stream, int):
            stream = torch.cuda.ExternalStream(stream, device=t.device)
        if stream is not None and stream != torch.cuda.current_stream(t.device):
            t.record_stream(stream)
        return t.data_ptr(), need, t

    def programmable_bootstrap_async(self, d_in, d_out, d_luts, lut_count: int, count: int,
                                     d_lut_indexes=None, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pbs_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_programmable_bootstrap_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out),
                  _dev_ptr(d_luts), lut_count, _dev_ptr(d_lut_indexes), count, sp, sb, _stream_ptr(stream))

    def blind_rotate_async(self, d_in, d_glwe_out, d_luts, lut_count: int, count: int, d_lut_indexes=None,
                           stream=None) -> None:
        _lib.call("tfhe_mi355_blind_rotate_async", self._h, _dev_ptr(d_in), _dev_ptr(d_glwe_out), _dev_ptr(d_luts),
                  lut_count, _dev_ptr(d_lut_indexes), count, _stream_ptr(stream))

    def keyswitch_async(self, d_in, d_out, count: int, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.ks_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_keyswitch_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out), count, sp, sb,
                  _stream_ptr(stream))

    def keyswitch_programmable_bootstrap_async(self, d_in, d_out, d_luts, lut_count: int, count: int,
                                               d_scratch=None, d_lut_indexes=None, stream=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.ks_pbs_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_keyswitch_programmable_bootstrap_async", self._h, _dev_ptr(d_in),
                  _dev_ptr(d_out), _dev_ptr(d_luts), lut_count, _dev_ptr(d_lut_indexes), count,
                  sp, sb, _stream_ptr(stream))

    def programmable_bootstrap_keyswitch_async(self, d_in, d_out, d_luts, lut_count: int, count: int,
                                               d_scratch=None, d_lut_indexes=None, stream=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pbs_ks_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_programmable_bootstrap_keyswitch_async", self._h, _dev_ptr(d_in),
                  _dev_ptr(d_out), _dev_ptr(d_luts), lut_count, _dev_ptr(d_lut_indexes), count,
                  sp, sb, _stream_ptr(stream))

    # -- compressed ciphertext ingress (tfhe_mi355_lwe_expand*, tfhe_mi355_apply_from*) -------------------
    def lwe_expand(self, source: LweSource) -> np.ndarray:
        """The expanded rows [count][n+1] of a host source (CompactCiphertextList::expand,
        CompressedCiphertext::decompress, decompress_seeded_lwe_ciphertext_list), written on the GPU."""
        out = np.empty((source.count, source.lwe_dimension + 1), dtype=np.uint64)
        c = source._c()
        _lib.call("tfhe_mi355_lwe_expand", self._h, ctypes.byref(c), source.count, _ptr(out))
        return out

    def lwe_expand_scratch_bytes(self, kind: int, lwe_dimension: int, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_lwe_expand_scratch", self._h, kind, lwe_dimension, count, ctypes.byref(b))
        return b.value

    def lwe_expand_async(self, d_source: LweSource, d_out, stream=None, d_scratch=None) -> None:
        need = self.lwe_expand_scratch_bytes(d_source.kind, d_source.lwe_dimension, d_source.count)
        sp, sb, _keep = self._scratch(d_scratch, need, stream)
        c = d_source._c()
        _lib.call("tfhe_mi355_lwe_expand_async", self._h, ctypes.byref(c), d_source.count, _dev_ptr(d_out), sp, sb,
                  _stream_ptr(stream))

    def apply_from(self, op: str, source: LweSource, luts=None, lut_indexes=None, out=None) -> np.ndarray:
        """`op` ("pbs", "ks_pbs", "pbs_ks", "ks") on the rows of a host source, expanded on the GPU chunk by
        chunk: the outputs of lwe_expand followed by the operation's own call, bit for bit.  `out` (optional):
        the caller's output array (one from `pinned_empty` is DMA'd into directly)."""
        code, _din, dout = self.OPS[op]
        w_out = (self.n if dout == "n" else self.big_dim) + 1
        count = source.count
        if code == 3:
            L, idxp, nl = None, None, 0
        else:
            L = self._luts(luts)
            idx, idxp = self._idx(lut_indexes, count, L.shape[0])
            nl = L.shape[0]
        out = self._out(out, (count, w_out))
        c = source._c()
        _lib.call("tfhe_mi355_apply_from", self._h, code, ctypes.byref(c), _ptr(out), None if L is None else _ptr(L),
                  nl, idxp, count)
        return out

    def apply_from_scratch_bytes(self, op: str, kind: int, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_apply_from_scratch", self._h, self.OPS[op][0], kind, count, ctypes.byref(b))
        return b.value

    def apply_from_async(self, op: str, d_source: LweSource, d_out, d_luts=None, lut_count: int = 0,
                         d_lut_indexes=None, stream=None, d_scratch=None) -> None:
        need = self.apply_from_scratch_bytes(op, d_source.kind, d_source.count)
        sp, sb, _keep = self._scratch(d_scratch, need, stream)
        c = d_source._c()
        _lib.call("tfhe_mi355_apply_from_async", self._h, self.OPS[op][0], ctypes.byref(c), _dev_ptr(d_out),
                  _dev_ptr(d_luts), lut_count, _dev_ptr(d_lut_indexes), d_source.count, sp, sb, _stream_ptr(stream))

    def lwe_scalar_mul_add_async(self, y_ptr: int, x_ptr, scalar: int, rows: int, words: int, y_stride: int,
                                 x_stride: int = 0, stream=None) -> None:
        """y[r] = y[r] * scalar + x[r] (u64 wrapping) on device rows (raw pointers: strided views allowed)."""
        _lib.call("tfhe_mi355_lwe_scalar_mul_add_async", self._h, y_ptr, x_ptr, scalar % (1 << 64), rows, words,
                  y_stride, x_stride, _stream_ptr(stream))

    @staticmethod
    def block_ops(ops):
        """The C table of a block layer from [(dst_ptr, dst_stride, body_add, [(src_ptr, stride, scalar), ...])]
        (raw device pointers, strides in words, at most 4 terms per op).  A table can be kept and passed to
        lwe_block_layer_async again."""
        table = (_lib.TfheMi355BlockOp * max(len(ops), 1))()
        for o, (dst, dst_stride, body_add, terms) in zip(table, ops):
            if len(terms) > _lib.BLOCK_OP_TERMS:
                raise ValueError(f"a block op takes at most {_lib.BLOCK_OP_TERMS} terms, got {len(terms)}")
            o.dst, o.dst_stride, o.body_add = dst, dst_stride, body_add % (1 << 64)
            for t, (src, stride, scalar) in zip(o.term, terms):
                t.src, t.stride, t.scalar = src, stride, scalar % (1 << 64)
        return table, len(ops)

    def lwe_block_layer_async(self, ops, rows: int, words: int, stream=None) -> None:
        """One layer of block arithmetic in one launch: for every op, dst[r] = sum_t scalar_t * src_t[r] with
        body_add on the last word (u64 wrapping), r < rows, `words` words per row.  `ops` is a list as block_ops
        takes it, or what block_ops returned.  A term may be the destination itself (same pointer and stride);
        any other overlap with a destination is the caller's error."""
        table, n = ops if isinstance(ops, tuple) else self.block_ops(ops)
        _lib.call("tfhe_mi355_lwe_block_layer_async", self._h, table, n, rows, words, _stream_ptr(stream))

    @staticmethod
    def clear_block_ops(ops):
        """The C table of a block layer with a clear digit per row, from
        [(dst_ptr, dst_stride, body_add, terms, clear)]: the first four as block_ops takes them, `clear` None (a
        plain op) or a dict with any of d_clear (device pointer of one u64 per row), negate, shift, bits, scale,
        d_lut_index (device pointer of one u32 per row) and lut_base; what is absent is 0 / NULL.  A table can be
        kept and passed to lwe_clear_block_layer_async again."""
        table = (_lib.TfheMi355ClearBlockOp * max(len(ops), 1))()
        for c, (dst, dst_stride, body_add, terms, clear) in zip(table, ops):
            if len(terms) > _lib.BLOCK_OP_TERMS:
                raise ValueError(f"a block op takes at most {_lib.BLOCK_OP_TERMS} terms, got {len(terms)}")
            o = c.op
            o.dst, o.dst_stride, o.body_add = dst, dst_stride, body_add % (1 << 64)
            for t, (src, stride, scalar) in zip(o.term, terms):
                t.src, t.stride, t.scalar = src, stride, scalar % (1 << 64)
            clear = clear or {}
            unknown = set(clear) - {"d_clear", "negate", "shift", "bits", "scale", "d_lut_index", "lut_base"}
            if unknown:
                raise ValueError(f"unknown fields of a clear block op: {sorted(unknown)}")
            c.d_clear, c.d_lut_index = clear.get("d_clear"), clear.get("d_lut_index")
            c.clear_negate, c.clear_shift = int(bool(clear.get("negate", 0))), clear.get("shift", 0)
            c.clear_bits, c.lut_base = clear.get("bits", 0), clear.get("lut_base", 0)
            c.clear_scale = clear.get("scale", 0) % (1 << 64)
        return table, len(ops)

    def lwe_clear_block_layer_async(self, ops, rows: int, words: int, stream=None) -> None:
        """lwe_block_layer_async with a clear digit per row, read from the device: per op and row r,
        digit = ((negate ? -d_clear[r] : d_clear[r]) >> shift) & (2^bits - 1); digit * scale is added to the body
        of row r and lut_base + digit written to d_lut_index[r].  `ops` is a list as clear_block_ops takes it, or
        what clear_block_ops returned."""
        table, n = ops if isinstance(ops, tuple) else self.clear_block_ops(ops)
        _lib.call("tfhe_mi355_lwe_clear_block_layer_async", self._h, table, n, rows, words, _stream_ptr(stream))

    def trivial_pbs_async(self, body_ptr: int, rows: int, stride: int, d_lut, stream=None) -> None:
        _lib.call("tfhe_mi355_trivial_pbs_async", self._h, body_ptr, rows, stride, _dev_ptr(d_lut),
                  _stream_ptr(stream))

    def packing_keyswitch_async(self, d_in, d_out, count: int, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.pks_scratch_bytes(count), stream)
        _lib.call("tfhe_mi355_packing_keyswitch_async", self._h, _dev_ptr(d_in), _dev_ptr(d_out), count, sp, sb,
                  _stream_ptr(stream))

    def glwe_poly_mul_async(self, d_glwe, glwe_per_item: int, d_polys, npoly: int, count: int, extract: bool,
                            d_out, stream=None) -> None:
        _lib.call("tfhe_mi355_glwe_poly_mul_async", self._h, _dev_ptr(d_glwe), glwe_per_item, _dev_ptr(d_polys),
                  npoly, count, int(extract), _dev_ptr(d_out), _stream_ptr(stream))

    def ggsw_list_fourier_bytes(self, ggsw_count: int, level: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_ggsw_list_fourier_bytes", self._h, ggsw_count, level, ctypes.byref(b))
        return b.value

    def ggsw_list_convert_async(self, d_ggsw_list, ggsw_count: int, level: int, d_fourier, stream=None) -> None:
        """Standard -> Fourier GGSW list on the device, for the async forms below."""
        _lib.call("tfhe_mi355_ggsw_list_convert_async", self._h, _dev_ptr(d_ggsw_list), ggsw_count, level,
                  _dev_ptr(d_fourier), _stream_ptr(stream))

    def ggsw_external_product_async(self, d_fourier, ggsw_count: int, base_log: int, level: int, d_glwe_in,
                                    d_glwe_inout, count: int, d_ggsw_indexes=None, stream=None) -> None:
        _lib.call("tfhe_mi355_ggsw_external_product_async", self._h, _dev_ptr(d_fourier), ggsw_count, base_log, level,
                  _dev_ptr(d_ggsw_indexes), _dev_ptr(d_glwe_in), _dev_ptr(d_glwe_inout), count, _stream_ptr(stream))

    def ggsw_cmux_async(self, d_fourier, ggsw_count: int, base_log: int, level: int, d_ct0, d_ct1, d_out,
                        count: int, d_ggsw_indexes=None, stream=None) -> None:
        _lib.call("tfhe_mi355_ggsw_cmux_async", self._h, _dev_ptr(d_fourier), ggsw_count, base_log, level,
                  _dev_ptr(d_ggsw_indexes), _dev_ptr(d_ct0), _dev_ptr(d_ct1), _dev_ptr(d_out), count,
                  _stream_ptr(stream))

    def vertical_packing_scratch_bytes(self, npoly: int, count: int) -> int:
        b = ctypes.c_size_t()
        _lib.call("tfhe_mi355_vertical_packing_scratch", self._h, npoly, count, ctypes.byref(b))
        return b.value

    def vertical_packing_async(self, d_fourier, base_log: int, level: int, nbits: int, d_luts, lut_count: int,
                               npoly: int, count: int, d_out, d_lut_indexes=None, stream=None, d_scratch=None) -> None:
        sp, sb, _keep = self._scratch(d_scratch, self.vertical_packing_scratch_bytes(npoly, count), stream)
        _lib.call("tfhe_mi355_vertical_packing_async", self._h, _dev_ptr(d_fourier), base_log, level, nbits,
                  _dev_ptr(d_luts), lut_count, npoly, _dev_ptr(d_lut_indexes), count, _dev_ptr(d_out), sp, sb,
                  _stream_ptr(stream))


def debug_torus32_from_fraction(fr, acc=None, device: int = 0):
    """(acc + X, X) with X = rint_half_even(fr * 2^32) mod 2^32, computed by the u32 PBS kernel's conversion."""
    f = np.ascontiguousarray(fr, dtype=np.float64).ravel()
    a = np.zeros(f.size, dtype=np.uint32) if acc is None else _u32(acc).ravel().copy()
    x = np.empty(f.size, dtype=np.uint32)
    _lib.call("tfhe_mi355_debug_torus32_from_fraction", device, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
              _ptr32(a), _ptr32(x), f.size)
    return a, x


def debug_fft128_tables(N: int):
    """(twist [4, N/2], twiddles [4, N/4]): the engine's canonical double-double tables (host only)."""
    f64p = ctypes.POINTER(ctypes.c_double)
    tw, w = np.empty((4, N // 2), dtype=np.float64), np.empty((4, N // 4), dtype=np.float64)
    _lib.call("tfhe_mi355_debug_fft128_tables", N, tw.ctypes.data_as(f64p), w.ctypes.data_as(f64p))
    return tw, w


def debug_torus128_from_f128(hi, lo, acc=None, device: int = 0) -> np.ndarray:
    """acc + X ([count, 2] uint64), X the f128 kernel's backward conversion of the double-double hi + lo."""
    f64p = ctypes.POINTER(ctypes.c_double)
    h = np.ascontiguousarray(hi, dtype=np.float64).ravel()
    l = np.ascontiguousarray(lo, dtype=np.float64).ravel()
    if h.size != l.size:
        raise ValueError("hi and lo must have the same size")
    a = None if acc is None else _u64(acc).reshape(h.size, 2)
    out = np.empty((h.size, 2), dtype=np.uint64)
    _lib.call("tfhe_mi355_debug_torus128_from_f128", device, h.ctypes.data_as(f64p), l.ctypes.data_as(f64p),
              None if a is None else _ptr(a), _ptr(out), h.size)
    return out


def fill_accumulator(params: ClassicPBSParameters, f) -> np.ndarray:
    """shortint fill_accumulator (shortint/engine/mod.rs:72-128) through the C ABI."""
    p = params.message_modulus * params.carry_modulus
    fv = _u64([int(f(i)) & 0xFFFFFFFFFFFFFFFF for i in range(p)])
    acc = np.zeros((params.glwe_dimension + 1) * params.polynomial_size, dtype=np.uint64)
    cp = c_params(params)
    _lib.call("tfhe_mi355_fill_accumulator", ctypes.byref(cp), _ptr(fv), _ptr(acc))
    return acc


class KeyswitchKey:
    """Handle of a keyswitching key object (Engine.keyswitch_key); it keeps its engine alive and is freed
    with the last reference (or close())."""

    def __init__(self, engine: Engine, handle, in_dim: int, out_dim: int, base_log: int, level: int):
        self.engine, self._h = engine, handle
        self.in_dim, self.out_dim, self.base_log, self.level = in_dim, out_dim, base_log, level

    def _handle(self, engine: Engine):
        if engine is not self.engine:
            raise ValueError("keyswitching key belongs to another engine")
        if not self._h or not self._h.value:
            raise ValueError("keyswitching key already closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.call("tfhe_mi355_lwe_keyswitch_key_destroy", self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Request:
    """Handle of a submitted small call (Engine.submit): keeps the host buffers alive until wait()."""

    def __init__(self, handle, buffers):
        self._h, self._bufs = handle, buffers

    def wait(self) -> np.ndarray:
        if self._h is None:
            raise RuntimeError("request already waited on")
        h, self._h = self._h, None
        _lib.call("tfhe_mi355_wait", h)
        return self._bufs[3]

    def __del__(self):
        # Dropped without wait() (e.g. an exception between a loop of submits and the waits): the
        # dispatcher may still copy from / into the numpy buffers this object keeps alive, so block
        # until the request is done (this also frees its native handle); errors are ignored here.
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                _lib.load().tfhe_mi355_wait(h)
            except Exception:  # interpreter shutdown
                pass
