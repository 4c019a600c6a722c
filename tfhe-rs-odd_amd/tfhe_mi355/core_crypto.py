"""Mirror of the reference core_crypto entry points on the PBS path, backed by the HIP engine.

  convert_standard_lwe_bootstrap_key_to_fourier   lwe_bootstrap_key_conversion.rs:21-151
  programmable_bootstrap_lwe_ciphertext           lwe_programmable_bootstrapping.rs:1017-1111
  multi_bit_programmable_bootstrap_lwe_ciphertext lwe_multi_bit_programmable_bootstrapping.rs:1035-1128
  keyswitch_lwe_ciphertext                        lwe_keyswitch.rs:96-170
  add_external_product_assign                     lwe_programmable_bootstrapping.rs:309-473
  cmux_assign                                     lwe_programmable_bootstrapping.rs:552-763
  vertical_packing                                fft_impl/fft64/crypto/wop_pbs/mod.rs:785-853

Argument meaning and error behaviour follow the reference: output buffers are caller-owned and
overwritten; dimension mismatches raise (the reference asserts, lwe_programmable_bootstrapping.rs
:1088-1102, lwe_keyswitch.rs:106-141).  The `_batch` forms are the engine's native shape.
"""
from __future__ import annotations

import numpy as np

from .engine import Engine
from .parameters import ClassicPBSParameters


class FourierLweBootstrapKey:
    """Fourier-domain BSK resident on one GPU (FourierLweBootstrapKey, bootstrap.rs:27-173)."""

    def __init__(self, engine: Engine):
        self.engine = engine

    @property
    def input_lwe_dimension(self):
        return self.engine.params.lwe_dimension

    @property
    def output_lwe_dimension(self):
        return self.engine.big_dim

    @property
    def polynomial_size(self):
        return self.engine.params.polynomial_size

    @property
    def glwe_size(self):
        return self.engine.params.glwe_dimension + 1


class LweKeyswitchKey:
    """Keyswitching key resident on one GPU (entities/lwe_keyswitch_key.rs)."""

    def __init__(self, engine: Engine):
        self.engine = engine

    @property
    def input_key_lwe_dimension(self):
        return self.engine.big_dim

    @property
    def output_key_lwe_dimension(self):
        return self.engine.params.lwe_dimension


def convert_standard_lwe_bootstrap_key_to_fourier(standard_bsk: np.ndarray, params: ClassicPBSParameters,
                                                  device: int = 0, engine: Engine | None = None
                                                  ) -> FourierLweBootstrapKey:
    eng = engine or Engine(params, device)
    eng.upload_bootstrap_key(standard_bsk)
    return FourierLweBootstrapKey(eng)


def upload_keyswitch_key(ksk: np.ndarray, params: ClassicPBSParameters, device: int = 0,
                         engine: Engine | None = None) -> LweKeyswitchKey:
    eng = engine or Engine(params, device)
    eng.upload_keyswitch_key(ksk)
    return LweKeyswitchKey(eng)


def programmable_bootstrap_lwe_ciphertext(input_ct: np.ndarray, output_ct: np.ndarray, accumulator: np.ndarray,
                                          fourier_bsk: FourierLweBootstrapKey) -> None:
    eng = fourier_bsk.engine
    if input_ct.shape[-1] != eng.n + 1:
        raise ValueError(f"input LweDimension {input_ct.shape[-1] - 1} != bsk input {eng.n}")
    if output_ct.shape[-1] != eng.big_dim + 1:
        raise ValueError(f"output LweDimension {output_ct.shape[-1] - 1} != bsk output {eng.big_dim}")
    output_ct[...] = eng.programmable_bootstrap(input_ct, accumulator).reshape(output_ct.shape)


def programmable_bootstrap_lwe_ciphertext_batch(inputs: np.ndarray, accumulators: np.ndarray,
                                                fourier_bsk: FourierLweBootstrapKey,
                                                lut_indexes=None) -> np.ndarray:
    return fourier_bsk.engine.programmable_bootstrap(inputs, accumulators, lut_indexes)


def multi_bit_programmable_bootstrap_lwe_ciphertext(input_ct: np.ndarray, output_ct: np.ndarray,
                                                    accumulator: np.ndarray, multi_bit_bsk: FourierLweBootstrapKey,
                                                    thread_count: int = 0) -> None:
    """The multi-bit PBS (deterministic group order); `thread_count` is accepted for signature
    parity with the reference and ignored (the GPU kernel fuses the keybundle producers)."""
    if not multi_bit_bsk.engine.params.grouping_factor:
        raise ValueError("multi_bit_programmable_bootstrap_lwe_ciphertext needs a multi-bit key")
    programmable_bootstrap_lwe_ciphertext(input_ct, output_ct, accumulator, multi_bit_bsk)


def keyswitch_lwe_ciphertext(ksk: LweKeyswitchKey, input_ct: np.ndarray, output_ct: np.ndarray) -> None:
    eng = ksk.engine
    if input_ct.shape[-1] != eng.big_dim + 1:
        raise ValueError("Mismatched input LweDimension")
    if output_ct.shape[-1] != eng.n + 1:
        raise ValueError("Mismatched output LweDimension")
    output_ct[...] = eng.keyswitch(input_ct).reshape(output_ct.shape)


def keyswitch_lwe_ciphertext_batch(ksk: LweKeyswitchKey, inputs: np.ndarray) -> np.ndarray:
    return ksk.engine.keyswitch(inputs)


class GgswCiphertextList:
    """GGSW ciphertexts in the standard domain with their decomposition (GgswCiphertextList,
    entities/ggsw_ciphertext_list.rs): data [count][level][k+1][(k+1)N], level l at index l-1 -- the
    layout of one bootstrap-key element.  Unlike the bootstrap key these are data of the call: the
    engine converts them to the Fourier domain on the device each time."""

    def __init__(self, data, glwe_size: int, polynomial_size: int, base_log: int, level: int):
        self.glwe_size, self.polynomial_size = glwe_size, polynomial_size
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        words = level * glwe_size * glwe_size * polynomial_size
        d = np.ascontiguousarray(data, dtype=np.uint64)
        if d.size == 0 or d.size % words:
            raise ValueError(f"GGSW list of {d.size} words is no multiple of one GGSW ({words} words)")
        self.data = d.reshape(-1, words)

    def __len__(self):
        return self.data.shape[0]


def _check_glwe(name: str, glwe: np.ndarray, ggsw: GgswCiphertextList) -> None:
    if glwe.shape[-1] != ggsw.glwe_size * ggsw.polynomial_size:
        raise ValueError(f"Mismatched GlweSize / PolynomialSize: {name} has {glwe.shape[-1]} words per GLWE, the "
                         f"GGSW {ggsw.glwe_size} x {ggsw.polynomial_size}")


def _check_engine(engine: Engine, ggsw: GgswCiphertextList) -> None:
    p = engine.params
    if (p.glwe_dimension + 1, p.polynomial_size) != (ggsw.glwe_size, ggsw.polynomial_size):
        raise ValueError("the engine's GlweSize / PolynomialSize differ from the GGSW's")


def add_external_product_assign(out: np.ndarray, ggsw: GgswCiphertextList, glwe: np.ndarray, engine: Engine,
                                ggsw_indexes=None) -> None:
    """out += ggsw (x) glwe, per item (reference order: out, ggsw, glwe).  The reference asserts equal
    sizes (lwe_programmable_bootstrapping.rs:320-340); a mismatch raises here."""
    _check_glwe("glwe", glwe, ggsw)
    _check_glwe("out", out, ggsw)
    if out.shape != glwe.shape:
        raise ValueError("out and glwe differ in shape")
    count = out.size // out.shape[-1]
    if ggsw_indexes is None and len(ggsw) != count:
        raise ValueError(f"{len(ggsw)} GGSWs for {count} GLWE ciphertexts")
    _check_engine(engine, ggsw)
    out[...] = engine.ggsw_external_product(ggsw.data, ggsw.decomposition_base_log, ggsw.decomposition_level_count,
                                            glwe, out.copy(), ggsw_indexes).reshape(out.shape)


def cmux_assign(ct0: np.ndarray, ct1: np.ndarray, ggsw: GgswCiphertextList, engine: Engine,
                ggsw_indexes=None) -> None:
    """ct0 <- ct0 + ggsw (x) (ct1 - ct0), per item (reference order: ct0, ct1, ggsw).  The reference
    also leaves ct1 - ct0 in ct1; here ct1 is untouched."""
    _check_glwe("ct0", ct0, ggsw)
    _check_glwe("ct1", ct1, ggsw)
    if ct0.shape != ct1.shape:
        raise ValueError("ct0 and ct1 differ in shape")
    count = ct0.size // ct0.shape[-1]
    if ggsw_indexes is None and len(ggsw) != count:
        raise ValueError(f"{len(ggsw)} GGSWs for {count} GLWE ciphertexts")
    _check_engine(engine, ggsw)
    ct0[...] = engine.ggsw_cmux(ggsw.data, ggsw.decomposition_base_log, ggsw.decomposition_level_count, ct0, ct1,
                                ggsw_indexes).reshape(ct0.shape)


def vertical_packing(lut: np.ndarray, lwe_out: np.ndarray, ggsw_list: GgswCiphertextList, engine: Engine) -> None:
    """lwe_out <- LUT[index] for the index whose bits the GGSWs encrypt, most significant first
    (reference order: lut, lwe_out, ggsw_list).  lut [npoly][N]; one item: every GGSW of the list is
    an index bit.  Engine.vertical_packing is the batched form."""
    if lut.ndim != 2 or lut.shape[1] != ggsw_list.polynomial_size:
        raise ValueError("lut must be [polynomial_count][PolynomialSize]")
    npoly = lut.shape[0]
    if npoly == 0 or npoly & (npoly - 1):
        raise ValueError(f"the LUT has {npoly} polynomials, not a power of two")
    nbits, log_n = len(ggsw_list), ggsw_list.polynomial_size.bit_length() - 1
    if npoly.bit_length() - 1 > nbits:
        raise ValueError(f"{npoly} LUT polynomials need {npoly.bit_length() - 1} GGSWs, {nbits} given")
    if nbits - (npoly.bit_length() - 1) > log_n:
        raise ValueError(f"{nbits - (npoly.bit_length() - 1)} rotation bits exceed log2(N) = {log_n}")
    lwe_dim = (ggsw_list.glwe_size - 1) * ggsw_list.polynomial_size
    if lwe_out.shape[-1] != lwe_dim + 1:
        raise ValueError(f"Output LWE ciphertext needs an LweDimension of {lwe_dim}, got {lwe_out.shape[-1] - 1}")
    _check_engine(engine, ggsw_list)
    lwe_out[...] = engine.vertical_packing(ggsw_list.data.reshape(1, -1), ggsw_list.decomposition_base_log,
                                           ggsw_list.decomposition_level_count, lut).reshape(lwe_out.shape)
