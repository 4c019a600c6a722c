"""Mirror of the reference core_crypto entry points on the PBS path, backed by the HIP engine.

  convert_standard_lwe_bootstrap_key_to_fourier   lwe_bootstrap_key_conversion.rs:21-151
  programmable_bootstrap_lwe_ciphertext           lwe_programmable_bootstrapping.rs:1017-1111
  multi_bit_programmable_bootstrap_lwe_ciphertext lwe_multi_bit_programmable_bootstrapping.rs:1035-1128
  keyswitch_lwe_ciphertext                        lwe_keyswitch.rs:96-170
  add_external_product_assign                     lwe_programmable_bootstrapping.rs:309-473
  cmux_assign                                     lwe_programmable_bootstrapping.rs:552-763
  vertical_packing                                fft_impl/fft64/crypto/wop_pbs/mod.rs:785-853
  private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext
                                                  lwe_private_functional_packing_keyswitch.rs:21-89
  extract_bits_from_lwe_ciphertext                lwe_wopbs.rs (extract_bits, wop_pbs/mod.rs:66-225)
  circuit_bootstrap_boolean                       wop_pbs/mod.rs:243-444
  circuit_bootstrap_boolean_vertical_packing      wop_pbs/mod.rs:647-746

  convert_standard_lwe_bootstrap_key_to_fourier_128
                                                  lwe_bootstrap_key_conversion.rs:164
  programmable_bootstrap_f128_lwe_ciphertext      lwe_programmable_bootstrapping.rs:1378-1459

  expand_lwe_compact_ciphertext_list              lwe_compact_ciphertext_list_expansion.rs:12-58 (par_: 61-107)
  decompress_seeded_lwe_ciphertext_list           seeded_lwe_ciphertext_list_decompression.rs:13-100
  decompress_seeded_lwe_ciphertext                seeded_lwe_ciphertext_decompression.rs:50-73

Argument meaning and error behaviour follow the reference: output buffers are caller-owned and
overwritten; dimension mismatches raise (the reference asserts, lwe_programmable_bootstrapping.rs
:1088-1102, lwe_keyswitch.rs:106-141).  The `_batch` forms are the engine's native shape.
"""
from __future__ import annotations

import numpy as np

from .engine import Engine, LweSource
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


class Fourier128LweBootstrapKey:
    """Fourier128LweBootstrapKey (fft128/crypto/bootstrap.rs:24-110) resident on one engine: any object with
    the u128 methods of Engine (upload_bootstrap_key_u128, programmable_bootstrap_u128, n, big_dim, params)."""

    def __init__(self, engine):
        self.engine = engine

    @property
    def input_lwe_dimension(self):
        return self.engine.n

    @property
    def output_lwe_dimension(self):
        return self.engine.big_dim

    @property
    def polynomial_size(self):
        return self.engine.params.polynomial_size

    @property
    def glwe_size(self):
        return self.engine.params.glwe_dimension + 1


def convert_standard_lwe_bootstrap_key_to_fourier_128(standard_bsk: np.ndarray, params: ClassicPBSParameters,
                                                      device: int = 0, engine=None) -> Fourier128LweBootstrapKey:
    """standard_bsk: uint64 [n, level, k+1, k+1, N, 2] (u128 words as low, high)."""
    eng = engine or Engine.for_u128(params, device)
    eng.upload_bootstrap_key_u128(standard_bsk)
    return Fourier128LweBootstrapKey(eng)


def _check_f128(input_shape, output_shape, accumulator_shape, eng) -> None:
    # lwe_programmable_bootstrapping.rs:1378-1426: the three dimension assertions
    if len(input_shape) < 2 or input_shape[-1] != 2 or input_shape[-2] != eng.n + 1:
        raise ValueError(f"Input LWE ciphertext and the bootstrap key's input LweDimension {eng.n} differ "
                         f"(input shape {tuple(input_shape)}, u128 words as [..., n+1, 2])")
    if output_shape is not None and (len(output_shape) < 2 or output_shape[-1] != 2
                                     or output_shape[-2] != eng.big_dim + 1):
        raise ValueError(f"Output LWE ciphertext and the bootstrap key's output LweDimension {eng.big_dim} differ "
                         f"(output shape {tuple(output_shape)})")
    glwe_len = (eng.params.glwe_dimension + 1) * eng.params.polynomial_size
    if len(accumulator_shape) < 2 or accumulator_shape[-1] != 2 or accumulator_shape[-2] != glwe_len:
        raise ValueError(f"Accumulator and the bootstrap key's GlweSize / PolynomialSize differ "
                         f"(accumulator shape {tuple(accumulator_shape)}, expected [..., {glwe_len}, 2])")


def programmable_bootstrap_f128_lwe_ciphertext(input_ct: np.ndarray, output_ct: np.ndarray, accumulator: np.ndarray,
                                               fourier_bsk: Fourier128LweBootstrapKey,
                                               ciphertext_modulus_log: int = 128) -> None:
    """input [n+1, 2], output [kN+1, 2] (overwritten), accumulator [(k+1)N, 2]: uint64 (low, high) u128 words.
    The reference reads the modulus from the ciphertexts; here it is the last argument (128 = native)."""
    eng = fourier_bsk.engine
    _check_f128(np.shape(input_ct), np.shape(output_ct), np.shape(accumulator), eng)
    output_ct[...] = eng.programmable_bootstrap_u128(
        input_ct, accumulator, ciphertext_modulus_log=ciphertext_modulus_log).reshape(output_ct.shape)


def programmable_bootstrap_f128_lwe_ciphertext_batch(inputs: np.ndarray, accumulators: np.ndarray,
                                                     fourier_bsk: Fourier128LweBootstrapKey, lut_indexes=None,
                                                     ciphertext_modulus_log: int = 128) -> np.ndarray:
    eng = fourier_bsk.engine
    _check_f128(np.shape(inputs), None, np.shape(accumulators), eng)
    return eng.programmable_bootstrap_u128(inputs, accumulators, lut_indexes,
                                           ciphertext_modulus_log=ciphertext_modulus_log)


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


class LwePrivateFunctionalPackingKeyswitchKeyList:
    """The circuit bootstrap's private functional packing keyswitching keys
    (entities/lwe_private_functional_packing_keyswitch_key_list.rs): data
    [k+1 keys][input LweSize][level][(k+1)N], level l at index l-1, resident on the engine's GPU."""

    def __init__(self, data, input_lwe_dimension: int, glwe_size: int, polynomial_size: int, base_log: int,
                 level: int, engine: Engine):
        self.input_key_lwe_dimension = input_lwe_dimension
        self.glwe_size, self.output_polynomial_size = glwe_size, polynomial_size
        self.decomposition_base_log, self.decomposition_level_count = base_log, level
        words = glwe_size * (input_lwe_dimension + 1) * level * glwe_size * polynomial_size
        d = np.ascontiguousarray(data, dtype=np.uint64)
        if d.size != words:
            raise ValueError(f"pfpksk list of {d.size} words, expected {words} ([k+1][LweSize][level][(k+1)N])")
        p = engine.params
        if (p.glwe_dimension + 1, p.polynomial_size) != (glwe_size, polynomial_size) or engine.big_dim != input_lwe_dimension:
            raise ValueError("the engine's GlweSize / PolynomialSize / big LweDimension differ from the key list's")
        self.engine = engine
        engine.upload_pfpksk_list(d, base_log, level)

    def __len__(self):
        return self.glwe_size


def private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext(
        pfpksk: LwePrivateFunctionalPackingKeyswitchKeyList, key_index: int, output_glwe: np.ndarray,
        input_lwe: np.ndarray) -> None:
    """output_glwe <- pfpks of input_lwe under key `key_index` of the list (reference order: key, output,
    input; the reference takes one key of the list, the engine runs them all in one launch)."""
    if input_lwe.shape[-1] != pfpksk.input_key_lwe_dimension + 1:
        raise ValueError("Mismatched input LweDimension")
    if output_glwe.shape[-1] != pfpksk.glwe_size * pfpksk.output_polynomial_size:
        raise ValueError("Mismatched output GlweSize / PolynomialSize")
    if not 0 <= key_index < len(pfpksk):
        raise ValueError(f"key index {key_index} outside the list of {len(pfpksk)} keys")
    out = pfpksk.engine.private_functional_packing_keyswitch(input_lwe)
    output_glwe[...] = out[:, key_index].reshape(output_glwe.shape)


def extract_bits_from_lwe_ciphertext(lwe_in: np.ndarray, lwe_list_out: np.ndarray,
                                     fourier_bsk: FourierLweBootstrapKey, ksk: LweKeyswitchKey, delta_log: int,
                                     number_of_bits_to_extract: int) -> None:
    """lwe_list_out [nbits][n+1] <- the bits of lwe_in, most significant first (reference order)."""
    eng = fourier_bsk.engine
    if ksk.engine is not eng:
        raise ValueError("the bootstrap key and the keyswitch key live on different engines")
    if 64 < delta_log + number_of_bits_to_extract:
        raise ValueError(f"Tried to extract {number_of_bits_to_extract} bits, while the maximum number of extractable "
                         f"bits for delta_log {delta_log} is {64 - delta_log}")
    if lwe_in.shape[-1] != eng.big_dim + 1:
        raise ValueError(f"lwe_in needs to have an LWE dimension of {eng.big_dim}, got {lwe_in.shape[-1] - 1}")
    if lwe_list_out.shape[-1] != eng.n + 1:
        raise ValueError(f"lwe_list_out needs to have an LWE dimension of {eng.n}, got {lwe_list_out.shape[-1] - 1}")
    if lwe_list_out.size // lwe_list_out.shape[-1] != number_of_bits_to_extract * (lwe_in.size // lwe_in.shape[-1]):
        raise ValueError(f"lwe_list_out needs to have a ciphertext count of {number_of_bits_to_extract}")
    lwe_list_out[...] = eng.extract_bits(lwe_in, delta_log, number_of_bits_to_extract).reshape(lwe_list_out.shape)


def circuit_bootstrap_boolean(fourier_bsk: FourierLweBootstrapKey, lwe_in: np.ndarray, ggsw_out: GgswCiphertextList,
                              delta_log: int, pfpksk_list: LwePrivateFunctionalPackingKeyswitchKeyList) -> None:
    """ggsw_out <- GGSW encryptions of the bit at 2^delta_log of every lwe_in, with ggsw_out's
    decomposition (reference order: bsk, lwe_in, ggsw_out, delta_log, pfpksk_list)."""
    eng = fourier_bsk.engine
    if pfpksk_list.engine is not eng:
        raise ValueError("the bootstrap key and the pfpksk list live on different engines")
    if lwe_in.shape[-1] != eng.n + 1:
        raise ValueError(f"lwe_in needs to have an LWE dimension of {eng.n}, got {lwe_in.shape[-1] - 1}")
    if (ggsw_out.glwe_size, ggsw_out.polynomial_size) != (pfpksk_list.glwe_size, pfpksk_list.output_polynomial_size):
        raise ValueError("The output GGSW ciphertext needs the GlweSize and PolynomialSize of the pfpksks")
    if len(ggsw_out) != lwe_in.size // lwe_in.shape[-1]:
        raise ValueError(f"{len(ggsw_out)} output GGSWs for {lwe_in.size // lwe_in.shape[-1]} input ciphertexts")
    ggsw_out.data[...] = eng.circuit_bootstrap(lwe_in, delta_log, ggsw_out.decomposition_base_log,
                                               ggsw_out.decomposition_level_count).reshape(ggsw_out.data.shape)


def circuit_bootstrap_boolean_vertical_packing(big_lut_as_polynomial_list: np.ndarray,
                                               fourier_bsk: FourierLweBootstrapKey, lwe_list_out: np.ndarray,
                                               lwe_list_in: np.ndarray,
                                               pfpksk_list: LwePrivateFunctionalPackingKeyswitchKeyList,
                                               level_cbs: int, base_log_cbs: int) -> None:
    """lwe_list_out [nout][kN+1] <- the LUTs at the index whose bits lwe_list_in [nbits][n+1] encrypt at
    q/2, most significant first; big_lut [nout * npoly][N] (reference order)."""
    eng = fourier_bsk.engine
    if pfpksk_list.engine is not eng:
        raise ValueError("the bootstrap key and the pfpksk list live on different engines")
    N = eng.params.polynomial_size
    if big_lut_as_polynomial_list.ndim != 2 or big_lut_as_polynomial_list.shape[1] != N:
        raise ValueError("big_lut must be [polynomial_count][PolynomialSize]")
    if lwe_list_in.ndim != 2 or lwe_list_in.shape[1] != eng.n + 1:
        raise ValueError(f"lwe_list_in needs to have an LWE dimension of {eng.n}")
    if lwe_list_out.ndim != 2 or lwe_list_out.shape[1] != eng.big_dim + 1:
        raise ValueError(f"lwe_list_out needs to have an LWE dimension of {eng.big_dim}")
    nout, npolys = lwe_list_out.shape[0], big_lut_as_polynomial_list.shape[0]
    if nout == 0 or npolys % nout:
        raise ValueError(f"{npolys} LUT polynomials do not divide into {nout} outputs")
    lut = big_lut_as_polynomial_list.reshape(1, nout, npolys // nout, N)
    lwe_list_out[...] = eng.circuit_bootstrap_vertical_packing(lwe_list_in[None], base_log_cbs, level_cbs, lut)[0]


# ---- compressed ciphertext ingress ----------------------------------------------------------------------
def _check_rows(output: np.ndarray, count: int, n: int) -> None:
    if output.size != count * (n + 1) or output.shape[-1] != n + 1:
        raise ValueError(f"Mismatched output list: {output.shape} for {count} ciphertexts of LweSize {n + 1}")


def expand_lwe_compact_ciphertext_list(output_lwe_ciphertext_list: np.ndarray, input_container: np.ndarray,
                                       engine: Engine) -> None:
    """output [count][n+1] <- the compact container [ceil(count / n)][n] masks then [count] bodies; the reference
    asserts the same count and LweSize on both sides."""
    out = output_lwe_ciphertext_list
    n = out.shape[-1] - 1
    count = out.size // (n + 1)
    src = LweSource("compact", n, input_container, count=count)
    out[...] = engine.lwe_expand(src).reshape(out.shape)


par_expand_lwe_compact_ciphertext_list = expand_lwe_compact_ciphertext_list


def decompress_seeded_lwe_ciphertext_list(output_list: np.ndarray, bodies: np.ndarray, compression_seed: int,
                                          engine: Engine) -> None:
    """output [count][n+1] <- a SeededLweCiphertextList (bodies and one CompressionSeed)"""
    b = np.ascontiguousarray(bodies, dtype=np.uint64).ravel()
    _check_rows(output_list, b.size, output_list.shape[-1] - 1)
    src = LweSource("seeded_list", output_list.shape[-1] - 1, b, seeds=int(compression_seed))
    output_list[...] = engine.lwe_expand(src).reshape(output_list.shape)


def decompress_seeded_lwe_ciphertext(output_ct: np.ndarray, body: int, compression_seed: int, engine: Engine) -> None:
    """output [n+1] <- a SeededLweCiphertext (one body word and its CompressionSeed)"""
    _check_rows(output_ct, 1, output_ct.shape[-1] - 1)
    src = LweSource("seeded_rows", output_ct.shape[-1] - 1, np.array([body], dtype=np.uint64), seeds=[int(compression_seed)])
    output_ct[...] = engine.lwe_expand(src).reshape(output_ct.shape)
