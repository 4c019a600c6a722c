"""The fork's gadget layer (tfhe-rs-odd `tfhe/src/gadget`) on the GPU engine.

Arithmetic encodings over Z_p (odd p, or even p for WoP-PBS encodings) and the bootstrapping that
maps one encoding to another, executed as batched keyswitch + PBS launches of the engine:

  Encoding                               gadget/ciphertext/mod.rs:23-270
  Memory::create_accumulator[_wopbs]     gadget/engine/bootstrapping.rs:41-90
  Memory::as_buffers (LUT filling)       gadget/engine/bootstrapping.rs:146-209
  Memory::as_buffers_common_factor       gadget/engine/bootstrapping.rs:214-236
  GadgetEngine::encode_message_into_plaintext / encrypt_arithmetic / decrypt_arithmetic
                                         gadget/engine/mod.rs:101-191
  GadgetEngine::exec_gadget_with_extraction, apply_lut
                                         gadget/engine/mod.rs:263-322
  Bootstrapper::keyswitch_bootstrap      gadget/engine/bootstrapping.rs:828-884
  bootstrap_without_sample_extract       fft64/crypto/bootstrap.rs:383-412 (Engine.blind_rotate)
  GadgetEngine::lwe_mult, woppbs_lut     gadget/engine/mod.rs:677-803 (Engine.lwe_mult: packing
                                         keyswitch + glwe_mult, custom_glwe_glwe_product.rs:13-321)

The fork's msgpack noise dumps ("cjp" patterns) are not reproduced.  Batched forms take many
independent gadget evaluations and issue one GPU launch for all of them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import client
from .engine import Engine
from .parameters import ClassicPBSParameters


class Encoding:
    """Encoding of Z_o into Z_p: parts[i] = the Z_p elements encoding i (gadget/ciphertext/mod.rs)."""

    def __init__(self, origin_modulus: int, parts, modulus_p: int, wopbs: bool = False, check: bool = True):
        self.origin_modulus = origin_modulus
        self.parts = [frozenset(int(x) for x in part) for part in parts]
        self.modulus_p = modulus_p
        self.wopbs = wopbs
        assert all(x < modulus_p for part in self.parts for x in part)
        if check and not self.is_valid():
            raise ValueError("This Arithmetic Encoding is not correct !")

    # -- constructors (ciphertext/mod.rs:157-215) ----------------------------------------------
    @classmethod
    def new_canonical(cls, origin_modulus: int, values_for_singletons, modulus_p: int) -> "Encoding":
        return cls(origin_modulus, [[v] for v in values_for_singletons], modulus_p)

    @classmethod
    def new_canonical_binary(cls, value_for_singleton_true: int, modulus_p: int) -> "Encoding":
        return cls.new_canonical(2, [0, value_for_singleton_true], modulus_p)

    @classmethod
    def parity_encoding(cls) -> "Encoding":
        return cls.new_canonical_binary(1, 2)

    @classmethod
    def new_trivial(cls, origin_modulus: int) -> "Encoding":
        return cls.new_canonical(origin_modulus, range(origin_modulus), origin_modulus)

    @classmethod
    def new_trivial_wopbs(cls, modulus: int) -> "Encoding":
        return cls(modulus, [[i] for i in range(modulus)], modulus, wopbs=True, check=False)

    @classmethod
    def new_all_one_wopbs(cls, modulus: int) -> "Encoding":
        return cls(modulus, [[1]] * modulus, modulus, wopbs=True, check=False)

    # -- predicates / accessors -------------------------------------------------------------------
    def is_valid(self) -> bool:
        """ciphertext/mod.rs:44-86 (the disjointness check is disabled in the reference too)."""
        assert self.origin_modulus == len(self.parts)
        p = self.modulus_p
        if p % 2 == 1 or p == 2 or self.wopbs:
            return True
        # negacyclicity: the opposite (x + p/2) of an element of part i may only lie in part [-i]_o
        for i in range(self.origin_modulus):
            neg_i = self.negative_on_o_ring(i)
            forbidden = set()
            for j, part in enumerate(self.parts):
                if j != neg_i:
                    forbidden |= part
            for x in self.parts[i]:
                if (x + p // 2) % p in forbidden:
                    return False
        return True

    def get_origin_modulus(self) -> int:
        return self.origin_modulus

    def get_modulus(self) -> int:
        return self.modulus_p

    def get_part(self, i: int) -> frozenset:
        return self.parts[i]

    def is_partition_containing(self, element_of_zo: int, value: int) -> bool:
        return value in self.parts[element_of_zo]

    def inverse_encoding(self, x: int):
        for i in range(self.origin_modulus):
            if x in self.parts[i]:
                return i
        return None

    def is_canonical(self) -> bool:
        return all(len(part) == 1 for part in self.parts)

    def get_part_single_value_if_canonical(self, i: int) -> int:
        assert self.is_canonical()
        return next(iter(self.parts[i]))

    def negative_on_p_ring(self, x: int) -> int:
        return (self.modulus_p - x) % self.modulus_p

    def negative_on_o_ring(self, i: int) -> int:
        return (self.origin_modulus - i) % self.origin_modulus

    # -- transformations -----------------------------------------------------------------------
    def add_constant(self, constant: int) -> "Encoding":
        p = self.modulus_p
        return Encoding(self.origin_modulus, [[(x + constant) % p for x in part] for part in self.parts], p)

    def multiply_encoding_by_constant(self, constant: int) -> "Encoding":
        p = self.modulus_p
        return Encoding(self.origin_modulus, [[x * constant % p for x in part] for part in self.parts], p)

    def apply_lut_to_encoding(self, f) -> "Encoding":
        """ciphertext/mod.rs:217-247: part j of the result = union of the parts i with f(i) = j."""
        parts = [set() for _ in range(self.origin_modulus)]
        for i in range(self.origin_modulus):
            j = f(i)
            if 0 <= j < self.origin_modulus:
                parts[j] |= self.parts[i]
        return Encoding(self.origin_modulus, parts, self.modulus_p, wopbs=self.wopbs, check=not self.wopbs)

    def __eq__(self, other) -> bool:
        return (isinstance(other, Encoding) and self.origin_modulus == other.origin_modulus
                and self.modulus_p == other.modulus_p and self.parts == other.parts)

    def __repr__(self) -> str:
        return f"Encoding(o={self.origin_modulus}, p={self.modulus_p}, parts={[sorted(p) for p in self.parts]})"


# ---- accumulators (gadget/engine/bootstrapping.rs) --------------------------------------------
def create_accumulator(enc_in: Encoding, enc_out: Encoding) -> list:
    """Memory::create_accumulator (:41-70), odd p: entry k of Z_p."""
    assert enc_in.is_valid() and enc_out.is_canonical()
    p = enc_in.get_modulus()
    assert p % 2 == 1
    accu = [0] * p
    for k in range(p):
        if k % 2 == 0:
            i = enc_in.inverse_encoding(k // 2)
            accu[k] = enc_out.get_part_single_value_if_canonical(i) if i is not None else 0
        else:
            i = enc_in.inverse_encoding((p + 1) // 2 + (k - 1) // 2)
            accu[k] = (enc_out.negative_on_p_ring(enc_out.get_part_single_value_if_canonical(i))
                       if i is not None else 0)
    return accu


def create_accumulator_wopbs(enc_in: Encoding, enc_out: Encoding) -> list:
    """Memory::create_accumulator_wopbs (:74-90), even p != 2."""
    assert enc_in.is_valid() and enc_out.is_canonical()
    p = enc_in.get_modulus()
    assert p % 2 == 0 and p != 2
    accu = [0] * p
    for k in range(p):
        i = enc_in.inverse_encoding(k)
        accu[k] = enc_out.get_part_single_value_if_canonical(i) if i is not None else 0
    return accu


def fill_lookup_table(params: ClassicPBSParameters, enc_in: Encoding, enc_out: Encoding) -> np.ndarray:
    """Memory::as_buffers (:146-209): GLWE accumulator (mask 0) whose body holds the p windows of
    the encoding map, window k = [N/(2p) + (k-1)N/p, N/(2p) + kN/p) (integer divisions as the
    reference's left-to-right usize arithmetic), the first window split in two negacyclic halves.
    Entries the reference leaves untouched when p does not divide N (they keep whatever its
    reused buffer held) are zero here."""
    k, N = params.glwe_dimension, params.polynomial_size
    acc = np.zeros((k + 1) * N, dtype=np.uint64)
    body = acc[k * N:]
    p = enc_in.get_modulus()
    new_p = enc_out.get_modulus()
    unit = (1 << 64) // new_p
    if p != 2:
        data = create_accumulator(enc_in, enc_out) if p % 2 == 1 else create_accumulator_wopbs(enc_in, enc_out)
        half = N // (2 * p)
        body[:half] = np.uint64(unit * data[0])
        for kk in range(1, len(data)):
            body[half + (kk - 1) * N // p: half + kk * N // p] = np.uint64(unit * data[kk])
        body[N - half:] = np.uint64(unit * ((new_p - data[0]) % new_p))
    else:
        new_false = enc_out.get_part_single_value_if_canonical(0)
        new_true = enc_out.get_part_single_value_if_canonical(1)
        assert new_false == (new_p - new_true) % new_p
        new_0, new_1 = (new_true, new_false) if enc_in.is_partition_containing(1, 0) else (new_false, new_true)
        body[:N // 2] = np.uint64(unit * new_0)
        body[N // 2:] = np.uint64(unit * new_1)
    return acc


def fill_common_factor_lookup_table(params: ClassicPBSParameters, enc_out: Encoding) -> np.ndarray:
    """Memory::as_buffers_common_factor (:214-236): constant body 2^64/p (2^63/p for even p)."""
    k, N = params.glwe_dimension, params.polynomial_size
    acc = np.zeros((k + 1) * N, dtype=np.uint64)
    constant = (1 << 63) if enc_out.get_modulus() % 2 == 0 else (1 << 64)
    acc[k * N:] = np.uint64(constant // enc_out.get_modulus())
    return acc


def create_vi_for_mvb(N: int, enc_inter: Encoding, enc_out: Encoding) -> np.ndarray:
    """Bootstrapper::create_vi_for_mvb (:503-541): the sparse plaintext polynomial v_i whose
    product with the common-factor rotation v0 realises the LUT: coefficient N/(2p) + iN/p holds
    the window-to-window difference of the (halved, for odd p_out) accumulator values."""
    data = create_accumulator(enc_inter, enc_out)
    p = enc_inter.get_modulus()
    new_p = enc_out.get_modulus()
    if new_p % 2 == 1:
        inv2 = (new_p + 1) // 2
        data = [x * inv2 % new_p for x in data]
    elif new_p == 2:
        new_p = 4
    v = np.zeros(N, dtype=np.uint64)
    for i in range(p - 1):
        v[N // (2 * p) + i * N // p] = (data[i + 1] - data[i]) % new_p
    v[N // (2 * p) + (p - 1) * N // p] = (new_p - data[0] - data[p - 1]) % new_p
    return v


def pack_window_polys(N: int, p: int) -> np.ndarray:
    """The window sums of Bootstrapper::pack_into_new_accumulator (:690-773) as plaintext
    polynomials: element k of the accumulator is shifted to X^(s/2 + (k-1)s + i), i < s
    (s = N/p; k = 0 covers X^0..X^(s/2-1)), and element 0, negated, to X^(N - s/2 + i)."""
    assert p % 2 == 1
    s = N // p
    minus_one = np.uint64((1 << 64) - 1)
    w = np.zeros((p, N), dtype=np.uint64)
    w[0, :s // 2] = 1
    for k in range(1, p):
        off = s // 2 + (k - 1) * s
        w[k, off:off + s] += np.uint64(1)
    w[0, N - s // 2:] += minus_one
    return w


# ---- ciphertexts and keys --------------------------------------------------------------------
@dataclass
class Ciphertext:
    """Ciphertext::EncodingEncrypted (gadget/ciphertext/mod.rs:14-17): an LWE under the big key
    (KS -> PBS order) or the small key (PBS -> KS order) and its encoding."""

    ct: np.ndarray
    encoding: Encoding

    def clone(self) -> "Ciphertext":
        return Ciphertext(self.ct.copy(), self.encoding)


def _round_half_away(x: float) -> int:
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


class ClientKey:
    """gadget ClientKey (gadget/client_key/mod.rs:29-142) with the engine's seeded client keygen."""

    def __init__(self, params: ClassicPBSParameters, seed: int = 0):
        self.parameters = params
        self.seed = seed
        self.lwe_secret_key = client.gen_binary_key(seed, 1, params.lwe_dimension)
        self.glwe_secret_key = client.gen_binary_key(seed, 2, params.glwe_dimension * params.polynomial_size)
        self._counter = 0

    def _key_and_noise(self):
        p = self.parameters
        if p.encryption_key_choice == "Big":
            return self.glwe_secret_key, p.glwe_modular_std_dev
        return self.lwe_secret_key, p.lwe_modular_std_dev

    @staticmethod
    def encode_message_into_plaintext(message: int, encoding: Encoding) -> int:
        """engine/mod.rs:126-134: (2^64 / p) * zp."""
        return ((1 << 64) // encoding.get_modulus() * encoding.get_part_single_value_if_canonical(message)) % (1 << 64)

    def encrypt_arithmetic_many(self, messages, encoding: Encoding) -> list:
        """encrypt_arithmetic (engine/mod.rs:136-150) for a list of messages."""
        assert encoding.is_canonical()
        assert all(0 <= m < encoding.get_origin_modulus() for m in messages)
        pts = np.array([self.encode_message_into_plaintext(m, encoding) for m in messages], dtype=np.uint64)
        key, std = self._key_and_noise()
        self._counter += 1
        cts = client.lwe_encrypt((self.seed << 24) + 0x9A0000 + self._counter, key, pts, std)
        return [Ciphertext(cts[i].copy(), encoding) for i in range(len(messages))]

    def encrypt_arithmetic(self, message: int, encoding: Encoding) -> Ciphertext:
        return self.encrypt_arithmetic_many([message], encoding)[0]

    def _phases(self, cts) -> np.ndarray:
        key, _ = self._key_and_noise()
        return client.lwe_decrypt(key, np.stack([c.ct for c in cts]))

    def decrypt_many(self, cts) -> list:
        """decrypt_arithmetic (engine/mod.rs:165-191): round(phase * p / 2^64) mod p, then the part."""
        out = []
        for phase, c in zip(self._phases(cts), cts):
            p = c.encoding.get_modulus()
            x = float(np.uint64(phase)) * (p / float(1 << 64))
            closest = int(math.floor(x + 0.5)) % p   # f64::round (x >= 0)
            i = c.encoding.inverse_encoding(closest)
            if i is None:
                raise ValueError(f"No value in Zo has been found for : {x}.")
            out.append(i)
        return out

    def decrypt(self, ct: Ciphertext) -> int:
        return self.decrypt_many([ct])[0]

    def measure_noise(self, ct: Ciphertext) -> int:
        """measure_noise (engine/mod.rs:193-231): distance to the closest Z_p point, scaled to 2^64."""
        phase = int(self._phases([ct])[0])
        p = ct.encoding.get_modulus()
        x = float(phase) * (p / float(1 << 64))
        closest = int(math.floor(x + 0.5)) % p
        noise = closest - x
        if abs(noise) > p / 2.0:
            noise = p - abs(noise)
        return _round_half_away(noise * float(1 << 64))


class ServerKey:
    """gadget ServerKey (engine/bootstrapping.rs:261-345; server_key/mod.rs) on the engine.

    Holds the bootstrapping key (Fourier, in HBM), the LWE keyswitching key and -- created on
    first use by mvb/tree bootstrapping and by lwe_mult -- the LWE -> GLWE packing keyswitching key
    and the GLWE relinearisation key of the "even transistor" (lwe_mult, woppbs_lut).
    Every method has a *_batch form that evaluates many independent inputs in one launch per
    step; the single forms mirror the reference's signatures."""

    def __init__(self, client_key: ClientKey, device: int = 0, engine=None):
        p = self.parameters = client_key.parameters
        self.engine = engine if engine is not None else Engine(p, device)
        self._ck_seed = client_key.seed
        self._big_key = client_key.glwe_secret_key
        self._glwe_key = client_key.glwe_secret_key
        ck = client_key
        bsk = client.gen_bootstrap_key(ck.seed * 7 + 3, ck.lwe_secret_key, ck.glwe_secret_key, p.glwe_dimension,
                                       p.polynomial_size, p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev)
        ksk = client.gen_keyswitch_key(ck.seed * 7 + 4, ck.glwe_secret_key, ck.lwe_secret_key, p.ks_base_log,
                                       p.ks_level, p.lwe_modular_std_dev)
        self.engine.upload_bootstrap_key(bsk)
        self.engine.upload_keyswitch_key(ksk)
        self.pbs_order = "KeyswitchBootstrap" if p.encryption_key_choice == "Big" else "BootstrapKeyswitch"
        self._pksk_ready = False
        self._rlk_ready = False

    # -- key material ----------------------------------------------------------------------
    def _require_packing_key(self):
        """allocate_and_generate_new_lwe_packing_keyswitch_key (bootstrapping.rs:331-339): big
        LWE key -> GLWE key, with the KS decomposition and the GLWE noise."""
        if self._pksk_ready:
            return
        p = self.parameters
        pksk = client.gen_packing_keyswitch_key(self._ck_seed * 7 + 5, self._big_key, self._glwe_key,
                                                p.glwe_dimension, p.polynomial_size, p.ks_base_log, p.ks_level,
                                                p.glwe_modular_std_dev)
        self.engine.upload_packing_keyswitch_key(pksk, p.ks_base_log, p.ks_level)
        self._pksk_ready = True

    def _require_relinearization_key(self):
        """allocate_and_generate_new_relinearization_key (bootstrapping.rs:367-374): products of the
        GLWE key's polynomials under the GLWE key, with the KS decomposition and the GLWE noise."""
        if self._rlk_ready:
            return
        p = self.parameters
        rlk = client.gen_relinearization_key(self._ck_seed * 7 + 6, self._glwe_key, p.glwe_dimension,
                                             p.polynomial_size, p.ks_base_log, p.ks_level, p.glwe_modular_std_dev)
        self.engine.upload_relinearization_key(rlk, p.ks_base_log, p.ks_level)
        self._rlk_ready = True

    @property
    def _lwe_size(self) -> int:
        p = self.parameters
        return p.big_lwe_dimension + 1 if self.pbs_order == "KeyswitchBootstrap" else p.lwe_dimension + 1

    def keyswitch(self, x: np.ndarray) -> np.ndarray:
        """ServerKey::keyswitch (bootstrapping.rs:902-914), batched."""
        return self.engine.keyswitch(x)

    def _bootstrap_pattern(self, x: np.ndarray, luts: np.ndarray, lut_indexes=None) -> np.ndarray:
        """apply_bootstrapping_pattern (:887-898): keyswitch_bootstrap (:828-884) or
        bootstrap_keyswitch (:776-825), batched over rows of x."""
        if self.pbs_order == "KeyswitchBootstrap":
            return self.engine.keyswitch_programmable_bootstrap(x, luts, lut_indexes)
        return self.engine.programmable_bootstrap_keyswitch(x, luts, lut_indexes)

    # -- gadget evaluation (BPR24) ---------------------------------------------------------
    def exec_gadget_with_extraction_batch(self, enc_inter: Encoding, enc_out: Encoding, inputs) -> list:
        """exec_gadget_with_extraction (engine/mod.rs:263-302) for many independent input lists at
        once: each list is summed (lwe_ciphertext_add_assign), then ONE keyswitch + PBS launch with
        the encoding accumulator."""
        x = np.stack([np.sum(np.stack([c.ct for c in lst]), axis=0, dtype=np.uint64) for lst in inputs])
        lut = fill_lookup_table(self.parameters, enc_inter, enc_out)
        out = self._bootstrap_pattern(x, lut)
        return [Ciphertext(out[i].copy(), enc_out) for i in range(len(inputs))]

    def exec_gadget_with_extraction(self, enc_in, enc_inter: Encoding, enc_out: Encoding, inputs) -> Ciphertext:
        return self.exec_gadget_with_extraction_batch(enc_inter, enc_out, [inputs])[0]

    # -- arithmetic LUTs -------------------------------------------------------------------
    def apply_lut_batch(self, inputs, encoding_out: Encoding, f) -> list:
        """apply_lut (engine/mod.rs:303-322) over inputs sharing one encoding: intermediate
        encoding = the input encoding pushed through f, one KS + PBS launch."""
        enc_in = inputs[0].encoding
        assert all(c.encoding == enc_in for c in inputs)
        enc_inter = enc_in.apply_lut_to_encoding(f)
        x = np.stack([c.ct for c in inputs])
        out = self._bootstrap_pattern(x, fill_lookup_table(self.parameters, enc_inter, encoding_out))
        return [Ciphertext(out[i].copy(), encoding_out) for i in range(len(inputs))]

    def apply_lut(self, ct: Ciphertext, encoding_out: Encoding, f) -> Ciphertext:
        return self.apply_lut_batch([ct], encoding_out, f)[0]

    def encoding_switching_lut(self, ct: Ciphertext, encoding_out: Encoding) -> Ciphertext:
        """server_key/mod.rs:97-99: apply_lut with the identity."""
        return self.apply_lut(ct, encoding_out, lambda x: x)

    # -- linear operations (engine/mod.rs:519-662) -------------------------------------------
    def encoding_switching_mul_constant(self, ct: Ciphertext, coefficient: int) -> Ciphertext:
        out = (ct.ct * np.uint64(coefficient % (1 << 64))).astype(np.uint64)
        return Ciphertext(out, ct.encoding.multiply_encoding_by_constant(coefficient))

    def simple_sum(self, inputs) -> Ciphertext:
        """Warning (as the reference): no encoding check; the result keeps inputs[0]'s encoding."""
        return Ciphertext(np.sum(np.stack([c.ct for c in inputs]), axis=0, dtype=np.uint64), inputs[0].encoding)

    @staticmethod
    def _plaintext(constant: int, modulus: int) -> np.uint64:
        return np.uint64(((1 << 64) // modulus * constant) % (1 << 64))

    def simple_plaintext_sum(self, ct: Ciphertext, constant: int, modulus: int) -> Ciphertext:
        out = ct.ct.copy()
        out[-1] += self._plaintext(constant, modulus)
        return Ciphertext(out, ct.encoding)

    def simple_mul_constant(self, ct: Ciphertext, constant: int, modulus: int) -> Ciphertext:
        return Ciphertext((ct.ct * np.uint64(constant % modulus)).astype(np.uint64), ct.encoding)

    def encoding_switching_sum_constant(self, ct: Ciphertext, constant: int, modulus: int) -> Ciphertext:
        out = ct.ct.copy()
        out[-1] += self._plaintext(constant, modulus)
        return Ciphertext(out, ct.encoding.add_constant(constant))

    def linear_combination(self, inputs, coefficients, modulus: int) -> Ciphertext:
        """server_key/mod.rs:128-137."""
        return self.simple_sum([self.simple_mul_constant(c, k, modulus) for c, k in zip(inputs, coefficients)])

    # -- multi-value bootstrapping (bootstrapping.rs:441-620) ---------------------------------
    def _mvb_polys(self, enc_in: Encoding, encodings_out, lut_fis) -> np.ndarray:
        N = self.parameters.polynomial_size
        return np.stack([create_vi_for_mvb(N, enc_in.apply_lut_to_encoding(lambda x, lut=lut: lut[x]), enc_out)
                         for enc_out, lut in zip(encodings_out, lut_fis)])

    def _common_factor(self, x_small: np.ndarray, enc_out: Encoding) -> np.ndarray:
        """bootstrap_common_factor (:441-500): blind rotation of the constant accumulator."""
        return self.engine.blind_rotate(x_small, fill_common_factor_lookup_table(self.parameters, enc_out))

    def mvb_batch(self, inputs, encodings_out, fis) -> list:
        """ServerKey::mvb (server_key/mod.rs:38-51; engine/mod.rs:324-372), KS -> PBS order, for
        inputs sharing one encoding: KS, one blind rotation per input (common factor for
        encodings_out[0]), then one product-and-extract launch for all (input, v_i) pairs."""
        assert len(encodings_out) == len(fis)
        if self.pbs_order != "KeyswitchBootstrap":
            raise NotImplementedError("mvb: BootstrapKeyswitch order")
        enc_in = inputs[0].encoding
        assert all(c.encoding == enc_in for c in inputs)
        lut_fis = [[int(f(x)) for x in range(enc_in.get_origin_modulus())] for f in fis]
        vis = self._mvb_polys(enc_in, encodings_out, lut_fis)
        v0 = self._common_factor(self.keyswitch(np.stack([c.ct for c in inputs])), encodings_out[0])
        out = self.engine.glwe_poly_mul(v0, vis, extract=True)  # [count][len(fis)][kN+1]
        return [[Ciphertext(out[c, i].copy(), e) for i, e in enumerate(encodings_out)] for c in range(len(inputs))]

    def mvb(self, ct: Ciphertext, encodings_out, fis) -> list:
        return self.mvb_batch([ct], encodings_out, fis)[0]

    # -- tree bootstrapping (server_key/mod.rs:53-94; engine/mod.rs:400-510) ------------------
    def pack_into_new_accumulator(self, lwes: np.ndarray, p: int) -> np.ndarray:
        """Bootstrapper::pack_into_new_accumulator (:690-773): accumulator element k = lwes[k/2]
        (k even) or -lwes[(p+1)/2 + (k-1)/2] (k odd; zero when absent), each packed to a GLWE by
        the packing keyswitch and summed over its Z_p window.  lwes: [count][m][kN+1]."""
        assert p % 2 == 1, "Pas sûr que ça marche avec une output paire"
        self._require_packing_key()
        count, m, width = lwes.shape
        elems = np.zeros((count, p, width), dtype=np.uint64)
        for k in range(p):
            src = k // 2 if k % 2 == 0 else (p + 1) // 2 + (k - 1) // 2
            if src < m:
                elems[:, k] = lwes[:, src] if k % 2 == 0 else (np.uint64(0) - lwes[:, src])
        packed = self.engine.packing_keyswitch(elems.reshape(count * p, width))
        packed = packed.reshape(count, p, -1)
        windows = pack_window_polys(self.parameters.polynomial_size, p)[None]   # [1][p][N]
        return self.engine.glwe_poly_mul(packed, windows, extract=False)[:, 0]  # [count][(k+1)N]

    def full_tree_bootstrapping_batch(self, inputs_list, encodings_out, t: int, f) -> list:
        """full_tree_bootstrapping (server_key/mod.rs:53-94) for many independent input pairs
        (depth-2 trees, KS -> PBS order): common factor of inputs[1], two MVB + packing rounds
        (lut_f0 = f mod o, lut_f1 = f div o), then a PBS of inputs[0] on each packed accumulator.
        Returns [r1, r0] per input pair."""
        if self.pbs_order != "KeyswitchBootstrap":
            raise NotImplementedError("tree bootstrapping: BootstrapKeyswitch order (the reference panics)")
        origin = [c.encoding.get_origin_modulus() for c in inputs_list[0]]
        assert math.prod(origin) == t
        o = origin[0]
        lut_f0 = [f(x) % o for x in range(t)]
        lut_f1 = [(f(x) - f(x) % o) // o for x in range(t)]
        count = len(inputs_list)
        c1 = np.stack([ins[1].ct for ins in inputs_list])
        c0 = np.stack([ins[0].ct for ins in inputs_list])
        common = self._common_factor(self.keyswitch(c1), encodings_out[0])          # [count][(k+1)N]
        enc_in_0 = inputs_list[0][1].encoding
        o0 = enc_in_0.get_origin_modulus()
        c0_small = self.keyswitch(c0)
        results = []
        for lut_fi, enc_out in ((lut_f0, encodings_out[0]), (lut_f1, encodings_out[1])):
            first = [[lut_fi[x + j * o0] for x in range(o0)] for j in range(t // o0)]
            vis = self._mvb_polys(enc_in_0, [enc_out] * (t // o0), first)
            lwes = self.engine.glwe_poly_mul(common, vis, extract=True)            # [count][t/o0][kN+1]
            accs = self.pack_into_new_accumulator(lwes, enc_in_0.get_modulus())    # [count][(k+1)N]
            out = self.engine.programmable_bootstrap(c0_small, accs, np.arange(count, dtype=np.uint32))
            results.append([Ciphertext(out[c].copy(), enc_out) for c in range(count)])
        r0, r1 = results
        return [[r1[c], r0[c]] for c in range(count)]

    def full_tree_bootstrapping(self, inputs, encodings_out, t: int, f) -> list:
        return self.full_tree_bootstrapping_batch([inputs], encodings_out, t, f)[0]

    # -- the even transistor (engine/mod.rs:677-803) -------------------------------------------
    def lwe_mult_batch(self, lhs, rhs, output_encoding: Encoding) -> list:
        """lwe_mult (engine/mod.rs:680-751) for many independent pairs: both LWEs packed to GLWEs by the
        packing keyswitch, multiplied with relinearisation (glwe_mult, log_p = ilog2 of the common
        modulus, which must be even) and sample-extracted, in ONE engine call.  The inputs' encodings
        only have to share their modulus; the result takes output_encoding."""
        assert len(lhs) == len(rhs)
        if not all(isinstance(c, Ciphertext) for c in list(lhs) + list(rhs)):
            raise ValueError("Calling LweMult with trivial ciphertexts")
        if self.pbs_order != "KeyswitchBootstrap":
            raise NotImplementedError("lwe_mult: BootstrapKeyswitch order (the inputs must be under the big key)")
        p = lhs[0].encoding.get_modulus()
        assert all(c.encoding.get_modulus() == p for c in list(lhs) + list(rhs)), "lwe_mult: unequal moduli"
        log_p = p.bit_length() - 1
        assert log_p % 2 == 0, f"lwe_mult: log2(p) = {log_p} is odd"
        self._require_packing_key()
        self._require_relinearization_key()
        out = self.engine.lwe_mult(np.stack([c.ct for c in lhs]), np.stack([c.ct for c in rhs]), log_p)
        return [Ciphertext(out[i].copy(), output_encoding) for i in range(len(lhs))]

    def lwe_mult(self, lhs: Ciphertext, rhs: Ciphertext, output_encoding: Encoding) -> Ciphertext:
        return self.lwe_mult_batch([lhs], [rhs], output_encoding)[0]

    def woppbs_lut_batch(self, inputs, encoding_out: Encoding, f) -> list:
        """woppbs_lut (engine/mod.rs:755-802) over inputs sharing one (WoP-PBS, even p) encoding: two
        bootstrapping launches over the batch -- ct_f with the input encoding pushed through f, ct_ones
        onto Encoding.new_all_one_wopbs, whose negacyclic sign cancels ct_f's -- then one lwe_mult.
        As in the reference, the wopbs accumulator spreads its p windows over half the torus, so an
        input encoded at x * 2^64/p reads window 2x mod p: on Encoding.new_trivial_wopbs(p) inputs the
        chain returns f(2x mod p), not f(x)."""
        if not all(isinstance(c, Ciphertext) for c in inputs):
            raise ValueError("woppbs_lut on a trivial ciphertext")
        enc_in = inputs[0].encoding
        assert all(c.encoding == enc_in for c in inputs)
        enc_inter = enc_in.apply_lut_to_encoding(f)
        enc_ones = Encoding.new_all_one_wopbs(enc_in.get_origin_modulus())
        x = np.stack([c.ct for c in inputs])
        ct_f = self._bootstrap_pattern(x, fill_lookup_table(self.parameters, enc_inter, encoding_out))
        ct_ones = self._bootstrap_pattern(x, fill_lookup_table(self.parameters, enc_in, enc_ones))
        return self.lwe_mult_batch([Ciphertext(ct_f[i], encoding_out) for i in range(len(inputs))],
                                   [Ciphertext(ct_ones[i], enc_ones) for i in range(len(inputs))], encoding_out)

    def woppbs_lut(self, ct: Ciphertext, encoding_out: Encoding, f) -> Ciphertext:
        return self.woppbs_lut_batch([ct], encoding_out, f)[0]

    def trivial_encrypt(self, message: int) -> int:
        """Ciphertext::Trivial (engine/mod.rs:97-99) is a bare integer in the reference."""
        return message


# ---- Gadget (gadget/gadget/mod.rs) -------------------------------------------------------
def split_int_in_booleans(x: int, expected_length: int, big_endian: bool) -> list:
    res = [(x >> i) & 1 for i in range(max(expected_length, x.bit_length()))]
    assert len(res) == expected_length, "value does not fit"
    return res[::-1] if big_endian else res


def vec_bool_to_int(x, big_endian: bool) -> int:
    bits = list(x)[::-1] if big_endian else list(x)
    return sum(1 << i for i, b in enumerate(bits) if b == 1)


class Gadget:
    """Gadget (gadget/gadget/mod.rs:6-176): a Boolean function evaluated with one bootstrapping
    on a sum of canonically encoded inputs (BPR24)."""

    def __init__(self, encodings_in, encoding_inter: Encoding, encoding_out: Encoding, size_input: int, true_fn):
        assert all(e.is_canonical() for e in encodings_in)
        assert encoding_out.is_canonical()
        self.encodings_in = list(encodings_in)
        self.encoding_inter = encoding_inter
        self.encoding_out = encoding_out
        self.size_input = size_input
        self.true_result = [true_fn(split_int_in_booleans(x, size_input, False)) for x in range(1 << size_input)]

    @classmethod
    def new_canonical(cls, qis, q_out: int, p_in: int, p_out: int, size_input: int, true_fn) -> "Gadget":
        encodings_in = [Encoding.new_canonical_binary(q, p_in) for q in qis]
        inter = cls.compute_sum_encodings_from_canonical_binary(qis, p_in, size_input, true_fn)
        return cls(encodings_in, inter, Encoding.new_canonical_binary(q_out, p_out), size_input, true_fn)

    @staticmethod
    def compute_sum_encodings_from_canonical_binary(qis, p: int, size_input: int, true_fn) -> Encoding:
        part_false, part_true = set(), set()
        for i in range(1 << size_input):
            bits = split_int_in_booleans(i, size_input, True)
            result = sum(q for b, q in zip(bits, qis) if b == 1) % p
            if true_fn(bits) == 1:
                assert result not in part_false
                part_true.add(result)
            else:
                assert result not in part_true
                part_false.add(result)
        return Encoding(2, [part_false, part_true], p)

    def get_encoding_in(self, index: int) -> Encoding:
        return self.encodings_in[index]

    def get_encoding_out(self) -> Encoding:
        return self.encoding_out

    def get_modulus_in(self) -> int:
        return self.encodings_in[0].get_modulus()

    def get_modulus_out(self) -> int:
        return self.encoding_out.get_modulus()

    def exec_clear(self, bits) -> int:
        return self.true_result[vec_bool_to_int(bits, False)]

    def exec_batch(self, inputs_list, server_key: ServerKey) -> list:
        for inputs in inputs_list:
            for c, e in zip(inputs, self.encodings_in):
                assert c.encoding == e
        return server_key.exec_gadget_with_extraction_batch(self.encoding_inter, self.encoding_out, inputs_list)

    def exec(self, inputs, server_key: ServerKey) -> Ciphertext:
        return self.exec_batch([inputs], server_key)[0]

    def test_full(self, client_key: ClientKey, server_key: ServerKey) -> None:
        """All 2^size_input inputs in one batch, checked against the truth table."""
        xs = list(range(1 << self.size_input))
        bits = [split_int_in_booleans(x, self.size_input, False) for x in xs]
        cts = [[client_key.encrypt_arithmetic(b, self.encodings_in[i]) for i, b in enumerate(bb)] for bb in bits]
        res = client_key.decrypt_many(self.exec_batch(cts, server_key))
        for bb, r in zip(bits, res):
            assert r == self.true_result[vec_bool_to_int(bb, False)], (bb, r)

    def cast_before_gadget(self, coefficients, inputs, server_key: ServerKey) -> list:
        return [server_key.encoding_switching_mul_constant(x, c) for x, c in zip(inputs, coefficients) if c != 0]

    def cast_before_gadget_from_1(self, inputs, server_key: ServerKey) -> list:
        coefficients = [e.get_part_single_value_if_canonical(1) for e in self.encodings_in]
        return self.cast_before_gadget(coefficients, inputs, server_key)

    def modulus_switching(self, inputs, p_in_vec, p_out: int, server_key: ServerKey) -> list:
        assert len(inputs) == len(p_in_vec)
        out = []
        for x, p_i in zip(inputs, p_in_vec):
            if p_i != p_out:
                g = Gadget.new_canonical([1], 1, p_i, p_out, 1, lambda b: b[0])
                out.append(g.exec([x], server_key))
            else:
                out.append(x.clone())
        return out
