"""Mirror of the reference shortint API on the PBS path (tfhe/src/shortint), backed by the engine.

  ClientKey.encrypt / decrypt_message_and_carry / decrypt   engine/client_side.rs:58-140,
                                                            client_key/mod.rs:281-330
  ServerKey.generate_lookup_table / generate_msg_lookup_table
                                                            server_key/mod.rs:383-432
  ServerKey.apply_lookup_table[_assign]                     server_key/mod.rs:457-476
  ServerKey.keyswitch_programmable_bootstrap_assign         server_key/mod.rs:783-857
  ServerKey.programmable_bootstrap_keyswitch_assign         server_key/mod.rs:859-932
  ServerKey.trivial_pbs_assign                              server_key/mod.rs:763-781
  gen_keys                                                  shortint/mod.rs (gen_keys)
  ClientKey.encrypt_without_padding / decrypt_without_padding
                                                            engine/client_side.rs:273-317, client_key/mod.rs:424-483
  WopbsKey.new_wopbs_key_only_for_wopbs / generate_lut[_without_padding] / wopbs /
  programmable_bootstrapping_without_padding                wopbs/mod.rs:235-495, 825-857
  WopbsKey.new_wopbs_key                                    engine/wopbs/mod.rs:50-183
  WopbsKey.keyswitch_to_wopbs_params / keyswitch_to_pbs_params / programmable_bootstrapping /
  extract_bits / circuit_bootstrapping_vertical_packing     wopbs/mod.rs:398-408, 547-754

  CompactPublicKey.encrypt_many                             public_key/compact.rs (CompactPublicKey::encrypt_slice)
  CompactCiphertextList.expand                              ciphertext/mod.rs:544-584
  CompressedCiphertext.decompress                           ciphertext/mod.rs:493-513
  ClientKey.encrypt_compressed_many                         engine/client_side.rs (encrypt_compressed)

Batched forms (`apply_lookup_table_batch`) hand a whole layer of independent ciphertexts to the
GPU in one launch -- the shape the integer layer produces (radix_parallel/mul.rs:347-407).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from . import client
from .engine import Engine, LweSource, fill_accumulator
from .parameters import ClassicPBSParameters, WopbsParameters

NOISE_ZERO = 0
NOISE_NOMINAL = 1
KEYSWITCH_BOOTSTRAP = "KeyswitchBootstrap"
BOOTSTRAP_KEYSWITCH = "BootstrapKeyswitch"


@dataclass
class Ciphertext:
    """shortint Ciphertext (shortint/ciphertext/mod.rs:263-270)."""

    ct: np.ndarray
    degree: int
    noise_level: int
    message_modulus: int
    carry_modulus: int
    pbs_order: str

    def is_trivial(self) -> bool:
        return self.noise_level == NOISE_ZERO and not np.any(self.ct[:-1])

    def clone(self) -> "Ciphertext":
        return copy.deepcopy(self)


@dataclass
class LookupTable:
    """LookupTableOwned { acc: GlweCiphertext, degree } (server_key/mod.rs)."""

    acc: np.ndarray
    degree: int


@dataclass
class ClientKey:
    parameters: ClassicPBSParameters
    seed: int = 0
    small_lwe_secret_key: np.ndarray = field(init=False)
    glwe_secret_key: np.ndarray = field(init=False)
    _enc_counter: int = field(init=False, default=0)

    def __post_init__(self):
        p = self.parameters
        self.small_lwe_secret_key = client.gen_binary_key(self.seed, 1, p.lwe_dimension)
        self.glwe_secret_key = client.gen_binary_key(self.seed, 2, p.glwe_dimension * p.polynomial_size)

    @property
    def large_lwe_secret_key(self) -> np.ndarray:
        return self.glwe_secret_key  # GlweSecretKey::into_lwe_secret_key

    @property
    def pbs_order(self) -> str:
        return KEYSWITCH_BOOTSTRAP if self.parameters.encryption_key_choice == "Big" else BOOTSTRAP_KEYSWITCH

    def _enc_key(self):
        p = self.parameters
        if self.pbs_order == KEYSWITCH_BOOTSTRAP:
            return self.large_lwe_secret_key, p.glwe_modular_std_dev
        return self.small_lwe_secret_key, p.lwe_modular_std_dev

    def encrypt_many(self, messages) -> list[Ciphertext]:
        p = self.parameters
        m = np.asarray(messages, dtype=np.uint64) % np.uint64(p.message_modulus)
        key, std = self._enc_key()
        self._enc_counter += 1
        cts = client.lwe_encrypt((self.seed << 20) + self._enc_counter, key, m * np.uint64(p.delta), std)
        return [Ciphertext(cts[i].copy(), p.message_modulus - 1, NOISE_NOMINAL, p.message_modulus,
                           p.carry_modulus, self.pbs_order) for i in range(len(m))]

    def encrypt(self, message: int) -> Ciphertext:
        return self.encrypt_many([message])[0]

    def encrypt_compressed_many(self, messages) -> list["CompressedCiphertext"]:
        """One CompressedCiphertext per message, each under a CompressionSeed of its own (derived from the key's
        seed and a counter; the reference draws it from its seeder)."""
        p = self.parameters
        m = np.asarray(messages, dtype=np.uint64) % np.uint64(p.message_modulus)
        key, std = self._enc_key()
        self._enc_counter += 1
        base = ((self.seed << 20) + self._enc_counter) << 64
        seeds = [(base + i) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % (1 << 128) for i in range(len(m))]
        bodies = client.seeded_lwe_encrypt((self.seed << 20) + self._enc_counter, seeds, key, m * np.uint64(p.delta), std)
        return [CompressedCiphertext(int(bodies[i]), seeds[i], len(key), p.message_modulus - 1, NOISE_NOMINAL,
                                     p.message_modulus, p.carry_modulus, self.pbs_order) for i in range(len(m))]

    def decrypt_message_and_carry_many(self, cts: list[Ciphertext]) -> np.ndarray:
        key = self.large_lwe_secret_key if cts[0].pbs_order == KEYSWITCH_BOOTSTRAP else self.small_lwe_secret_key
        raw = client.lwe_decrypt(key, np.stack([c.ct for c in cts]))
        return client.decode(raw, self.parameters.delta)

    def decrypt_message_and_carry(self, ct: Ciphertext) -> int:
        return int(self.decrypt_message_and_carry_many([ct])[0])

    def decrypt(self, ct: Ciphertext) -> int:
        return self.decrypt_message_and_carry(ct) % ct.message_modulus

    # -- without padding bit (the WoP-PBS encoding): delta doubled, the message not reduced --------
    def encrypt_without_padding_many(self, messages) -> list[Ciphertext]:
        p = self.parameters
        m = np.asarray(messages, dtype=np.uint64)
        key, std = self._enc_key()
        self._enc_counter += 1
        cts = client.lwe_encrypt((self.seed << 20) + self._enc_counter, key, m * np.uint64(2 * p.delta), std)
        return [Ciphertext(cts[i].copy(), p.message_modulus - 1, NOISE_NOMINAL, p.message_modulus,
                           p.carry_modulus, self.pbs_order) for i in range(len(m))]

    def encrypt_without_padding(self, message: int) -> Ciphertext:
        return self.encrypt_without_padding_many([message])[0]

    def decrypt_message_and_carry_without_padding_many(self, cts: list[Ciphertext]) -> np.ndarray:
        key = self.large_lwe_secret_key if cts[0].pbs_order == KEYSWITCH_BOOTSTRAP else self.small_lwe_secret_key
        raw = client.lwe_decrypt(key, np.stack([c.ct for c in cts]))
        return client.decode(raw, 2 * self.parameters.delta)

    def decrypt_message_and_carry_without_padding(self, ct: Ciphertext) -> int:
        return int(self.decrypt_message_and_carry_without_padding_many([ct])[0])

    def decrypt_without_padding(self, ct: Ciphertext) -> int:
        return self.decrypt_message_and_carry_without_padding(ct) % ct.message_modulus


def _order_code(pbs_order: str) -> int:
    return 0 if pbs_order == KEYSWITCH_BOOTSTRAP else 1


def _order_name(code: int) -> str:
    return KEYSWITCH_BOOTSTRAP if code == 0 else BOOTSTRAP_KEYSWITCH


def _engine_of(where) -> Engine:
    return where.engine if hasattr(where, "engine") else where


@dataclass
class CompressedCiphertext:
    """shortint CompressedCiphertext (ciphertext/mod.rs:467-476): a SeededLweCiphertext -- one body word and the
    CompressionSeed of its mask."""

    body: int
    seed: int
    lwe_dimension: int
    degree: int
    noise_level: int
    message_modulus: int
    carry_modulus: int
    pbs_order: str

    def decompress(self, where) -> Ciphertext:
        """The full ciphertext, its mask regenerated on the GPU of `where` (an Engine or a ServerKey)."""
        return decompress_many([self], where)[0]

    def serialize(self) -> bytes:
        from .serialization import serialize_compressed_ciphertext

        return serialize_compressed_ciphertext(self.body, self.lwe_dimension, self.seed, self.degree, self.message_modulus,
                                               self.carry_modulus, _order_code(self.pbs_order), self.noise_level)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressedCiphertext":
        from .serialization import inspect_compressed_ciphertext

        i = inspect_compressed_ciphertext(data)
        return cls(int(i.words(data)[0]), i.seed, i.lwe_dimension, i.degree, i.noise_level, i.message_modulus,
                   i.carry_modulus, _order_name(i.pbs_order))


def _compressed_source(cts: list[CompressedCiphertext]) -> LweSource:
    n = cts[0].lwe_dimension
    if any(c.lwe_dimension != n for c in cts):
        raise ValueError("compressed ciphertexts of different LweSize")
    return LweSource("seeded_rows", n, np.array([c.body for c in cts], dtype=np.uint64), seeds=[c.seed for c in cts])


def decompress_many(cts: list[CompressedCiphertext], where) -> list[Ciphertext]:
    rows = _engine_of(where).lwe_expand(_compressed_source(cts))
    return [Ciphertext(rows[i].copy(), c.degree, c.noise_level, c.message_modulus, c.carry_modulus, c.pbs_order)
            for i, c in enumerate(cts)]


@dataclass
class CompactCiphertextList:
    """shortint CompactCiphertextList (ciphertext/mod.rs:521-529): an LweCompactCiphertextList container
    ([ceil(count / n)][n] masks, then [count] bodies) and the fields every ciphertext of it gets."""

    container: np.ndarray
    lwe_dimension: int
    count: int
    degree: int
    noise_level: int
    message_modulus: int
    carry_modulus: int
    pbs_order: str

    def __len__(self):
        return self.count

    def source(self) -> LweSource:
        return LweSource("compact", self.lwe_dimension, self.container, count=self.count)

    def expand(self, where) -> list[Ciphertext]:
        """The ciphertexts, expanded on the GPU of `where` (an Engine or a ServerKey)."""
        rows = _engine_of(where).lwe_expand(self.source())
        return [Ciphertext(rows[i].copy(), self.degree, self.noise_level, self.message_modulus, self.carry_modulus,
                           self.pbs_order) for i in range(self.count)]

    def serialize(self) -> bytes:
        from .serialization import serialize_compact_ciphertext_list

        return serialize_compact_ciphertext_list(self.container, self.lwe_dimension, self.count, self.degree,
                                                 self.message_modulus, self.carry_modulus, _order_code(self.pbs_order),
                                                 self.noise_level)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompactCiphertextList":
        from .serialization import inspect_compact_ciphertext_list

        i = inspect_compact_ciphertext_list(data)
        return cls(i.words(data), i.lwe_dimension, i.count, i.degree, i.noise_level, i.message_modulus, i.carry_modulus,
                   _order_name(i.pbs_order))


class CompactPublicKey:
    """shortint CompactPublicKey (public_key/compact.rs): an LweCompactPublicKey of the client key's encryption key
    (the big key for KS -> PBS sets, the small one for PBS -> KS sets); its dimension must be a power of two."""

    def __init__(self, client_key: ClientKey):
        self.parameters = client_key.parameters
        self.pbs_order = client_key.pbs_order
        key, self.std_dev = client_key._enc_key()
        self.lwe_dimension = len(key)
        self.seed = client_key.seed
        self._counter = 0
        self.key = client.gen_compact_public_key(client_key.seed * 7 + 5, key, self.std_dev)

    def encrypt_many(self, messages) -> CompactCiphertextList:
        p = self.parameters
        m = np.asarray(messages, dtype=np.uint64) % np.uint64(p.message_modulus)
        self._counter += 1
        box = client.compact_encrypt((self.seed << 20) + (1 << 19) + self._counter, self.key, m * np.uint64(p.delta),
                                     self.std_dev)
        return CompactCiphertextList(box, self.lwe_dimension, len(m), p.message_modulus - 1, NOISE_NOMINAL,
                                     p.message_modulus, p.carry_modulus, self.pbs_order)


class ServerKey:
    """shortint ServerKey whose bootstrapping key is the MI355X engine (the `Gpu` arm of
    ShortintBootstrappingKey, server_key/mod.rs:104-111)."""

    def __init__(self, client_key: ClientKey | None = None, device: int = 0, *, engine: Engine | None = None,
                 bsk: np.ndarray | None = None, ksk: np.ndarray | None = None,
                 parameters: ClassicPBSParameters | None = None):
        p = client_key.parameters if client_key is not None else parameters
        if p is None:
            raise ValueError("parameters required")
        self.parameters = p
        self.message_modulus = p.message_modulus
        self.carry_modulus = p.carry_modulus
        self.engine = engine or Engine(p, device)
        if client_key is not None and bsk is None:
            ck = client_key
            if p.grouping_factor:
                bsk = client.gen_multi_bit_bootstrap_key(
                    ck.seed * 7 + 3, ck.small_lwe_secret_key, ck.glwe_secret_key, p.glwe_dimension,
                    p.polynomial_size, p.pbs_base_log, p.pbs_level, p.grouping_factor, p.glwe_modular_std_dev)
            else:
                bsk = client.gen_bootstrap_key(ck.seed * 7 + 3, ck.small_lwe_secret_key, ck.glwe_secret_key,
                                               p.glwe_dimension, p.polynomial_size, p.pbs_base_log,
                                               p.pbs_level, p.glwe_modular_std_dev)
            ksk = client.gen_keyswitch_key(ck.seed * 7 + 4, ck.large_lwe_secret_key, ck.small_lwe_secret_key,
                                           p.ks_base_log, p.ks_level, p.lwe_modular_std_dev)
        if bsk is not None:
            self.engine.upload_bootstrap_key(bsk)
        if ksk is not None:
            self.engine.upload_keyswitch_key(ksk)
        self.pbs_order = KEYSWITCH_BOOTSTRAP if p.encryption_key_choice == "Big" else BOOTSTRAP_KEYSWITCH

    @classmethod
    def deserialize(cls, data: bytes, device: int = 0, parameters: ClassicPBSParameters | None = None) -> "ServerKey":
        """A bincode-serialized shortint ServerKey (server_key/mod.rs:283-297: standard KSK +
        Fourier BSK) straight onto the GPU (serialization.py, csrc/serde.cpp)."""
        from .serialization import inspect_server_key

        p = parameters or inspect_server_key(data).parameters()
        eng = Engine(p, device)
        eng.upload_server_key(data)
        return cls(None, engine=eng, parameters=p)

    # -- lookup tables ---------------------------------------------------------------------
    def generate_lookup_table(self, f) -> LookupTable:
        p = self.parameters
        acc = fill_accumulator(p, f)
        max_value = max(int(f(i)) for i in range(p.message_modulus * p.carry_modulus))
        return LookupTable(acc, max_value)

    def generate_msg_lookup_table(self, f, modulus: int) -> LookupTable:
        return self.generate_lookup_table(lambda x: f(x % modulus) % modulus)

    # -- PBS ---------------------------------------------------------------------------------
    def trivial_pbs_assign(self, ct: Ciphertext, acc: LookupTable) -> None:
        assert ct.noise_level == NOISE_ZERO
        p = self.parameters
        modulus_sup = p.message_modulus * p.carry_modulus
        delta = p.delta
        value = int(ct.ct[-1]) // delta
        box = p.polynomial_size // modulus_sup
        body = acc.acc[p.glwe_dimension * p.polynomial_size:]
        if value >= modulus_sup:
            res = (0 - int(body[(value % modulus_sup) * box])) % (1 << 64)
        else:
            res = int(body[value * box])
        ct.ct[-1] = np.uint64(res)
        ct.degree = acc.degree

    def create_trivial(self, value: int) -> Ciphertext:
        p = self.parameters
        dim = p.big_lwe_dimension if self.pbs_order == KEYSWITCH_BOOTSTRAP else p.lwe_dimension
        ct = np.zeros(dim + 1, dtype=np.uint64)
        ct[-1] = np.uint64((value % (p.message_modulus * p.carry_modulus)) * p.delta)
        return Ciphertext(ct, value, NOISE_ZERO, p.message_modulus, p.carry_modulus, self.pbs_order)

    def engine_ks_pbs(self, x: np.ndarray, luts: np.ndarray, lut_indexes=None) -> np.ndarray:
        """One batched launch of the key's PBS order over rows of x (big-key LWEs for KS->PBS)."""
        if self.pbs_order == KEYSWITCH_BOOTSTRAP:
            return self.engine.keyswitch_programmable_bootstrap(x, luts, lut_indexes)
        return self.engine.programmable_bootstrap_keyswitch(x, luts, lut_indexes)

    def apply_lookup_table_batch_assign(self, cts: list[Ciphertext], accs) -> None:
        """One GPU launch for a whole layer; accs: one LookupTable or one per ciphertext."""
        if isinstance(accs, LookupTable):
            accs = [accs] * len(cts)
        todo = [i for i, c in enumerate(cts) if not c.is_trivial()]
        for i, c in enumerate(cts):
            if c.is_trivial():
                self.trivial_pbs_assign(c, accs[i])
        if todo:
            uniq, idx = {}, []
            for i in todo:
                key = id(accs[i])
                if key not in uniq:
                    uniq[key] = (len(uniq), accs[i].acc)
                idx.append(uniq[key][0])
            luts = np.stack([a for _, a in sorted(uniq.values(), key=lambda t: t[0])])
            x = np.stack([cts[i].ct for i in todo])
            lut_idx = np.asarray(idx, dtype=np.uint32) if len(uniq) > 1 else None
            if self.pbs_order == KEYSWITCH_BOOTSTRAP:
                out = self.engine.keyswitch_programmable_bootstrap(x, luts, lut_idx)
            else:
                out = self.engine.programmable_bootstrap_keyswitch(x, luts, lut_idx)
            for j, i in enumerate(todo):
                cts[i].ct = out[j].copy()
                cts[i].noise_level = NOISE_NOMINAL
        for i, c in enumerate(cts):
            c.degree = accs[i].degree

    def _apply_from(self, source: LweSource, like, accs) -> list[Ciphertext]:
        """a compressed source straight through the key's PBS order (Engine.apply_from): the rows are expanded on
        the GPU, chunk by chunk, where the copy of expanded rows would have landed"""
        count = source.count
        if isinstance(accs, LookupTable):
            accs = [accs] * count
        uniq, idx = {}, []
        for a in accs:
            if id(a) not in uniq:
                uniq[id(a)] = (len(uniq), a.acc)
            idx.append(uniq[id(a)][0])
        luts = np.stack([a for _, a in sorted(uniq.values(), key=lambda t: t[0])])
        lut_idx = np.asarray(idx, dtype=np.uint32) if len(uniq) > 1 else None
        op = "ks_pbs" if self.pbs_order == KEYSWITCH_BOOTSTRAP else "pbs_ks"
        out = self.engine.apply_from(op, source, luts, lut_idx)
        return [Ciphertext(out[i].copy(), accs[i].degree, NOISE_NOMINAL, like(i).message_modulus, like(i).carry_modulus,
                           self.pbs_order) for i in range(count)]

    def apply_lookup_table_batch(self, cts, accs) -> list[Ciphertext]:
        """cts: a list of Ciphertext, or -- compressed ingress -- a CompactCiphertextList or a list of
        CompressedCiphertext, which go to the GPU in their compressed form."""
        if isinstance(cts, CompactCiphertextList):
            return self._apply_from(cts.source(), lambda i: cts, accs) if cts.count else []
        if len(cts) and all(isinstance(c, CompressedCiphertext) for c in cts):
            return self._apply_from(_compressed_source(cts), lambda i: cts[i], accs)
        res = [c.clone() for c in cts]
        self.apply_lookup_table_batch_assign(res, accs)
        return res

    def apply_lookup_table_assign(self, ct: Ciphertext, acc: LookupTable) -> None:
        self.apply_lookup_table_batch_assign([ct], acc)

    def apply_lookup_table(self, ct: Ciphertext, acc: LookupTable) -> Ciphertext:
        res = ct.clone()
        self.apply_lookup_table_assign(res, acc)
        return res

    def keyswitch_programmable_bootstrap_assign(self, ct: Ciphertext, acc: LookupTable) -> None:
        if ct.is_trivial():
            self.trivial_pbs_assign(ct, acc)
            return
        ct.ct = self.engine.keyswitch_programmable_bootstrap(ct.ct, acc.acc)[0].copy()
        ct.degree = acc.degree
        ct.noise_level = NOISE_NOMINAL

    def programmable_bootstrap_keyswitch_assign(self, ct: Ciphertext, acc: LookupTable) -> None:
        if ct.is_trivial():
            self.trivial_pbs_assign(ct, acc)
            return
        ct.ct = self.engine.programmable_bootstrap_keyswitch(ct.ct, acc.acc)[0].copy()
        ct.degree = acc.degree
        ct.noise_level = NOISE_NOMINAL

    def message_extract(self, ct: Ciphertext) -> Ciphertext:
        acc = self.generate_lookup_table(lambda x: x % ct.message_modulus)
        return self.apply_lookup_table(ct, acc)

    def carry_extract(self, ct: Ciphertext) -> Ciphertext:
        acc = self.generate_lookup_table(lambda x: x // ct.message_modulus)
        return self.apply_lookup_table(ct, acc)


class WopbsKey:
    """shortint WopbsKey (wopbs/mod.rs) on the engine of its server key: the circuit bootstrap's private
    functional packing keyswitching keys next to the bootstrapping and keyswitching keys."""

    def __init__(self, wopbs_server_key: ServerKey, param: WopbsParameters, pfpksk: np.ndarray | None = None, *,
                 pbs_server_key: ServerKey | None = None, ksk_pbs_to_wopbs=None, ksk_wopbs_to_pbs=None):
        """pbs_server_key: the PBS set's server key (None: the WoP set is the PBS set, a key "only for
        wopbs").  ksk_pbs_to_wopbs: keyswitching key object PBS big key -> WoP big key on the WoP engine;
        ksk_wopbs_to_pbs: WoP big key -> PBS small key on the PBS server key's engine (the reference's
        pbs_server_key.key_switching_key)."""
        if not isinstance(param, WopbsParameters):
            raise ValueError("WopbsKey needs WopbsParameters")
        if param.pbs_level > 4:
            raise ValueError(f"pbs_level {param.pbs_level}: no classic PBS kernel for WoP-PBS sets of 5 or 6 levels")
        self.wopbs_server_key = wopbs_server_key
        self.pbs_server_key = pbs_server_key if pbs_server_key is not None else wopbs_server_key
        self.ksk_pbs_to_wopbs = ksk_pbs_to_wopbs
        self.ksk_wopbs_to_pbs = ksk_wopbs_to_pbs
        self.param = param
        self._wopbs_client_key = None
        if pfpksk is not None:
            wopbs_server_key.engine.upload_pfpksk_list(pfpksk, param.pfks_base_log, param.pfks_level)

    @classmethod
    def new_wopbs_key(cls, cks: ClientKey, sks: ServerKey, parameters: WopbsParameters, device: int = 0,
                      engine=None) -> "WopbsKey":
        """engine/wopbs/mod.rs:50-183: secret keys of the WoP set's own, its bootstrapping, keyswitching and
        pfpks keys on a second engine (`engine`, or a new Engine on `device`), and the two keyswitching
        keys between the sets.  Every seed derives from cks.seed."""
        if not isinstance(parameters, WopbsParameters):
            raise ValueError("new_wopbs_key: parameters are no WopbsParameters")
        if parameters.grouping_factor or cks.parameters.grouping_factor:
            raise ValueError("new_wopbs_key: multi-bit keys are not supported (the reference refuses them)")
        p, pp = parameters, cks.parameters
        wcks = ClientKey(p, cks.seed * 7 + 6)
        s = wcks.seed
        bsk = client.gen_bootstrap_key(s * 7 + 3, wcks.small_lwe_secret_key, wcks.glwe_secret_key, p.glwe_dimension,
                                       p.polynomial_size, p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev)
        ksk = client.gen_keyswitch_key(s * 7 + 4, wcks.large_lwe_secret_key, wcks.small_lwe_secret_key, p.ks_base_log,
                                       p.ks_level, p.lwe_modular_std_dev)
        pfpksk = client.gen_pfpksk_list(s * 7 + 5, wcks.large_lwe_secret_key, wcks.glwe_secret_key, p.glwe_dimension,
                                        p.polynomial_size, p.pfks_base_log, p.pfks_level, p.pfks_modular_std_dev)
        # PBS big key -> WoP big key: the PBS set's keyswitch decomposition, the WoP set's LWE noise
        to_wop = client.gen_keyswitch_key(cks.seed * 7 + 8, cks.large_lwe_secret_key, wcks.large_lwe_secret_key,
                                          pp.ks_base_log, pp.ks_level, p.lwe_modular_std_dev)
        # WoP big key -> PBS small key: the PBS set's decomposition and noise
        to_pbs = client.gen_keyswitch_key(cks.seed * 7 + 9, wcks.large_lwe_secret_key, cks.small_lwe_secret_key,
                                          pp.ks_base_log, pp.ks_level, pp.lwe_modular_std_dev)
        wop_engine = engine if engine is not None else Engine(p, device)
        wsks = ServerKey(None, engine=wop_engine, bsk=bsk, ksk=ksk, parameters=p)
        wsks.pbs_order = sks.pbs_order
        key = cls(wsks, p, pfpksk, pbs_server_key=sks,
                  ksk_pbs_to_wopbs=wop_engine.keyswitch_key(to_wop, pp.big_lwe_dimension, p.big_lwe_dimension,
                                                            pp.ks_base_log, pp.ks_level),
                  ksk_wopbs_to_pbs=sks.engine.keyswitch_key(to_pbs, p.big_lwe_dimension, pp.lwe_dimension,
                                                            pp.ks_base_log, pp.ks_level))
        key._wopbs_client_key = wcks
        return key

    @classmethod
    def new_wopbs_key_only_for_wopbs(cls, cks: ClientKey, sks: ServerKey) -> "WopbsKey":
        p = cks.parameters
        if not isinstance(p, WopbsParameters):
            raise ValueError("new_wopbs_key_only_for_wopbs: the client key's parameters are no WopbsParameters")
        pfpksk = client.gen_pfpksk_list(cks.seed * 7 + 5, cks.large_lwe_secret_key, cks.glwe_secret_key,
                                        p.glwe_dimension, p.polynomial_size, p.pfks_base_log, p.pfks_level,
                                        p.pfks_modular_std_dev)
        key = cls(sks, p, pfpksk)
        key._wopbs_client_key = cks
        return key

    @property
    def engine(self) -> Engine:
        return self.wopbs_server_key.engine

    def _basis_bits(self, ct: Ciphertext) -> int:
        return int(np.ceil(np.log2(ct.message_modulus * ct.carry_modulus)))

    def _lut(self, ct: Ciphertext, f, delta_log: int) -> np.ndarray:
        lut = np.zeros(self.param.polynomial_size, dtype=np.uint64)
        for i in range(ct.message_modulus * ct.carry_modulus):
            lut[i] = np.uint64((int(f(i % ct.message_modulus)) << delta_log) % (1 << 64))
        return lut

    def generate_lut(self, ct: Ciphertext, f) -> np.ndarray:
        """one bit of padding: entry i = f(i mod message_modulus) << (63 - log2(basis))."""
        return self._lut(ct, f, 64 - self._basis_bits(ct) - 1)

    def generate_lut_without_padding(self, ct: Ciphertext, f) -> np.ndarray:
        return self._lut(ct, f, 64 - self._basis_bits(ct))

    def extract_bits_circuit_bootstrapping(self, cts, lut, delta_log: int, nbits: int):
        """extract_bits then circuit_bootstrap_boolean_vertical_packing (wopbs/mod.rs:825-857); a list of
        ciphertexts is one batch."""
        single = isinstance(cts, Ciphertext)
        batch = [cts] if single else list(cts)
        if batch[0].pbs_order != KEYSWITCH_BOOTSTRAP:
            raise ValueError("WoP-PBS runs on big-key ciphertexts (KeyswitchBootstrap order)")
        p = self.param
        lut = np.ascontiguousarray(lut, dtype=np.uint64).reshape(1, 1, -1, p.polynomial_size)
        bits = self.engine.extract_bits(np.stack([c.ct for c in batch]), delta_log, nbits)
        out = self.engine.circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, lut)
        sks = self.wopbs_server_key
        res = [Ciphertext(out[i, 0].copy(), sks.message_modulus - 1, NOISE_NOMINAL, sks.message_modulus,
                          sks.carry_modulus, batch[i].pbs_order) for i in range(len(batch))]
        return res[0] if single else res

    def wopbs(self, ct_in, lut):
        p = self.param
        delta_log = p.delta.bit_length() - 1
        return self.extract_bits_circuit_bootstrapping(ct_in, lut, delta_log,
                                                       int(np.log2(p.message_modulus * p.carry_modulus)))

    def programmable_bootstrapping_without_padding(self, ct_in, lut):
        p = self.param
        delta_log = (2 * p.delta).bit_length() - 1
        return self.extract_bits_circuit_bootstrapping(ct_in, lut, delta_log,
                                                       int(np.log2(p.message_modulus * p.carry_modulus)))


    # -- between the PBS and the WoP parameter sets (wopbs/mod.rs:660-754); a list is one batch -------
    @staticmethod
    def _batch(cts):
        single = isinstance(cts, Ciphertext)
        return single, ([cts] if single else list(cts))

    def keyswitch_to_wopbs_params(self, sks: ServerKey, ct_in):
        """Identity PBS under the PBS set (to clean the noise), then the keyswitch PBS big key -> WoP big
        key.  The degree is the input's (the identity LUT would set the maximum)."""
        if self.ksk_pbs_to_wopbs is None:
            raise ValueError("keyswitch_to_wopbs_params: a key only for wopbs has no PBS -> WoP keyswitching key "
                             "(the reference's would be the big -> small one and its result unusable)")
        single, batch = self._batch(ct_in)
        clean = sks.apply_lookup_table_batch(batch, sks.generate_lookup_table(lambda x: x))
        out = self.engine.keyswitch_with_key(self.ksk_pbs_to_wopbs, np.stack([c.ct for c in clean]))
        res = [Ciphertext(out[i].copy(), batch[i].degree, NOISE_NOMINAL, clean[i].message_modulus,
                          clean[i].carry_modulus, batch[i].pbs_order) for i in range(len(batch))]
        return res[0] if single else res

    def keyswitch_to_pbs_params(self, ct_in):
        """Keyswitch WoP big key -> PBS small key, then an identity PBS under the PBS set."""
        single, batch = self._batch(ct_in)
        ps = self.pbs_server_key
        x = np.stack([c.ct for c in batch])
        if self.ksk_wopbs_to_pbs is None:
            small = ps.engine.keyswitch(x)
        else:
            small = ps.engine.keyswitch_with_key(self.ksk_wopbs_to_pbs, x)
        out = ps.engine.programmable_bootstrap(small, ps.generate_lookup_table(lambda x: x).acc)
        res = [Ciphertext(out[i].copy(), c.degree, NOISE_NOMINAL, c.message_modulus, c.carry_modulus, c.pbs_order)
               for i, c in enumerate(batch)]
        return res[0] if single else res

    def programmable_bootstrapping(self, sks: ServerKey, ct_in, lut):
        """wopbs/mod.rs:398-408: to the WoP set, the WoP-PBS, back to the PBS set."""
        return self.keyswitch_to_pbs_params(self.wopbs(self.keyswitch_to_wopbs_params(sks, ct_in), lut))

    def extract_bits(self, delta_log: int, ct_in, nbits: int) -> np.ndarray:
        """[nbits][n+1] for one ciphertext, [count][nbits][n+1] for a list, most significant bit first."""
        single, batch = self._batch(ct_in)
        bits = self.engine.extract_bits(np.stack([c.ct for c in batch]), delta_log, nbits)
        return bits[0] if single else bits

    def circuit_bootstrapping_vertical_packing(self, lut, bits) -> np.ndarray:
        """lut [nout][size] (size a multiple of N), bits [count][nbits][n+1] (or [nbits][n+1]): one composed
        call with nout outputs under one set of GGSWs; returns [count][nout][kN+1] (or [nout][kN+1])."""
        p = self.param
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        if lut.ndim != 2 or lut.shape[1] % p.polynomial_size:
            raise ValueError("circuit_bootstrapping_vertical_packing: lut must be [nout][size], size a multiple of N")
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        single = bits.ndim == 2
        if single:
            bits = bits.reshape(1, *bits.shape)
        out = self.engine.circuit_bootstrap_vertical_packing(
            bits, p.cbs_base_log, p.cbs_level, lut.reshape(1, lut.shape[0], -1, p.polynomial_size))
        return out[0] if single else out


class CompressedServerKey:
    """shortint CompressedServerKey (server_key/compressed.rs:43-55) in its serialized (bincode)
    form: seeded keyswitching and bootstrapping keys, decompressed on the GPU."""

    def __init__(self, data: bytes):
        from .serialization import inspect_compressed_server_key

        self.data = bytes(data)
        self.info = inspect_compressed_server_key(self.data)   # validates the whole buffer

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressedServerKey":
        return cls(data)

    def decompress(self, device: int = 0, parameters: ClassicPBSParameters | None = None) -> ServerKey:
        """CompressedServerKey::decompress (compressed.rs) + the Fourier conversion, on the GPU."""
        p = parameters or self.info.parameters()
        eng = Engine(p, device)
        eng.upload_compressed_server_key(self.data)
        return ServerKey(None, engine=eng, parameters=p)


def gen_keys(parameters: ClassicPBSParameters, seed: int = 0, device: int = 0):
    ck = ClientKey(parameters, seed)
    sk = ServerKey(ck, device)
    return ck, sk
