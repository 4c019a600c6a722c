"""tfhe::boolean on the MI355X engine's 32-bit-torus path (include/tfhe_mi355.h "32-bit torus").

Mirrors tfhe/src/boolean: the five parameter sets (boolean/parameters/mod.rs:123-192), a ClientKey
(encrypt / decrypt of bools, boolean/engine/mod.rs:241-270, 354-375) and a ServerKey with the gates of
BinaryGatesEngine (mod.rs:607-1065), NOT (mod.rs:377-398) and MUX (mod.rs:461-569) -- on BATCHES: a
BoolBatch is `count` ciphertexts [count][size] of u32 words (a host numpy array, or a torch.int32
device tensor), or one trivial value for the whole batch (the reference's Ciphertext::Trivial).

The ServerKey runs over any engine object with the u32 methods of tfhe_mi355.Engine
(boolean_gates, boolean_mux, boolean_not, and the _async forms for device tensors), so the gate algebra
is the same code over the HIP engine and over a CPU restatement of it.
"""
from __future__ import annotations

import numpy as np

from . import client
from .parameters import (BOOLEAN_DEFAULT_PARAMETERS as DEFAULT_PARAMETERS,
                         BOOLEAN_DEFAULT_PARAMETERS_KS_PBS as DEFAULT_PARAMETERS_KS_PBS,
                         BOOLEAN_PARAMETER_SETS as PARAMETER_SETS,
                         BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165 as PARAMETERS_ERROR_PROB_2_POW_MINUS_165,
                         BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS
                         as PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS,
                         BOOLEAN_TFHE_LIB_PARAMETERS as TFHE_LIB_PARAMETERS, BooleanParameters)

# boolean/mod.rs:77-80
PLAINTEXT_TRUE = 1 << 29
PLAINTEXT_FALSE = 7 << 29

# opcodes of tfhe_mi355_boolean_gates
AND, NAND, NOR, OR, XOR, XNOR = range(6)
GATE_NAMES = ("and", "nand", "nor", "or", "xor", "xnor")
_TRUTH = {
    AND: lambda a, b: a and b, NAND: lambda a, b: not (a and b), NOR: lambda a, b: not (a or b),
    OR: lambda a, b: a or b, XOR: lambda a, b: a != b, XNOR: lambda a, b: a == b,
}


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr")


class BoolBatch:
    """`count` boolean ciphertexts: `data` [count][size] u32 words (numpy uint32 on the host, torch.int32 on
    the device), or -- `data` None -- the trivial value `value` for the whole batch."""

    def __init__(self, data=None, value=None, count=None):
        if data is None:
            if value is None or count is None:
                raise ValueError("a trivial batch needs a value and a count")
            self.data, self.value, self.count = None, bool(value), int(count)
            return
        if not _is_device(data):
            data = np.ascontiguousarray(data, dtype=np.uint32)
        if data.ndim != 2:
            raise ValueError("ciphertext batches are [count][size]")
        self.data, self.value, self.count = data, None, int(data.shape[0])

    @classmethod
    def trivial(cls, value: bool, count: int) -> "BoolBatch":
        return cls(None, value, count)

    @property
    def is_trivial(self) -> bool:
        return self.data is None

    @property
    def on_device(self) -> bool:
        return self.data is not None and _is_device(self.data)

    def clone(self) -> "BoolBatch":
        if self.is_trivial:
            return BoolBatch.trivial(self.value, self.count)
        return BoolBatch(self.data.clone() if self.on_device else self.data.copy())

    def host(self) -> np.ndarray:
        """The ciphertext words as a numpy uint32 array (copied off the device if needed)."""
        if self.is_trivial:
            raise ValueError("a trivial batch has no ciphertext words")
        if self.on_device:
            return self.data.cpu().numpy().view(np.uint32)
        return self.data


class ClientKey:
    """boolean::ClientKey: the LWE and GLWE secret keys of a parameter set.  Encryption is under the key
    `encryption_key_choice` names, with its noise (mod.rs:249-258); decryption is phase < 2^31
    (mod.rs:354-375).  The randomness is the client helpers' seeded stream (tfhe_mi355.client)."""

    def __init__(self, parameters: BooleanParameters, seed: int):
        p = parameters
        self.parameters, self.seed = p, seed
        self.lwe_secret_key = client.gen_binary_key(seed, 1, p.lwe_dimension)
        self.glwe_secret_key = client.gen_binary_key(seed, 2, p.big_lwe_dimension)
        self._calls = 0

    def _encryption_key(self):
        p = self.parameters
        if p.encryption_key_choice == "Big":
            return self.glwe_secret_key, p.glwe_modular_std_dev
        return self.lwe_secret_key, p.lwe_modular_std_dev

    def encrypt(self, messages) -> BoolBatch:
        m = np.asarray(messages, dtype=bool).ravel()
        sk, std = self._encryption_key()
        pts = np.where(m, PLAINTEXT_TRUE, PLAINTEXT_FALSE).astype(np.uint32)
        self._calls += 1
        return BoolBatch(client.lwe_encrypt_u32(self.seed * 1000003 + self._calls, sk, pts, std))

    def decrypt(self, batch: BoolBatch) -> np.ndarray:
        if batch.is_trivial:
            return np.full(batch.count, batch.value, dtype=bool)
        sk, _ = self._encryption_key()
        return client.lwe_decrypt_u32(sk, batch.host()) < np.uint32(1 << 31)

    def server_key_material(self):
        """(u32 bootstrapping key, u32 keyswitching key) in the standard domain.

        Generated by the u64 client generators and rounded to the top 32 bits, (x + 2^31) >> 32
        (client.round_to_u32): the rounding adds a uniform error of at most 2^-33 per word, below the
        noise of every boolean parameter set.  BSK: lwe key under the glwe key, glwe noise
        (bootstrapping.rs:160-171); KSK: glwe key (as an LWE key) to the lwe key, lwe noise
        (bootstrapping.rs:197-206, mod.rs:226-234)."""
        p = self.parameters
        bsk = client.gen_bootstrap_key(self.seed + 1, self.lwe_secret_key, self.glwe_secret_key, p.glwe_dimension,
                                       p.polynomial_size, p.pbs_base_log, p.pbs_level, p.glwe_modular_std_dev)
        ksk = client.gen_keyswitch_key(self.seed + 2, self.glwe_secret_key, self.lwe_secret_key, p.ks_base_log,
                                       p.ks_level, p.lwe_modular_std_dev)
        return client.round_to_u32(bsk), client.round_to_u32(ksk)


class ServerKey:
    """boolean::ServerKey over `engine` (a tfhe_mi355.Engine with the u32 keys uploaded, or any object with
    the same u32 methods).  Operands are BoolBatch objects or one Python bool for the whole batch; the
    reference's shortcuts for plain and trivial operands apply as written (mod.rs:470-500, 614-623,
    970-1065): they return a trivial batch, a clone or a negation, and run no bootstrap."""

    def __init__(self, engine, parameters: BooleanParameters):
        self.engine, self.parameters = engine, parameters
        self.pbs_order = parameters.pbs_order

    # -- encrypted paths ---------------------------------------------------------------------------
    def _check(self, *batches):
        w = self.parameters.ciphertext_words
        count = batches[0].count
        for b in batches:
            if b.is_trivial or b.data.shape != (count, w):
                raise ValueError(f"encrypted operands must be [count][{w}] batches of one size")
        dev = [b.on_device for b in batches]
        if any(dev) != all(dev):
            raise ValueError("operands must all be on the host or all on the device")
        return count, all(dev)

    def gates(self, ops, lhs: BoolBatch, rhs: BoolBatch) -> BoolBatch:
        """One mixed batch: item i computes gate ops[i] (AND .. XNOR) of lhs[i], rhs[i]; one prologue, one
        PBS and one keyswitch launch for the whole batch.  Both operands encrypted."""
        count, dev = self._check(lhs, rhs)
        ops = np.ascontiguousarray(ops, dtype=np.uint8).ravel()
        if ops.size != count:
            raise ValueError("one opcode per gate")
        if not dev:
            return BoolBatch(self.engine.boolean_gates(ops, lhs.data, rhs.data, self.pbs_order))
        import torch

        if ops.size and ops.max() > XNOR:
            raise ValueError("opcode above 5")
        d_ops = torch.from_numpy(ops).to(lhs.data.device)
        out = torch.empty_like(lhs.data)
        self.engine.boolean_gates_async(d_ops, lhs.data, rhs.data, out, count, self.pbs_order)
        return BoolBatch(out)

    def _mux_encrypted(self, cond, then_, else_) -> BoolBatch:
        count, dev = self._check(cond, then_, else_)
        if not dev:
            return BoolBatch(self.engine.boolean_mux(cond.data, then_.data, else_.data, self.pbs_order))
        import torch

        out = torch.empty_like(cond.data)
        self.engine.boolean_mux_async(cond.data, then_.data, else_.data, out, count, self.pbs_order)
        return BoolBatch(out)

    # -- NOT: a negation of every word, no bootstrap (mod.rs:377-398) ---------------------------------
    def not_(self, ct: BoolBatch) -> BoolBatch:
        if ct.is_trivial:
            return BoolBatch.trivial(not ct.value, ct.count)
        if not ct.on_device:
            return BoolBatch(self.engine.boolean_not(ct.data))
        import torch

        out = torch.empty_like(ct.data)
        self.engine.boolean_not_async(ct.data, out, ct.data.numel())
        return BoolBatch(out)

    # -- binary gates ----------------------------------------------------------------------------------
    def _plain(self, op: int, ct: BoolBatch, b: bool) -> BoolBatch:
        """gate(ct, plain b), BinaryGatesEngine<&Ciphertext, bool> (mod.rs:969-1039)."""
        triv = lambda v: BoolBatch.trivial(v, ct.count)  # noqa: E731
        if op == AND:
            return ct.clone() if b else triv(False)
        if op == NAND:
            return self.not_(ct) if b else triv(True)
        if op == NOR:
            return triv(False) if b else self.not_(ct)
        if op == OR:
            return triv(True) if b else ct.clone()
        if op == XOR:
            return self.not_(ct) if b else ct.clone()
        return ct.clone() if b else self.not_(ct)  # XNOR

    def _binary(self, op: int, left, right) -> BoolBatch:
        lb, rb = isinstance(left, (bool, np.bool_)), isinstance(right, (bool, np.bool_))
        if lb and rb:
            raise TypeError("at least one operand must be a BoolBatch")
        if rb:  # (ct, bool)
            return self._plain(op, left, bool(right))
        if lb:  # (bool, ct) = gate(ct, bool) (mod.rs:1041-1065)
            return self._plain(op, right, bool(left))
        if left.count != right.count:
            raise ValueError("operands of different batch sizes")
        if left.is_trivial and right.is_trivial:  # mod.rs:614-617
            return BoolBatch.trivial(_TRUTH[op](left.value, right.value), left.count)
        if right.is_trivial:  # mod.rs:618-620
            return self._plain(op, left, right.value)
        if left.is_trivial:  # mod.rs:621-623
            return self._plain(op, right, left.value)
        return self.gates(np.full(left.count, op, dtype=np.uint8), left, right)

    def and_(self, left, right) -> BoolBatch:
        return self._binary(AND, left, right)

    def nand(self, left, right) -> BoolBatch:
        return self._binary(NAND, left, right)

    def nor(self, left, right) -> BoolBatch:
        return self._binary(NOR, left, right)

    def or_(self, left, right) -> BoolBatch:
        return self._binary(OR, left, right)

    def xor(self, left, right) -> BoolBatch:
        return self._binary(XOR, left, right)

    def xnor(self, left, right) -> BoolBatch:
        return self._binary(XNOR, left, right)

    # -- MUX (mod.rs:461-569) ---------------------------------------------------------------------------
    def mux(self, cond, then_, else_) -> BoolBatch:
        batches = [x for x in (cond, then_, else_) if isinstance(x, BoolBatch)]
        if not batches:
            raise TypeError("at least one operand must be a BoolBatch")
        count = batches[0].count
        cond, then_, else_ = (x if isinstance(x, BoolBatch) else BoolBatch.trivial(bool(x), count)
                              for x in (cond, then_, else_))
        if not (cond.count == then_.count == else_.count):
            raise ValueError("operands of different batch sizes")
        if cond.is_trivial:  # mod.rs:472-478
            return then_.clone() if cond.value else else_.clone()
        if then_.is_trivial:  # mod.rs:483-490
            return self.or_(cond, else_) if then_.value else self.and_(self.not_(cond), else_)
        if else_.is_trivial:  # mod.rs:493-500
            return self.or_(then_, self.not_(cond)) if else_.value else self.and_(cond, then_)
        return self._mux_encrypted(cond, self.to_lwe(then_), self.to_lwe(else_))

    def to_lwe(self, ct: BoolBatch) -> BoolBatch:
        """convert_into_lwe_ciphertext_32 (mod.rs:573-605): an encrypted batch as it is; a trivial one as
        trivial LWE encryptions (zero mask, body T or F) of the size the pbs order takes as input."""
        if not ct.is_trivial:
            return ct
        rows = np.zeros((ct.count, self.parameters.ciphertext_words), dtype=np.uint32)
        rows[:, -1] = PLAINTEXT_TRUE if ct.value else PLAINTEXT_FALSE
        return BoolBatch(rows)


def gen_keys(parameters: BooleanParameters = DEFAULT_PARAMETERS, seed: int = 0, device=0):
    """(ClientKey, ServerKey) of a parameter set.  `device`: a GPU ordinal (a tfhe_mi355.Engine is created
    there), or an engine object of its own with upload_bootstrap_key_u32 / upload_keyswitch_key_u32.

    The u32 key material is the u64 generators' output rounded to its top 32 bits, (x + 2^31) >> 32: a
    uniform error of at most 2^-33 per word on top of the key's Gaussian noise, below every set's noise
    (ClientKey.server_key_material)."""
    cks = ClientKey(parameters, seed)
    if hasattr(device, "upload_bootstrap_key_u32"):
        engine = device
    else:
        from .engine import Engine

        engine = Engine(parameters, int(device))
    bsk, ksk = cks.server_key_material()
    engine.upload_bootstrap_key_u32(bsk)
    engine.upload_keyswitch_key_u32(ksk)
    return cks, ServerKey(engine, parameters)
