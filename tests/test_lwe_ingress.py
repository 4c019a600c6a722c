"""Compressed ciphertext ingress, the parts that need no GPU: the numpy restatement of the compact expansion
(tests/lwe_ingress_reference.py), the client-side compact and seeded encryption, the two bincode readers of
csrc/serde.cpp, and the bookkeeping of the compact-public-key parameter sets."""
import json
import os

import numpy as np
import pytest

import lwe_ingress_reference as R
from conftest import ROOT, decode

U64 = np.uint64
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- 1. the restatement's algebra --------------------------------------------------------------------------
def _masks(seed, *shape):
    m = np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=U64)
    m.reshape(-1)[:2] = [0, 1 << 63]  # the fixed points of negation
    return m


@pytest.mark.parametrize("n", [8, 256])
def test_last_row_of_a_bin_keeps_the_mask_and_first_row_shifts_it_by_n_minus_one(n):
    box = np.concatenate([_masks(n, n), np.arange(n, dtype=U64) + U64(100)])
    rows = R.expand_compact(box, n, n)
    mask = box[:n]
    assert np.array_equal(rows[n - 1, :n], mask)                      # t = n - 1: X^0
    assert np.array_equal(rows[0, :n - 1], U64(0) - mask[1:])         # t = 0: out[j] = -mask[j + 1], j < n - 1
    assert rows[0, n - 1] == mask[0]                                  #        out[n - 1] = mask[0]
    assert np.array_equal(rows[:, n], box[n:])
    for t in (1, n // 2):  # the issue's formula, word for word
        d = n - (t + 1)
        want = np.concatenate([U64(0) - mask[n - d:], mask[:n - d]])
        assert np.array_equal(rows[t, :n], want)


def test_compact_encryption_decrypts_after_cpu_expansion():
    """compact-encrypt known messages with the client code, expand on the CPU, decrypt: the expansion composed
    with the negacyclic products of the public key reproduces <mask_i, s> (bins: full, full, partial)"""
    from tfhe_mi355 import client

    n, count, delta, std = 256, 2 * 256 + 3, 1 << 59, 2.0 ** -40
    sk = client.gen_binary_key(3, 1, n)
    pk = client.gen_compact_public_key(4, sk, std)
    msgs = (np.arange(count, dtype=U64) * U64(7)) % U64(16)
    box = client.compact_encrypt(5, pk, msgs * U64(delta), std)
    assert box.size == R.compact_words(n, count) == client.compact_list_words(n, count)
    rows = R.expand_compact(box, n, count)
    assert np.array_equal(decode(client.lwe_decrypt(sk, rows), delta) % 16, msgs)
    # the error is small: binary r against two noise polynomials, far below delta / 2
    err = (client.lwe_decrypt(sk, rows) - msgs * U64(delta)).astype(np.int64)
    assert np.abs(err).max() < 1 << 40


def test_compact_encryption_at_a_large_dimension_uses_the_exact_fft_product():
    from tfhe_mi355 import client

    n, delta, std = 4096, 1 << 59, 2.0 ** -50
    sk = client.gen_binary_key(6, 1, n)
    pk = client.gen_compact_public_key(7, sk, std)
    msgs = np.array([0, 5, 15], dtype=U64)
    rows = R.expand_compact(client.compact_encrypt(8, pk, msgs * U64(delta), std), n, 3)
    assert np.array_equal(decode(client.lwe_decrypt(sk, rows), delta) % 16, msgs)


def test_seeded_encryptions_use_the_oracle_stream(orc):
    from tfhe_mi355 import client

    n, delta, std = 7, 1 << 59, 2.0 ** -40
    sk = client.gen_binary_key(9, 1, n)
    msgs = np.array([1, 2, 3, 15], dtype=U64)
    seeds = [0, (1 << 128) - 1, 5, 5]
    rows = R.seeded_rows(orc, seeds, client.seeded_lwe_encrypt(1, seeds, sk, msgs * U64(delta), std), n)
    assert np.array_equal(decode(client.lwe_decrypt(sk, rows), delta) % 16, msgs)
    assert np.array_equal(rows[2, :n], rows[3, :n])
    seed = 0x0123456789ABCDEF_FEDCBA9876543210
    rows = R.seeded_list(orc, seed, client.seeded_lwe_encrypt_list(2, seed, sk, msgs * U64(delta), std), n)
    assert np.array_equal(decode(client.lwe_decrypt(sk, rows), delta) % 16, msgs)


# ---- 2. serde ----------------------------------------------------------------------------------------------
def _fields(sizes):
    """[(name, first byte)] from [(name, bytes)]"""
    out, at = [], 0
    for name, b in sizes:
        out.append((name, at))
        at += b
    return out, at


def _compact_bytes(n=8, count=19, **kw):
    from tfhe_mi355 import serialization as S

    box = np.arange(R.compact_words(n, count), dtype=U64) * U64(0x9E3779B97F4A7C15)
    args = dict(degree=3, message_modulus=4, carry_modulus=4, pbs_order=1, noise_level=1)
    args.update(kw)
    return S.serialize_compact_ciphertext_list(box, n, count, **args), box


def test_compact_list_round_trip():
    from tfhe_mi355 import serialization as S

    data, box = _compact_bytes()
    i = S.inspect_compact_ciphertext_list(data)
    assert (i.lwe_dimension, i.count, i.degree, i.message_modulus, i.carry_modulus, i.pbs_order, i.noise_level,
            i.seed) == (8, 19, 3, 4, 4, 1, 1, 0)
    assert (i.data_offset, i.data_words) == (8, box.size)
    assert np.array_equal(i.words(data), box)


def test_compressed_ciphertext_round_trip():
    from tfhe_mi355 import serialization as S

    seed = 0x0123456789ABCDEF_FEDCBA9876543210
    data = S.serialize_compressed_ciphertext(0xDEADBEEF12345678, 742, seed, 3, 4, 4, 0, 1)
    i = S.inspect_compressed_ciphertext(data)
    assert (i.lwe_dimension, i.count, i.degree, i.message_modulus, i.carry_modulus, i.pbs_order, i.noise_level,
            i.seed) == (742, 1, 3, 4, 4, 0, 1, seed)
    assert (i.data_offset, i.data_words) == (0, 1) and int(i.words(data)[0]) == 0xDEADBEEF12345678


def _tail():
    return [("degree", 8), ("message_modulus", 8), ("carry_modulus", 8), ("pbs_order", 4), ("noise_level", 8)]


def test_truncated_compact_list_names_the_field():
    from tfhe_mi355 import EngineError
    from tfhe_mi355 import serialization as S

    data, box = _compact_bytes()
    fields, total = _fields([("compact list data", 8 + 8 * box.size), ("lwe_size", 8), ("lwe_ciphertext_count", 8),
                             ("compact ciphertext list", 24)] + _tail())
    assert total == len(data)
    for name, at in fields:
        for cut in (at, at + 1):
            with pytest.raises(EngineError, match="truncated: " + name) as e:
                S.inspect_compact_ciphertext_list(data[:cut])
            assert "byte" in str(e.value)
    with pytest.raises(EngineError, match="trailing"):
        S.inspect_compact_ciphertext_list(data + b"\0")


def test_truncated_compressed_ciphertext_names_the_field():
    from tfhe_mi355 import EngineError
    from tfhe_mi355 import serialization as S

    data = S.serialize_compressed_ciphertext(1, 742, 2, 3, 4, 4, 0, 1)
    fields, total = _fields([("seeded ciphertext body", 8), ("lwe_size", 8), ("compression_seed", 16),
                             ("compressed ciphertext", 24)] + _tail())
    assert total == len(data)
    for name, at in fields:
        for cut in (at, at + 1):
            with pytest.raises(EngineError, match="truncated: " + name):
                S.inspect_compressed_ciphertext(data[:cut])
    with pytest.raises(EngineError, match="trailing"):
        S.inspect_compressed_ciphertext(data + b"\0")


def test_wrong_container_length_and_shape_are_refused():
    import struct

    from tfhe_mi355 import EngineError
    from tfhe_mi355 import serialization as S

    data, box = _compact_bytes(n=8, count=19)
    at_count = 8 + 8 * box.size + 8
    for count in (18, 20, 24, 0, 1 << 63):  # 24 ciphertexts would need the same 3 masks but 24 bodies
        bad = data[:at_count] + struct.pack("<Q", count) + data[at_count + 8:]
        with pytest.raises(EngineError, match="data words"):
            S.inspect_compact_ciphertext_list(bad)
    with pytest.raises(EngineError, match="power of two"):
        S.inspect_compact_ciphertext_list(S.serialize_compact_ciphertext_list(np.zeros(7 + 3, dtype=U64), 7, 3, 3, 4, 4, 0))
    with pytest.raises(EngineError, match="lwe_size"):
        S.inspect_compact_ciphertext_list(data[:at_count - 8] + struct.pack("<Q", 1) + data[at_count:])
    with pytest.raises(EngineError, match="pbs_order"):
        S.inspect_compact_ciphertext_list(_compact_bytes(pbs_order=2)[0])


def test_non_native_modulus_is_refused():
    import struct

    from tfhe_mi355 import EngineError
    from tfhe_mi355 import serialization as S

    data, box = _compact_bytes()
    at_mod = 8 + 8 * box.size + 16
    for mod, bits in ((1 << 63, 64), (0, 32)):
        bad = data[:at_mod] + struct.pack("<QQQ", mod & (2 ** 64 - 1), mod >> 64, bits) + data[at_mod + 24:]
        with pytest.raises(EngineError, match="modulus"):
            S.inspect_compact_ciphertext_list(bad)
    one = S.serialize_compressed_ciphertext(1, 742, 2, 3, 4, 4, 0, 1)
    bad = one[:32] + struct.pack("<QQQ", 1 << 62, 0, 64) + one[56:]
    with pytest.raises(EngineError, match="non-native"):
        S.inspect_compressed_ciphertext(bad)


def test_shortint_types_serialize_and_deserialize():
    from tfhe_mi355 import shortint as SI
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    ck = SI.ClientKey(P.with_(glwe_dimension=1, polynomial_size=256, name="small"), seed=3)
    lst = SI.CompactPublicKey(ck).encrypt_many([0, 1, 2, 3, 1])
    back = SI.CompactCiphertextList.deserialize(lst.serialize())
    assert back.count == 5 and back.lwe_dimension == 256 and back.pbs_order == SI.KEYSWITCH_BOOTSTRAP
    assert np.array_equal(back.container, lst.container)
    assert (back.degree, back.message_modulus, back.carry_modulus, back.noise_level) == (3, 4, 4, 1)
    rows = R.expand_compact(back.container, 256, 5)
    assert np.array_equal(decode(__import__("tfhe_mi355").client.lwe_decrypt(ck.large_lwe_secret_key, rows), P.delta) % 4,
                          [0, 1, 2, 3, 1])
    cts = ck.encrypt_compressed_many([3, 2])
    assert cts[0].seed != cts[1].seed
    for c in cts:
        assert SI.CompressedCiphertext.deserialize(c.serialize()) == c


# ---- 3. parameter bookkeeping --------------------------------------------------------------------------------
def test_every_compact_pk_set_is_accepted_or_refused():
    from tfhe_mi355 import parameters as P

    with open(os.path.join(GOLDEN, "compact_pk_names.json")) as f:
        names = json.load(f)
    assert len(names) == 56 == len(set(names))
    refused = dict(P.COMPACT_PK_REFUSED)
    assert len(refused) == len(P.COMPACT_PK_REFUSED) and all(len(m) > 10 for m in refused.values())
    assert not set(refused) & set(P.COMPACT_PK_ALL)
    assert set(refused) | set(P.COMPACT_PK_ALL) == set(names)
    assert P.COMPACT_PK_NAMES == tuple(names)
    for name, p in P.COMPACT_PK_ALL.items():
        assert getattr(P, name) is p and p.name == name


def test_accepted_compact_pk_sets_hold_the_recorded_values():
    from tfhe_mi355 import parameters as P

    with open(os.path.join(GOLDEN, "compact_pk_params.json")) as f:
        want = json.load(f)
    assert set(want) == set(P.COMPACT_PK_ALL)
    for name, fields in want.items():
        p = P.COMPACT_PK_ALL[name]
        for k, v in fields.items():
            assert getattr(p, k) == v, (name, k)
        assert p.grouping_factor == 0
        enc = p.big_lwe_dimension if p.encryption_key_choice == "Big" else p.lwe_dimension
        assert enc & (enc - 1) == 0, f"{name}: a compact public key needs a power-of-two dimension"
        assert name.endswith("KS_PBS") == (p.encryption_key_choice == "Big")


def test_refusals_are_the_engines_own():
    """the engine refuses an N = 65536 set before it touches a GPU; the keyswitch refusals are checked on the GPU"""
    import ctypes

    from tfhe_mi355 import _lib
    from tfhe_mi355 import parameters as P

    table = {t[0]: t for t in P._COMPACT_PK_TABLE}
    lib = _lib.load()
    for name, msg in P.COMPACT_PK_REFUSED:
        t = table[name]
        if t[4] != 65536:
            assert t[9] > 7 and msg == "launch keyswitch: invalid argument"
            continue
        cp = _lib.TfheMi355Parameters(t[2], t[3], t[4], t[7], t[8], t[9], t[10], t[11], t[12], 0)
        h = _lib.vp()
        assert lib.tfhe_mi355_context_create(ctypes.byref(cp), 0, ctypes.byref(h)) == 1
        assert lib.tfhe_mi355_last_error().decode() == msg
    assert all(p.ks_base_log <= 7 for p in P.COMPACT_PK_ALL.values())
