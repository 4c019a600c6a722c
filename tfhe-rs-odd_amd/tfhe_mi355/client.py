"""Client-side helpers (key generation, LWE encryption/decryption) through the C ABI.

They follow the reference's rules (binary keys, Marsaglia-polar Gaussian noise, GGSW rows of
ggsw_encryption.rs:116-150, KSK levels L..1 of lwe_keyswitch_key_generation.rs:109) with a seeded
xoshiro256** stream instead of the reference's AES-CTR CSPRNG.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from ._lib import u64p


def _ptr(a):
    return a.ctypes.data_as(u64p)


def gen_binary_key(seed: int, stream: int, length: int) -> np.ndarray:
    k = np.zeros(length, dtype=np.uint64)
    _lib.call("tfhe_mi355_client_gen_binary_key", seed, stream, _ptr(k), length)
    return k


def gen_bootstrap_key(seed, lwe_sk, glwe_sk, glwe_dimension, polynomial_size, base_log, level, std_dev,
                      threads: int = 0) -> np.ndarray:
    lwe_sk = np.ascontiguousarray(lwe_sk, dtype=np.uint64)
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N = glwe_dimension, polynomial_size
    bsk = np.empty(len(lwe_sk) * level * (k + 1) * (k + 1) * N, dtype=np.uint64)
    if threads <= 0:
        threads = min(16, os.cpu_count() or 1)
    _lib.call("tfhe_mi355_client_gen_bootstrap_key", seed, _ptr(lwe_sk), len(lwe_sk), _ptr(glwe_sk), k, N,
              base_log, level, std_dev, _ptr(bsk), threads)
    return bsk


def gen_ggsw_list(seed, bits, glwe_sk, glwe_dimension, polynomial_size, base_log, level, std_dev,
                  threads: int = 0) -> np.ndarray:
    """GGSW encryptions of the constant polynomials `bits[i]`, [len(bits)][level][k+1][(k+1)N]
    (encrypt_constant_ggsw_ciphertext, ggsw_encryption.rs:116-150), levels stored 1..L.

    A bootstrap key is exactly that list for the bits of an LWE key (lwe_bootstrap_key_generation.rs:
    one constant GGSW per key bit), so this is gen_bootstrap_key with `bits` in the LWE key's place;
    any decomposition may be asked for, e.g. the circuit-bootstrap one of the WoP-PBS sets."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64).ravel()
    k, N = glwe_dimension, polynomial_size
    out = gen_bootstrap_key(seed, bits, glwe_sk, k, N, base_log, level, std_dev, threads)
    return out.reshape(len(bits), level, k + 1, (k + 1) * N)


def gen_multi_bit_bootstrap_key(seed, lwe_sk, glwe_sk, glwe_dimension, polynomial_size, base_log, level,
                                grouping_factor, std_dev, threads: int = 0) -> np.ndarray:
    """[n/g][2^g][L][k+1][k+1][N] (lwe_multi_bit_bootstrap_key_generation.rs:87-173)."""
    lwe_sk = np.ascontiguousarray(lwe_sk, dtype=np.uint64)
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N, g = glwe_dimension, polynomial_size, grouping_factor
    bsk = np.empty((len(lwe_sk) // g) * (1 << g) * level * (k + 1) * (k + 1) * N, dtype=np.uint64)
    if threads <= 0:
        threads = min(16, os.cpu_count() or 1)
    _lib.call("tfhe_mi355_client_gen_multi_bit_bootstrap_key", seed, _ptr(lwe_sk), len(lwe_sk), _ptr(glwe_sk),
              k, N, base_log, level, g, std_dev, _ptr(bsk), threads)
    return bsk


def gen_keyswitch_key(seed, in_sk, out_sk, base_log, level, std_dev) -> np.ndarray:
    in_sk = np.ascontiguousarray(in_sk, dtype=np.uint64)
    out_sk = np.ascontiguousarray(out_sk, dtype=np.uint64)
    ksk = np.empty(len(in_sk) * level * (len(out_sk) + 1), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_gen_keyswitch_key", seed, _ptr(in_sk), len(in_sk), _ptr(out_sk), len(out_sk),
              base_log, level, std_dev, _ptr(ksk))
    return ksk


def gen_packing_keyswitch_key(seed, in_sk, glwe_sk, glwe_dimension, polynomial_size, base_log, level, std_dev,
                              threads: int = 0) -> np.ndarray:
    """LWE -> GLWE packing KSK [in][level][(k+1)N] (lwe_packing_keyswitch_key_generation.rs:74-149)."""
    in_sk = np.ascontiguousarray(in_sk, dtype=np.uint64)
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N = glwe_dimension, polynomial_size
    out = np.empty(len(in_sk) * level * (k + 1) * N, dtype=np.uint64)
    _lib.call("tfhe_mi355_client_gen_packing_keyswitch_key", seed, _ptr(in_sk), len(in_sk), _ptr(glwe_sk), k, N,
              base_log, level, std_dev, _ptr(out), threads)
    return out


def gen_pfpksk_list(seed, in_sk, glwe_sk, glwe_dimension, polynomial_size, base_log, level, std_dev,
                    threads: int = 0) -> np.ndarray:
    """Private functional packing keyswitching keys of the circuit bootstrap
    [k+1][in+1][level][(k+1)N], level 1 first (lwe_wopbs.rs:80-158)."""
    in_sk = np.ascontiguousarray(in_sk, dtype=np.uint64)
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N = glwe_dimension, polynomial_size
    out = np.empty((k + 1) * (len(in_sk) + 1) * level * (k + 1) * N, dtype=np.uint64)
    if threads <= 0:
        threads = min(16, os.cpu_count() or 1)
    _lib.call("tfhe_mi355_client_gen_pfpksk_list", seed, _ptr(in_sk), len(in_sk), _ptr(glwe_sk), k, N, base_log,
              level, std_dev, _ptr(out), threads)
    return out


def gen_relinearization_key(seed, glwe_sk, glwe_dimension, polynomial_size, base_log, level, std_dev) -> np.ndarray:
    """GLWE relinearisation key of lwe_mult [k(k+1)/2][level][(k+1)N], level L first: block i(i+1)/2 + j
    (j <= i) encrypts (S_i * S_j) << (64 - base_log*lvl) (custom_relinearization_key_generation.rs:72-161)."""
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N = glwe_dimension, polynomial_size
    out = np.empty((k * (k + 1) // 2, level, (k + 1) * N), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_gen_relinearization_key", seed, _ptr(glwe_sk), k, N, base_log, level, std_dev,
              _ptr(out))
    return out


def _seed_parts(seed: int):
    return seed & 0xFFFFFFFFFFFFFFFF, (seed >> 64) & 0xFFFFFFFFFFFFFFFF


def csprng_mask_words(compression_seed: int, first_word: int, count: int) -> np.ndarray:
    """Mask words of a seeded key: word w = LE u64 of AES-CTR stream bytes [1 + 8w, 9 + 8w)."""
    out = np.empty(count, dtype=np.uint64)
    lo, hi = _seed_parts(compression_seed)
    _lib.call("tfhe_mi355_client_csprng_mask_words", lo, hi, first_word, count, _ptr(out))
    return out


def gen_seeded_bootstrap_key(noise_seed, compression_seed: int, lwe_sk, glwe_sk, glwe_dimension, polynomial_size,
                             base_log, level, std_dev, threads: int = 0) -> np.ndarray:
    """SeededLweBootstrapKey bodies [n][L][k+1][N]; masks = the AES-CTR stream of compression_seed."""
    lwe_sk = np.ascontiguousarray(lwe_sk, dtype=np.uint64)
    glwe_sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    k, N = glwe_dimension, polynomial_size
    out = np.empty(len(lwe_sk) * level * (k + 1) * N, dtype=np.uint64)
    lo, hi = _seed_parts(compression_seed)
    _lib.call("tfhe_mi355_client_gen_seeded_bootstrap_key", noise_seed, lo, hi, _ptr(lwe_sk), len(lwe_sk),
              _ptr(glwe_sk), k, N, base_log, level, std_dev, _ptr(out), threads)
    return out


def gen_seeded_keyswitch_key(noise_seed, compression_seed: int, in_sk, out_sk, base_log, level,
                             std_dev) -> np.ndarray:
    """SeededLweKeyswitchKey bodies [in_dim][L]."""
    in_sk = np.ascontiguousarray(in_sk, dtype=np.uint64)
    out_sk = np.ascontiguousarray(out_sk, dtype=np.uint64)
    out = np.empty(len(in_sk) * level, dtype=np.uint64)
    lo, hi = _seed_parts(compression_seed)
    _lib.call("tfhe_mi355_client_gen_seeded_keyswitch_key", noise_seed, lo, hi, _ptr(in_sk), len(in_sk),
              _ptr(out_sk), len(out_sk), base_log, level, std_dev, _ptr(out))
    return out


def lwe_encrypt(seed, sk, plaintexts, std_dev) -> np.ndarray:
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    pts = np.ascontiguousarray(plaintexts, dtype=np.uint64).ravel()
    cts = np.empty((len(pts), len(sk) + 1), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_lwe_encrypt", seed, _ptr(sk), len(sk), _ptr(pts), len(pts), std_dev, _ptr(cts))
    return cts


def lwe_decrypt(sk, cts) -> np.ndarray:
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, len(sk) + 1)
    pts = np.empty(cts.shape[0], dtype=np.uint64)
    _lib.call("tfhe_mi355_client_lwe_decrypt", _ptr(sk), len(sk), _ptr(cts), cts.shape[0], _ptr(pts))
    return pts


# ---- compressed ciphertext forms (compact public key, seeded ciphertexts) ----------------------------
def _seed_words(seeds) -> np.ndarray:
    """[count][2] = {lo, hi} words of 128-bit seeds given as Python ints"""
    return np.array([[int(s) & 0xFFFFFFFFFFFFFFFF, (int(s) >> 64) & 0xFFFFFFFFFFFFFFFF] for s in seeds],
                    dtype=np.uint64).reshape(-1, 2)


def gen_compact_public_key(seed, sk, std_dev) -> np.ndarray:
    """[2n] = mask, body (generate_lwe_compact_public_key, lwe_compact_public_key_generation.rs:15-54); n a
    power of two."""
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    pk = np.empty(2 * len(sk), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_gen_compact_public_key", seed, _ptr(sk), len(sk), std_dev, _ptr(pk))
    return pk


def compact_list_words(lwe_dimension: int, count: int) -> int:
    """lwe_compact_ciphertext_list_size (entities/lwe_compact_ciphertext_list.rs:55-63)"""
    return -(-count // lwe_dimension) * lwe_dimension + count


def compact_encrypt(seed, pk, plaintexts, mask_std_dev, body_std_dev=None) -> np.ndarray:
    """The container of an LweCompactCiphertextList, [ceil(count / n)][n] masks then [count] bodies
    (encrypt_lwe_compact_ciphertext_list_with_compact_public_key, lwe_encryption.rs:1837-2043)."""
    pk = np.ascontiguousarray(pk, dtype=np.uint64)
    n = len(pk) // 2
    pts = np.ascontiguousarray(plaintexts, dtype=np.uint64).ravel()
    out = np.empty(compact_list_words(n, len(pts)), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_compact_encrypt", seed, _ptr(pk), n, _ptr(pts), len(pts), mask_std_dev,
              mask_std_dev if body_std_dev is None else body_std_dev, _ptr(out))
    return out


def seeded_lwe_encrypt(noise_seed, seeds, sk, plaintexts, std_dev) -> np.ndarray:
    """Bodies of seeded ciphertexts, one 128-bit CompressionSeed each (encrypt_seeded_lwe_ciphertext,
    lwe_encryption.rs:1415-1585): the mask of ciphertext c is words [0, n) of the stream of seeds[c]."""
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    pts = np.ascontiguousarray(plaintexts, dtype=np.uint64).ravel()
    sw = _seed_words(seeds)
    if len(sw) != len(pts):
        raise ValueError("one seed per plaintext")
    bodies = np.empty(len(pts), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_seeded_lwe_encrypt", noise_seed, _ptr(sw), _ptr(sk), len(sk), _ptr(pts), len(pts),
              std_dev, _ptr(bodies))
    return bodies


def seeded_lwe_encrypt_list(noise_seed, compression_seed: int, sk, plaintexts, std_dev) -> np.ndarray:
    """Bodies of a seeded list under one seed (encrypt_seeded_lwe_ciphertext_list, lwe_encryption.rs:1096-1253):
    ciphertext c takes mask words [c n, (c + 1) n) of the stream."""
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    pts = np.ascontiguousarray(plaintexts, dtype=np.uint64).ravel()
    bodies = np.empty(len(pts), dtype=np.uint64)
    _lib.call("tfhe_mi355_client_seeded_lwe_encrypt_list", noise_seed, compression_seed & 0xFFFFFFFFFFFFFFFF,
              (compression_seed >> 64) & 0xFFFFFFFFFFFFFFFF, _ptr(sk), len(sk), _ptr(pts), len(pts), std_dev,
              _ptr(bodies))
    return bodies


def decode(plaintexts, delta: int) -> np.ndarray:
    """shortint decrypt_message_and_carry rounding (shortint/client_key/mod.rs:281-302)."""
    d = np.asarray(plaintexts, dtype=np.uint64)
    rb = np.uint64(delta >> 1)
    rounding = (d & rb) << np.uint64(1)
    return (d + rounding) // np.uint64(delta)


# ---- 32-bit torus (boolean module) -------------------------------------------------------------------
def round_to_u32(words64) -> np.ndarray:
    """The top 32 bits of u64 torus words, rounded: (x + 2^31) >> 32 mod 2^32.  The boolean helpers
    derive u32 keys and ciphertexts from the u64 generators this way; the rounding adds a uniform
    error of at most 2^-33 to each word, below every boolean set's noise (>= 2^-30)."""
    x = np.ascontiguousarray(words64, dtype=np.uint64)
    return ((x + np.uint64(1 << 31)) >> np.uint64(32)).astype(np.uint32)


def lwe_encrypt_u32(seed, sk, plaintexts32, std_dev) -> np.ndarray:
    """u32 LWE encryptions [count][len(sk)+1] of u32 plaintexts (u64 encryption of pt << 32, rounded)."""
    pts = np.ascontiguousarray(plaintexts32, dtype=np.uint64).ravel() << np.uint64(32)
    return round_to_u32(lwe_encrypt(seed, sk, pts, std_dev))


def lwe_decrypt_u32(sk, cts32) -> np.ndarray:
    """Phases body - <mask, sk> mod 2^32 of u32 LWE ciphertexts."""
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    c = np.ascontiguousarray(cts32, dtype=np.uint32).reshape(-1, len(sk) + 1).astype(np.uint64)
    dot = (c[:, :-1] * sk[None, :]).sum(axis=1, dtype=np.uint64)
    return ((c[:, -1] - dot) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
