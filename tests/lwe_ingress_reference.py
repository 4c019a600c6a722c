"""numpy restatement of the compressed ciphertext expansions (tests/test_lwe_ingress*.py).

  expand_compact   expand_lwe_compact_ciphertext_list (core_crypto/algorithms/
                   lwe_compact_ciphertext_list_expansion.rs:12-58): the container is [mask_count][n] masks then
                   [count] bodies, mask_count = ceil(count / n); row i of bin b = i // n, t = i % n takes the bin's
                   mask times X^(n - (t + 1)) in Z[X]/(X^n + 1) -- polynomial_wrapping_monic_monomial_mul_assign
                   (polynomial_algorithms.rs:261-282): rotate right by the degree, negate the words that wrapped.
  seeded_list      decompress_seeded_lwe_ciphertext_list: mask word j of row r is word r n + j of the seed's stream.
  seeded_rows      decompress_seeded_lwe_ciphertext per row: mask word j of row r is word j of ITS seed's stream.
The stream itself is the oracle's (oracle/csprng_oracle.c through oracle.seeded_mask_words).
"""
import numpy as np

U64 = np.uint64


def compact_words(n: int, count: int) -> int:
    """lwe_compact_ciphertext_list_size (entities/lwe_compact_ciphertext_list.rs:55-63)"""
    return -(-count // n) * n + count


def monic_monomial_mul(poly: np.ndarray, degree: int) -> np.ndarray:
    """poly * X^degree in Z[X]/(X^n + 1), 0 <= degree < n"""
    out = np.roll(poly, degree)
    out[:degree] = U64(0) - out[:degree]
    return out


def expand_compact(container, n: int, count: int) -> np.ndarray:
    c = np.ascontiguousarray(container, dtype=U64).ravel()
    assert c.size == compact_words(n, count)
    bins = -(-count // n)
    masks, bodies = c[:bins * n].reshape(bins, n), c[bins * n:]
    out = np.empty((count, n + 1), dtype=U64)
    for i in range(count):
        out[i, :n] = monic_monomial_mul(masks[i // n], n - (i % n + 1))
        out[i, n] = bodies[i]
    return out


def seeded_list(orc, seed: int, bodies, n: int) -> np.ndarray:
    b = np.ascontiguousarray(bodies, dtype=U64).ravel()
    out = np.empty((b.size, n + 1), dtype=U64)
    out[:, :n] = orc.seeded_mask_words(seed, 0, b.size * n).reshape(b.size, n)
    out[:, n] = b
    return out


def seeded_rows(orc, seeds, bodies, n: int) -> np.ndarray:
    b = np.ascontiguousarray(bodies, dtype=U64).ravel()
    out = np.empty((b.size, n + 1), dtype=U64)
    cache = {}
    for r, s in enumerate(seeds):
        if s not in cache:
            cache[s] = orc.seeded_mask_words(int(s), 0, n)
        out[r, :n] = cache[s]
    out[:, n] = b
    return out
