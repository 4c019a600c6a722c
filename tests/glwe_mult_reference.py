"""CPU reference of the fork's GLWE product with relinearisation ("even transistor": glwe_mult,
lwe_mult, woppbs_lut) built from the oracle alone (oracle/ stays as it is); shared by test_glwe_mult.py
and test_glwe_mult_gpu.py.

  glwe_mult       custom_glwe_glwe_product.rs:13-321: shift by 32 - log_p/2, tensor product, relinearisation
  relin. key      custom_relinearization_key_generation.rs:72-161, [k(k+1)/2][L][(k+1)N], level L first
  lwe_mult        gadget/engine/mod.rs:680-751: packing keyswitch of both LWEs, glwe_mult, extraction
  woppbs_lut      gadget/engine/mod.rs:755-802 (RefEngine runs gadget.ServerKey's chain on the CPU)

Every polynomial product goes through O.glwe_poly_mul, the oracle's exact negacyclic product over
Z/2^64 (test_glwe_mult.py checks it against a schoolbook product); the decomposer is restated in numpy
and pinned by the reference's known answers.
"""
import numpy as np

from oracle.oracle import OracleEngine

U64 = np.uint64


# ---- block order -------------------------------------------------------------------------------
def block_index(i: int, j: int) -> int:
    """Block of the key polynomials' product S_i S_j, j <= i (custom_glwe_glwe_product.rs:280-289)."""
    assert 0 <= j <= i
    return i * (i + 1) // 2 + j


def block_pairs(k: int) -> list:
    """(i, j) of blocks 0 .. k(k+1)/2 - 1, found as the reference finds them: i is the root of the
    greatest triangular number <= n."""
    tri = [i * (i + 1) // 2 for i in range(k + 1)]
    out = []
    for n in range(k * (k + 1) // 2):
        i = 0
        while tri[i] <= n:
            i += 1
        i = max(1, i) - 1
        out.append((i, n - tri[i]))
    return out


# ---- SignedDecomposer in numpy (decomposer.rs:99-119, iter.rs:134-141) ----------------------------
def closest_representable(x, base_log: int, level: int) -> np.ndarray:
    x = np.atleast_1d(np.asarray(x, dtype=U64))  # arrays wrap silently, as the reference's u64 does
    shift = U64(64 - base_log * level - 1)
    res = (x >> shift) + U64(1)
    res &= ~U64(1)
    return res << shift


def decompose(x, base_log: int, level: int) -> np.ndarray:
    """Balanced digits of closest_representable(x) as int64, [level] + x.shape (a scalar counts as one
    element), level L first (the order the reference's iterator yields them)."""
    beta = U64(base_log)
    state = closest_representable(x, base_log, level) >> U64(64 - base_log * level)
    mask = U64((1 << base_log) - 1)
    out = np.empty((level,) + state.shape, dtype=np.int64)
    for l in range(level):
        res = state & mask
        state = state >> beta
        carry = ((res - U64(1)) | state) & res
        carry >>= U64(base_log - 1)
        state = state + carry
        out[l] = (res - (carry << beta)).view(np.int64)
    return out


# ---- products ---------------------------------------------------------------------------------
def poly_mul(O, a, b) -> np.ndarray:
    """Exact negacyclic product of two polynomials over Z/2^64."""
    N = len(a)
    a2 = np.concatenate([np.asarray(a, dtype=U64), np.zeros(N, dtype=U64)])  # a "GLWE" of k = 1
    return O.glwe_poly_mul(1, N, a2[None, None, :], np.asarray(b, dtype=U64)[None, None, :], False)[0, 0, :N]


def sample_extract(glwe, k: int, N: int) -> np.ndarray:
    """extract_lwe_sample_from_glwe_ciphertext at degree 0: [count][(k+1)N] -> [count][kN+1]."""
    g = np.asarray(glwe, dtype=U64).reshape(-1, k + 1, N)
    out = np.empty((g.shape[0], k * N + 1), dtype=U64)
    for p in range(k):
        out[:, p * N] = g[:, p, 0]
        out[:, p * N + 1:(p + 1) * N] = U64(0) - g[:, p, :0:-1]
    out[:, k * N] = g[:, k, 0]
    return out


def tensor_product(O, lhs, rhs, k: int, N: int, log_p: int):
    """Modulus switch and tensor product: (out [count][(k+1)N] holding mask_i = A_i B' + A'_i B and
    body = B B', tr [count][k(k+1)/2][N] holding T_i / R_ij in block order)."""
    assert log_p % 2 == 0 and 0 <= log_p <= 64
    glwe = (k + 1) * N
    shift = U64(32 - log_p // 2)
    A = np.asarray(lhs, dtype=U64).reshape(-1, glwe) >> shift
    B = np.asarray(rhs, dtype=U64).reshape(-1, glwe) >> shift
    count = A.shape[0]
    out = np.zeros((count, k + 1, N), dtype=U64)
    tr = np.zeros((count, k * (k + 1) // 2, N), dtype=U64)
    for c in range(count):
        # P[y][x] = lhs polynomial x times rhs polynomial y
        P = O.glwe_poly_mul(k, N, A[c][None, None, :], B[c].reshape(k + 1, 1, N), False)[0].reshape(k + 1, k + 1, N)
        for i in range(k):
            out[c, i] = P[k][i] + P[i][k]
            tr[c, block_index(i, i)] = P[i][i]
            for j in range(i):
                tr[c, block_index(i, j)] = P[j][i] + P[i][j]
        out[c, k] = P[k][k]
    return out.reshape(count, glwe), tr


def relinearise(O, out, tr, rlk, k: int, N: int, base_log: int, level: int) -> np.ndarray:
    """out_q += sum_n sum_l digit_l(tr[n]) * rlk[n][l][q], digit 0 = level L = the block's first GLWE."""
    glwe = (k + 1) * N
    nblk = k * (k + 1) // 2
    count = tr.shape[0]
    key = np.asarray(rlk, dtype=U64).reshape(1, nblk * level, glwe)
    digits = decompose(tr, base_log, level)                       # [level][count][nblk][N]
    polys = np.ascontiguousarray(digits.transpose(1, 2, 0, 3)).view(U64).reshape(count, nblk * level, N)
    return np.asarray(out, dtype=U64).reshape(count, glwe) + O.glwe_poly_mul(k, N, key, polys, False)[0]


def glwe_mult(O, lhs, rhs, rlk, k: int, N: int, base_log: int, level: int, log_p: int, extract=False) -> np.ndarray:
    out, tr = tensor_product(O, lhs, rhs, k, N, log_p)
    res = relinearise(O, out, tr, rlk, k, N, base_log, level)
    return sample_extract(res, k, N) if extract else res


def lwe_mult(O, lhs, rhs, pksk, pks, rlk, rl, k: int, N: int, log_p: int) -> np.ndarray:
    """pks, rl: (base_log, level) of the packing and relinearisation keys."""
    a = np.asarray(lhs, dtype=U64).reshape(-1, k * N + 1)
    b = np.asarray(rhs, dtype=U64).reshape(-1, k * N + 1)
    packed = O.packing_keyswitch(pksk, k * N, k, N, pks[0], pks[1], np.concatenate([a, b]))
    return glwe_mult(O, packed[:len(a)], packed[len(a):], rlk, k, N, rl[0], rl[1], log_p, extract=True)


# ---- keys ---------------------------------------------------------------------------------------
def glwe_phase(O, glwe_sk, ct, k: int, N: int) -> np.ndarray:
    """body - sum_i mask_i S_i of one GLWE."""
    ct = np.asarray(ct, dtype=U64).reshape(k + 1, N)
    S = np.asarray(glwe_sk, dtype=U64).reshape(k, N)
    ph = ct[k].copy()
    for i in range(k):
        ph -= poly_mul(O, ct[i], S[i])
    return ph


def gen_relinearization_key(O, rng, glwe_sk, k: int, N: int, base_log: int, level: int, std: float) -> np.ndarray:
    """[k(k+1)/2][level][(k+1)N] with numpy's randomness: uniform masks, rounded Gaussian noise."""
    S = np.asarray(glwe_sk, dtype=U64).reshape(k, N)
    out = np.zeros((k * (k + 1) // 2, level, k + 1, N), dtype=U64)
    for n, (i, j) in enumerate(block_pairs(k)):
        prod = poly_mul(O, S[i], S[j])
        for l in range(level):
            g = out[n, l]
            g[:k] = rng.integers(0, 1 << 64, (k, N), dtype=U64)
            noise = np.rint(rng.normal(0.0, std, N) * 2.0 ** 64).astype(np.int64).view(U64)
            g[k] = (prod << U64(64 - base_log * (level - l))) + noise
            for q in range(k):
                g[k] += poly_mul(O, g[q], S[q])
    return out.reshape(k * (k + 1) // 2, level, (k + 1) * N)


def torus_distance(a, b) -> np.ndarray:
    d = (np.asarray(a, dtype=U64) - np.asarray(b, dtype=U64)).view(np.int64)
    return np.abs(d.astype(np.float64))


# ---- the engine behind gadget.ServerKey, on the CPU ---------------------------------------------------
class RefEngine(OracleEngine):
    """OracleEngine plus the relinearisation key and the two products, so that
    gadget.ServerKey(ck, engine=RefEngine(P)) runs lwe_mult and woppbs_lut on the CPU."""

    def upload_relinearization_key(self, rlk, base_log, level):
        self.rlk, self.rl = np.ascontiguousarray(rlk, dtype=U64), (base_log, level)

    def glwe_mult(self, lhs, rhs, log_p, extract=False):
        p = self.p
        return glwe_mult(self.O, lhs, rhs, self.rlk, p.glwe_dimension, p.polynomial_size, self.rl[0], self.rl[1],
                         log_p, extract)

    def lwe_mult(self, lhs, rhs, log_p):
        p = self.p
        return lwe_mult(self.O, lhs, rhs, self.pksk, self.pks, self.rlk, self.rl, p.glwe_dimension,
                        p.polynomial_size, log_p)


# ---- test-only parameter sets -----------------------------------------------------------------------
# The fork's gadget sets keyswitch with 12 bits (SHA3_40: 4 x 3, AES_23: 3 x 4), too few for the
# relinearisation: the product then decrypts wrong for most message pairs.  These sets keep a shipped
# shape and noise and take a 24-bit keyswitch decomposition (the keyswitch kernels accept base_log <= 7).
# The default shape also takes the SHA3 set's GLWE noise (2^-60): the product multiplies each packed
# GLWE's noise, shifted down by 32 - log_p/2, with the other's UNREDUCED integer phase (about
# kN/4 * 2^(32 + log_p/2), the sum of kN/2 shifted mask words), so the default set's own 2^-24.3 leaves
# 2^39.7 * 2^10.2 (packing) / 2^31 * 2^41 = 2^60 of noise at p = 4 and 10 of 16 pairs decrypt wrong.
# They are insecure and exist for these tests only.
def mult_sets():
    from tfhe_mi355 import parameters as P

    return {
        "sha3": P.GADGET_SHA3_PARAMETERS_40.with_(ks_base_log=6, ks_level=4, name="TEST_MULT_SHA3_5_256"),
        "default": P.GADGET_DEFAULT_PARAMETERS.with_(ks_base_log=6, ks_level=4, encryption_key_choice="Big",
                                                     glwe_modular_std_dev=P.GADGET_SHA3_PARAMETERS_40.glwe_modular_std_dev,
                                                     name="TEST_MULT_DEFAULT_2_512"),
        "aes23": P.GADGET_AES_PARAMETERS_23.with_(pbs_base_log=7, pbs_level=4, ks_base_log=6, ks_level=4,
                                                  name="TEST_MULT_AES23_3_512"),
    }


# ---- woppbs_lut in the clear ----------------------------------------------------------------------
def woppbs_lut_clear(x: int, enc_in, enc_out, f) -> int:
    """What the chain of woppbs_lut decrypts to for the message x, from its three rules.

    Accumulator: the wopbs accumulator holds p windows of N/p coefficients on HALF the torus, window w
    carrying the output value of the message whose input part contains w (0 when none does).
    Negacyclic wrap: the blind rotation of an input at zp 2^64/p lands on coefficient 2 zp N/p, the
    middle of window 2 zp for 2 zp < p; for 2 zp >= p it has gone once round X^N = -1 and reads
    MINUS window 2 zp - p.  Product: ct_f carries s data_f[w], ct_ones carries s 1 with the same sign
    s, and lwe_mult multiplies the two messages mod p, so the sign cancels."""
    p = enc_in.get_modulus()
    zp = enc_in.get_part_single_value_if_canonical(x)
    w, sign = (2 * zp) % p, (-1 if 2 * zp >= p else 1)
    enc_inter = enc_in.apply_lut_to_encoding(f)

    def window(enc_from, enc_to, w):
        i = enc_from.inverse_encoding(w)
        return enc_to.get_part_single_value_if_canonical(i) if i is not None else 0

    enc_ones = type(enc_in).new_all_one_wopbs(enc_in.get_origin_modulus())
    m_f = sign * window(enc_inter, enc_out, w) % enc_out.get_modulus()
    m_one = sign * window(enc_in, enc_ones, w) % enc_ones.get_modulus()
    return enc_out.inverse_encoding(m_f * m_one % enc_out.get_modulus())
