"""CPU reference of the GGSW operations (external product, CMUX, vertical packing), built from the
oracle's blind rotation alone (oracle/ stays as it is); shared by test_ggsw_ops.py and
test_ggsw_ops_gpu.py.

External product.  G (x) d is what the oracle's blind rotation adds for a ONE-element key and a
rotation by X^N = -1: with the accumulator acc = (0 - d) >> 1, ct1 = X^N acc - acc = -2 acc = d up to
its lowest bit (which never reaches the decomposer for base_log * level <= 62), so
blind_rotate(acc) = acc + G (x) d.

Rotation phase.  The nr rotation steps of vertical packing equal ONE oracle blind rotation under the
key (GGSW list reversed, n = nr) with mask element i = (2N - 2^i) << (64 - log2(2N)) and body 0: the
modulus switch gives 2N - 2^i, i.e. a multiplication by X^(-2^i).

A GGSW is [level][k+1][(k+1)N] u64 with level l at index l-1 (one bootstrap-key element).
"""
import numpy as np

U64 = np.uint64


def ggsw_words(k, N, level):
    return level * (k + 1) * (k + 1) * N


class Ref:
    def __init__(self, O, k, N, base_log, level):
        self.O, self.k, self.N, self.B, self.L = O, k, N, base_log, level
        self.glwe = (k + 1) * N

    # ---- single operations -----------------------------------------------------------------
    def external_product(self, ggsw, d):
        """G (x) d for d [count][(k+1)N] under ONE GGSW."""
        d = np.ascontiguousarray(d, dtype=U64).reshape(-1, self.glwe)
        f = self.O.FourierBsk(np.ascontiguousarray(ggsw, dtype=U64).ravel(), 1, self.k, self.N, self.B, self.L)
        acc = (U64(0) - d) >> U64(1)
        lwe = np.tile(np.array([[1 << 63, 0]], dtype=U64), (d.shape[0], 1))
        out = f.blind_rotate(lwe, acc, lut_idx=np.arange(d.shape[0], dtype=np.uint32))
        return out - acc

    def external_product_batch(self, ggsws, d, idx=None):
        """item i under GGSW idx[i] (None: i)."""
        d = np.ascontiguousarray(d, dtype=U64).reshape(-1, self.glwe)
        g = np.ascontiguousarray(ggsws, dtype=U64).reshape(-1, ggsw_words(self.k, self.N, self.L))
        idx = np.arange(d.shape[0]) if idx is None else np.asarray(idx)
        out = np.empty_like(d)
        for gi in np.unique(idx):
            sel = np.nonzero(idx == gi)[0]
            out[sel] = self.external_product(g[gi], d[sel])
        return out

    def cmux_batch(self, ggsws, ct0, ct1, idx=None):
        ct0 = np.ascontiguousarray(ct0, dtype=U64).reshape(-1, self.glwe)
        ct1 = np.ascontiguousarray(ct1, dtype=U64).reshape(-1, self.glwe)
        return ct0 + self.external_product_batch(ggsws, ct1 - ct0, idx)

    def monomial_div(self, glwe, r):
        """every polynomial of the GLWE(s) divided by X^r (polynomial_wrapping_monic_monomial_div)."""
        p = np.ascontiguousarray(glwe, dtype=U64).reshape(-1, self.N)
        out = np.concatenate([p[:, r:], U64(0) - p[:, :r]], axis=1)
        return out.reshape(np.shape(glwe))

    def sample_extract(self, glwe):
        g = np.ascontiguousarray(glwe, dtype=U64).reshape(-1, self.k + 1, self.N)
        out = np.empty((g.shape[0], self.k * self.N + 1), dtype=U64)
        mask = g[:, :self.k]
        ext = np.concatenate([mask[:, :, :1], U64(0) - mask[:, :, :0:-1]], axis=2)
        out[:, :-1] = ext.reshape(g.shape[0], -1)
        out[:, -1] = g[:, self.k, 0]
        return out

    # ---- vertical packing --------------------------------------------------------------------
    def rotation_phase(self, ggsws, acc):
        """blind_rotate_assign by GGSWs (wop_pbs/mod.rs:866-892) of ONE accumulator, as one oracle
        blind rotation."""
        g = np.ascontiguousarray(ggsws, dtype=U64).reshape(-1, ggsw_words(self.k, self.N, self.L))
        nr = g.shape[0]
        if nr == 0:
            return np.array(acc, dtype=U64)
        f = self.O.FourierBsk(np.ascontiguousarray(g[::-1]).ravel(), nr, self.k, self.N, self.B, self.L)
        log2n2 = (2 * self.N).bit_length() - 1
        lwe = np.array([[((2 * self.N - (1 << i)) << (64 - log2n2)) for i in range(nr)] + [0]], dtype=U64)
        return f.blind_rotate(lwe, np.ascontiguousarray(acc, dtype=U64).reshape(1, -1))[0]

    def rotation_phase_by_cmuxes(self, ggsws, acc):
        """the same by single CMUXes with explicit rotations."""
        g = np.ascontiguousarray(ggsws, dtype=U64).reshape(-1, ggsw_words(self.k, self.N, self.L))
        acc = np.array(acc, dtype=U64).reshape(1, -1)
        for i, gg in enumerate(g[::-1]):
            acc = self.cmux_batch(gg[None], acc, self.monomial_div(acc, 1 << i))
        return acc[0]

    def cmux_tree(self, ggsws, lut):
        """cmux_tree_memory_optimized (wop_pbs/mod.rs:468-592) of ONE item, level by level: layer j
        uses GGSW nt-1-j on the adjacent pairs (2i, 2i+1); leaves = trivial GLWEs of the LUT."""
        g = np.ascontiguousarray(ggsws, dtype=U64).reshape(-1, ggsw_words(self.k, self.N, self.L))
        lut = np.ascontiguousarray(lut, dtype=U64).reshape(-1, self.N)
        nt = g.shape[0]
        assert lut.shape[0] == 1 << nt
        nodes = np.zeros((lut.shape[0], self.glwe), dtype=U64)
        nodes[:, self.k * self.N:] = lut
        for j in range(nt):
            gg = g[nt - 1 - j]
            nodes = nodes[0::2] + self.external_product(gg, nodes[1::2] - nodes[0::2])
        return nodes[0]

    def vertical_packing(self, ggsws, lut):
        """vertical_packing (wop_pbs/mod.rs:785-853) of ONE item: ggsws [nbits] most significant bit
        first, lut [npoly][N]."""
        g = np.ascontiguousarray(ggsws, dtype=U64).reshape(-1, ggsw_words(self.k, self.N, self.L))
        lut = np.ascontiguousarray(lut, dtype=U64).reshape(-1, self.N)
        nt = lut.shape[0].bit_length() - 1
        acc = self.cmux_tree(g[:nt], lut)
        acc = self.rotation_phase(g[nt:], acc)
        return self.sample_extract(acc)[0]

    # ---- exact arithmetic ----------------------------------------------------------------------
    def digits(self, x):
        """signed digits (as wrapping u64) of every word of x, [level index l-1][...] -- the
        SignedDecomposer (decomposer.rs:99-119, iter.rs:134-141) vectorised."""
        x = np.ascontiguousarray(x, dtype=U64)
        B, L = self.B, self.L
        state = ((x >> U64(63 - B * L)) + U64(1)) >> U64(1)
        state &= U64((1 << (B * L)) - 1) if B * L < 64 else ~U64(0)  # a rounding overflow wraps to 0
        out = np.empty((L,) + x.shape, dtype=U64)
        mask = U64((1 << B) - 1)
        for lvl in range(L, 0, -1):
            res = state & mask
            state = state >> U64(B)
            carry = (((res - U64(1)) | state) & res) >> U64(B - 1)
            state = state + carry
            out[lvl - 1] = res - (carry << U64(B))
        return out

    def external_product_exact(self, ggsw, d):
        """G (x) d with exact negacyclic products over the standard-domain rows (no FFT)."""
        k, N = self.k, self.N
        g = np.ascontiguousarray(ggsw, dtype=U64).reshape(self.L, k + 1, k + 1, N)
        dg = self.digits(np.ascontiguousarray(d, dtype=U64).reshape(k + 1, N))
        out = np.zeros((k + 1, N), dtype=U64)
        for lvl in range(self.L):
            for row in range(k + 1):
                for col in range(k + 1):
                    out[col] = self.O.negacyclic_mul_add_exact(dg[lvl, row], g[lvl, row, col], out[col])
        return out.ravel()

    def phase(self, glwe_sk, glwe):
        """body - sum_i mask_i * s_i of ONE GLWE."""
        k, N = self.k, self.N
        g = np.ascontiguousarray(glwe, dtype=U64).reshape(k + 1, N)
        sk = np.ascontiguousarray(glwe_sk, dtype=U64).reshape(k, N)
        acc = np.zeros(N, dtype=U64)
        for i in range(k):
            acc = self.O.negacyclic_mul_add_exact(g[i], sk[i], acc)
        return g[k] - acc


def torus_distance(a, b):
    """|a - b| on the 64-bit torus, as floats."""
    d = (np.asarray(a, dtype=U64) - np.asarray(b, dtype=U64)).astype(np.int64)
    return np.abs(d.astype(np.float64))


def index_bits(index, nbits):
    """bits of `index`, most significant first (the GGSW order of vertical packing)."""
    return [(index >> (nbits - 1 - b)) & 1 for b in range(nbits)]


def lut_value(i):
    """the 4-bit function the decryption tests look up."""
    return (7 * i + 3) % 16


def vp_lut(npoly, N, nr, delta, shift=0):
    """LUT polynomials for an index of log2(npoly) tree bits and nr rotation bits: polynomial p holds
    delta * lut_value(p 2^nr + j + shift) at coefficient j, so the looked-up sample (coefficient r of
    polynomial p, r < 2^nr) is delta * lut_value(index + shift)."""
    j = np.arange(N, dtype=np.int64)
    return np.stack([(lut_value((p << nr) + j + shift) * delta).astype(U64) for p in range(npoly)])
