"""The keyswitch family (csrc/keyswitch.hip: LWE -> LWE and the LWE -> GLWE packing keyswitch; the
small-base arm of csrc/pfpks.hip) bit-exact against the oracle, and at the small shapes against the
numpy reference of test_keyswitch_reference.py, on that file's edge rows.  Keys are random u64 words
(exactness needs no valid key); engines come from params_2_2.with_(...) with no bootstrap key.

In process (the int8-MFMA arm, asserted through the scratch queries: capi_pbs.cpp returns 0 bytes exactly
when the scalar arm is chosen): the column-tile edges out_dim + 1 = 63, 64, 65, 130 at counts 1, 6
and 67; every decomposition of parameters.py and (7, 9), (1, 16), (3, 17); the input shape (N, k) =
(256, 5); the unsplit launch (gridDim.z == 1) reached by construction with 16 x 8 = 128 tiles; the
rows past `count` of a device output; the shapes no kernel takes.

The library reads TFHE_MI355_KS_NO_MFMA, TFHE_MI355_PFPKS_NO_MFMA and TFHE_MI355_KS_SPLIT_WG once per
process, so the scalar kernels (keyswitch_kernel, pfpks_kernel at small bases) and the unsplit launch at
a small count run in fresh child processes: this file run as a script, one child at a time.
  scalar   both NO_MFMA variables: the scalar keyswitch at two column-tile edges and five
           decompositions up to L = KS_MAXL = 16, the packing keyswitch at the Manticore shape, the
           generic pfpks kernel at bases 7 and 9.
  unsplit  TFHE_MI355_KS_SPLIT_WG=1 (launch_keyswitch_mfma then computes split = 1 for any count:
           known from reading it, nothing reports it): the largest shape ks_mfma_supported accepts,
           in_dim = 32768 at (7, 7), mpad * 2^6 * 128 = 1 879 048 192 < 2^31, on the two heavy rows
           against keys of all-zero and all-one words (every plane byte -128 / +127 after the repack)
           -- the int32 accumulators at their largest; and (7, 8), which the bound rejects.
A child prints one line per failed case and exits non-zero if any failed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # a child process: the paths tests/conftest.py sets up under pytest
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tfhe-rs-odd_amd")]

from tfhe_mi355 import parameters as P  # noqa: E402
from test_keyswitch_reference import (ALL_ONES, BODY_ONLY, HEAVY_NEG, HEAVY_POS, N_EDGE, ZERO, edge_rows,  # noqa: E402
                                      keyswitch_reference)

pytestmark = pytest.mark.gpu

U64 = np.uint64
SENTINEL = 0xA5C3_0FF0_5A3C_F00F
ROWS = N_EDGE + 1  # the edge rows and one random row
TABLE_DECOMPOSITIONS = sorted({(p.ks_base_log, p.ks_level) for p in list(P.ALL.values()) + list(P.WOPBS_ALL.values())})
SCALAR_DECOMPOSITIONS = [(3, 5), (7, 2), (7, 9), (1, 16), (3, 16)]
_cache = {}


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=U64, order="C").view(np.int64)).cuda()  # a copy: `a` may be read-only


def _host(t):
    return t.cpu().numpy().view(U64)


def _sync():
    import torch

    torch.cuda.current_stream().synchronize()


def _engine(N, k, n, B, L, base=P.PARAM_MESSAGE_2_CARRY_2_KS_PBS):
    from tfhe_mi355 import Engine

    return Engine(base.with_(glwe_dimension=k, polynomial_size=N, lwe_dimension=n, ks_base_log=B, ks_level=L,
                             pbs_level=1 if base.polynomial_size <= 2048 else base.pbs_level,
                             name=f"ks_{N}_{k}_{n}_{B}_{L}"), 0)


def _random_key(seed, words):
    return np.random.default_rng(seed).integers(0, 1 << 64, words, dtype=U64)


def _ks_case(orc, N, k, n, B, L, count):
    """an engine with a random keyswitching key uploaded, the rows and the oracle's output."""
    in_dim = k * N
    ksk = _random_key(1000 * n + 10 * B + L, in_dim * L * (n + 1))
    eng = _engine(N, k, n, B, L)
    eng.upload_keyswitch_key(ksk)
    x = edge_rows(B, L, in_dim + 1, count, seed=n + B + L)
    return eng, ksk, x, orc.keyswitch(ksk, in_dim, n, B, L, x)


def _same(got, exp, what):
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{what}: rows {bad.tolist()[:16]} differ, {np.count_nonzero(got != exp)} words"


def _check_keyswitch(eng, x, exp, counts, what):
    """the host form at each count from row 0, and every one of the first ROWS rows as a call of its own."""
    for count in counts:
        _same(eng.keyswitch(x[:count]), exp[:count], f"{what} count {count}")
    for r in range(ROWS):
        _same(eng.keyswitch(x[r]), exp[r:r + 1], f"{what} row {r} alone")
    assert not eng.keyswitch(x[ZERO]).any(), f"{what}: the all-zero row"


# ---- in process: the int8-MFMA arm ------------------------------------------------------------------
@pytest.mark.parametrize("n", [62, 63, 64, 129])
def test_column_tile_edges(orc, n):
    """in_dim = 512 at (3, 5): out_dim + 1 = 63, 64, 65 and 130 columns around the 64-column tile; 67 rows
    cross the 64-row tile with three live rows."""
    eng, ksk, x, exp = _ks_case(orc, 512, 1, n, 3, 5, 67)
    assert eng.ks_scratch_bytes(1) > 0
    assert np.array_equal(exp, keyswitch_reference(ksk, 512, n + 1, n, 3, 5, x))
    _check_keyswitch(eng, x, exp, (1, 6, 67), f"n = {n}")
    d_out = _dev(np.zeros((67, n + 1), dtype=U64))
    eng.keyswitch_async(_dev(x), d_out, 67)
    _sync()
    _same(_host(d_out), exp, f"n = {n} device form")
    eng.close()


@pytest.mark.parametrize("dec", TABLE_DECOMPOSITIONS + [(7, 9), (1, 16), (3, 17)], ids=str)
def test_every_decomposition(orc, dec):
    """in_dim = 512, out_dim = 63, the edge rows and one random row; (3, 17) has more levels than the
    scalar kernel holds and the MFMA arm must still take it."""
    B, L = dec
    eng, ksk, x, exp = _ks_case(orc, 512, 1, 63, B, L, ROWS)
    assert eng.ks_scratch_bytes(1) > 0
    assert np.array_equal(exp, keyswitch_reference(ksk, 512, 64, 63, B, L, x))
    _check_keyswitch(eng, x, exp, (ROWS,), str(dec))
    eng.close()


def test_table_decompositions_are_the_15_of_the_parameter_tables():
    assert len(TABLE_DECOMPOSITIONS) == 15 and TABLE_DECOMPOSITIONS[0] == (2, 4) and TABLE_DECOMPOSITIONS[-1] == (7, 2)


def test_second_input_shape(orc):
    """(N, k) = (256, 5): in_dim = 1280 at (4, 3), LWE -> LWE to 71 columns and the packing keyswitch to
    (k + 1) N = 1536 columns with the body on column kN = 1280."""
    N, k, n, B, L = 256, 5, 70, 4, 3
    eng, ksk, x, exp = _ks_case(orc, N, k, n, B, L, 67)
    assert eng.ks_scratch_bytes(1) > 0
    assert np.array_equal(exp, keyswitch_reference(ksk, k * N, n + 1, n, B, L, x))
    _check_keyswitch(eng, x, exp, (6, 67), "(256, 5)")
    pksk = _random_key(77, k * N * L * (k + 1) * N)
    eng.upload_packing_keyswitch_key(pksk, B, L)
    assert eng.pks_scratch_bytes(1) > 0
    pexp = orc.packing_keyswitch(pksk, k * N, k, N, B, L, x)
    assert np.array_equal(pexp[:ROWS], keyswitch_reference(pksk, k * N, (k + 1) * N, k * N, B, L, x[:ROWS]))
    for r in (BODY_ONLY, ALL_ONES):  # no digit: the body alone, on column kN
        assert np.flatnonzero(pexp[r]).tolist() == [k * N] and pexp[r, k * N] == x[r, -1]
    _same(eng.packing_keyswitch(x), pexp, "(256, 5) packing, 67 rows")
    _same(eng.packing_keyswitch(x[:ROWS]), pexp[:ROWS], "(256, 5) packing")
    _same(eng.packing_keyswitch(x[HEAVY_NEG]), pexp[HEAVY_NEG:HEAVY_NEG + 1], "(256, 5) packing, one row")
    assert not eng.packing_keyswitch(x[ZERO]).any()
    eng.close()


def _big_case(orc):
    """in_dim = 512 at (3, 5) to 1024 columns, LWE (lwe_dimension = 1023) and GLWE ((k + 1) N): 16 column
    tiles, so 449 to 512 rows make the 128 tiles from which launch_keyswitch_mfma does not split K.
    512 rows with the edge rows in front, the oracle's outputs, once."""
    if "big" not in _cache:
        N, k, n, B, L = 512, 1, 1023, 3, 5
        eng, ksk, x, exp = _ks_case(orc, N, k, n, B, L, 512)
        pksk = _random_key(78, k * N * L * (k + 1) * N)
        eng.upload_packing_keyswitch_key(pksk, B, L)
        pexp = orc.packing_keyswitch(pksk, k * N, k, N, B, L, x[:449])
        for a in (x, exp, pexp):
            a.setflags(write=False)
        assert eng.ks_scratch_bytes(1) > 0 and eng.pks_scratch_bytes(1) > 0
        _cache["big"] = dict(eng=eng, x=x, exp=exp, pexp=pexp, d_x=_dev(x))
    return _cache["big"]


@pytest.mark.parametrize("count", [449, 512])
def test_unsplit_path(orc, count):
    """one device call of `count` rows: 8 row tiles x 16 column tiles, gridDim.z == 1 (plain stores)."""
    c = _big_case(orc)
    d_out = _dev(np.zeros((count, 1024), dtype=U64))
    c["eng"].keyswitch_async(c["d_x"], d_out, count)
    _sync()
    _same(_host(d_out), c["exp"][:count], f"unsplit, {count} rows")
    _same(c["eng"].keyswitch(c["x"][:count]), c["exp"][:count], f"host form, {count} rows")


@pytest.mark.parametrize("count", [5, 449])
@pytest.mark.parametrize("packing", [False, True], ids=["lwe", "glwe"])
def test_rows_past_count_stay_untouched(orc, count, packing):
    """count 5 splits K (ks_digits_kernel zeroes the rows, the slices add into them with atomics), count
    449 does not: either way the first `count` rows of a sentinel-filled output equal the oracle, the
    three rows after them keep the sentinel, and a second call into the same buffer gives the same."""
    c = _big_case(orc)
    eng, exp = c["eng"], (c["pexp"] if packing else c["exp"])[:count]
    call = eng.packing_keyswitch_async if packing else eng.keyswitch_async
    d_out = _dev(np.full((count + 3, 1024), SENTINEL, dtype=U64))
    for attempt in (1, 2):
        call(c["d_x"], d_out, count)
        _sync()
        got = _host(d_out)
        _same(got[:count], exp, f"call {attempt}")
        assert (got[count:] == U64(SENTINEL)).all(), f"call {attempt}: rows past count were written"


def test_rejected_shapes_fail_loudly(orc):
    """ks_base_log = 8: neither kernel takes it (digits up to 128 do not fit int8), so every form of the
    call raises; a packing key with base_log * level >= 64 is refused at upload, one with base_log = 8 at
    the call."""
    from tfhe_mi355 import EngineError

    eng, ksk, x, exp = _ks_case(orc, 512, 1, 63, 8, 5, ROWS)
    assert eng.ks_scratch_bytes(1) == 0
    for rows in (x[:ROWS], x[5]):
        with pytest.raises(EngineError):
            eng.keyswitch(rows)
    d_out = _dev(np.full((ROWS, 64), SENTINEL, dtype=U64))
    with pytest.raises(EngineError):
        eng.keyswitch_async(_dev(x[:ROWS]), d_out, ROWS)
    _sync()
    assert (_host(d_out) == U64(SENTINEL)).all()
    pksk = _random_key(79, 512 * 8 * 1024)
    for B, L in ((8, 8), (32, 2), (63, 2), (0, 8)):
        with pytest.raises(EngineError, match="invalid packing ks decomposition"):
            eng.upload_packing_keyswitch_key(pksk[:512 * L * 1024], B, L)
    eng.upload_packing_keyswitch_key(pksk[:512 * 2 * 1024], 8, 2)
    assert eng.pks_scratch_bytes(1) == 0
    with pytest.raises(EngineError):
        eng.packing_keyswitch(x[:ROWS])
    eng.close()


# ---- fresh child processes ------------------------------------------------------------------------------
def _run_child(mode, env):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=300)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    done = [line for line in run.stdout.splitlines() if line.startswith(f"{mode}: ")]
    assert done, out
    return done[-1]


def test_scalar_arm_in_a_fresh_process():
    """keyswitch_kernel (LWE and packing) and pfpks_kernel at bases 7 and 9, never chosen otherwise."""
    done = _run_child("scalar", {"TFHE_MI355_KS_NO_MFMA": "1", "TFHE_MI355_PFPKS_NO_MFMA": "1"})
    assert done == f"scalar: {2 * len(SCALAR_DECOMPOSITIONS) + 4} cases, 0 failed", done


def test_unsplit_worst_case_in_a_fresh_process():
    """the int32 accumulator bound of ks_mfma_supported at the largest accepted shape, K not split."""
    done = _run_child("unsplit", {"TFHE_MI355_KS_SPLIT_WG": "1"})
    assert done == "unsplit: 4 cases, 0 failed", done


class _Cases:
    """runs the cases of a child: a mismatch is recorded and the next case runs; anything else (an
    engine or HIP error) ends the child at once."""

    def __init__(self, mode):
        self.mode, self.ran, self.failed = mode, 0, []

    def run(self, name, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.failed.append(name)
            print(f"FAILED {name}: {e}", flush=True)

    def finish(self):
        print(f"{self.mode}: {self.ran} cases, {len(self.failed)} failed", flush=True)
        sys.exit(1 if self.failed else 0)


def _child_scalar(orc):
    from tfhe_mi355 import Engine, EngineError
    from wopbs_reference import pfpks, pfpksk_shape

    cases = _Cases("scalar")

    def lwe(n, B, L):
        eng, ksk, x, exp = _ks_case(orc, 512, 1, n, B, L, 67)
        assert eng.ks_scratch_bytes(1) == 0 and eng.ks_scratch_bytes(67) == 0, "the MFMA arm is on"
        _check_keyswitch(eng, x, exp, (1, 67), f"scalar n = {n} {(B, L)}")
        d_out = _dev(np.full((70, n + 1), SENTINEL, dtype=U64))
        eng.keyswitch_async(_dev(x), d_out, 67)
        _sync()
        _same(_host(d_out)[:67], exp, "device form")
        assert (_host(d_out)[67:] == U64(SENTINEL)).all(), "rows past count were written"
        eng.close()

    for n in (62, 64):
        for B, L in SCALAR_DECOMPOSITIONS:
            cases.run(f"keyswitch n = {n} {(B, L)}", lambda: lwe(n, B, L))

    def too_many_levels():
        eng, ksk, x, exp = _ks_case(orc, 512, 1, 62, 3, 17, ROWS)
        assert eng.ks_scratch_bytes(1) == 0
        try:
            eng.keyswitch(x[:ROWS])
        except EngineError:
            return
        raise AssertionError("17 levels did not raise")

    cases.run("keyswitch (3, 17) raises", too_many_levels)

    def packing():
        """the Manticore shape and the 67 rows of test_gadget_gpu.test_packing_keyswitch_bit_exact, then
        the edge rows."""
        p = P.MANTICORE_PARAMETERS
        k, N, B, L = p.glwe_dimension, p.polynomial_size, p.ks_base_log, p.ks_level
        glwe_sk = orc.binary_key(11, 2, k * N)
        pksk = orc.gen_pksk(31, glwe_sk, glwe_sk, k, N, B, L, p.glwe_modular_std_dev)
        eng = Engine(p, 0)
        eng.upload_packing_keyswitch_key(pksk, B, L)
        assert eng.pks_scratch_bytes(1) == 0 and eng.pks_scratch_bytes(67) == 0, "the MFMA arm is on"
        x = np.random.default_rng(5).integers(0, 2 ** 64, (67, k * N + 1), dtype=U64)
        x[3] = 0
        x[4, :] = U64(1 << 63)
        _same(eng.packing_keyswitch(x), orc.packing_keyswitch(pksk, k * N, k, N, B, L, x), "Manticore rows")
        e = edge_rows(B, L, k * N + 1, ROWS, seed=6)
        exp = orc.packing_keyswitch(pksk, k * N, k, N, B, L, e)
        _same(eng.packing_keyswitch(e), exp, "edge rows")
        assert not eng.packing_keyswitch(e[ZERO]).any()
        d_out = _dev(np.full((ROWS + 3, (k + 1) * N), SENTINEL, dtype=U64))
        eng.packing_keyswitch_async(_dev(e), d_out, ROWS)
        _sync()
        _same(_host(d_out)[:ROWS], exp, "device form")
        assert (_host(d_out)[ROWS:] == U64(SENTINEL)).all(), "rows past count were written"
        eng.close()

    cases.run("packing keyswitch, Manticore", packing)

    def generic_pfpks(N, k, B, L, count):
        key = _random_key(N + 3 * k + B, int(np.prod(pfpksk_shape(k, N, L))))
        eng = Engine(P.PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(glwe_dimension=k, polynomial_size=N, pbs_level=1,
                                                            name=f"pfpks_{N}_{k}"), 0)
        eng.upload_pfpksk_list(key, B, L)
        assert eng.pfpks_scratch_bytes(1) == 0, "the MFMA arm is on"
        x = edge_rows(B, L, k * N + 1, count, seed=B)
        exp = pfpks(orc, key, k, N, B, L, x)
        eng.kernel_timing(1)
        got = eng.private_functional_packing_keyswitch(x)
        ran = set(eng.kernel_times())
        assert ran == {"pfpks_generic"}, ran
        assert np.array_equal(got, exp), f"{np.count_nonzero(got != exp)} words differ"
        assert not got[ZERO].any()
        assert np.array_equal(eng.private_functional_packing_keyswitch(x[HEAVY_NEG]), exp[HEAVY_NEG:HEAVY_NEG + 1])
        eng.close()

    cases.run("pfpks generic (512, 1, 7, 6)", lambda: generic_pfpks(512, 1, 7, 6, 67))
    cases.run("pfpks generic (512, 3, 9, 3)", lambda: generic_pfpks(512, 3, 9, 3, ROWS))
    cases.finish()


def _child_unsplit(orc):
    base = P.PARAM_MESSAGE_4_CARRY_4_KS_PBS
    N, n, B = base.polynomial_size, 4, 7
    cases = _Cases("unsplit")
    x = edge_rows(B, 7, N + 1, ROWS, seed=3)[[HEAVY_NEG, HEAVY_POS, N_EDGE]]

    def at(L, fill, mfma):
        words = N * L * (n + 1)
        ksk = _random_key(L, words) if fill is None else np.full(words, fill, dtype=U64)
        eng = _engine(N, 1, n, B, L, base)
        eng.upload_keyswitch_key(ksk)
        assert (eng.ks_scratch_bytes(1) > 0) == mfma, "the other arm is on"
        rows = x if L == 7 else edge_rows(B, L, N + 1, ROWS, seed=3)[[HEAVY_NEG, HEAVY_POS, N_EDGE]]
        exp = orc.keyswitch(ksk, N, n, B, L, rows)
        _same(eng.keyswitch(rows), exp, "three rows")
        d_out = _dev(np.full((6, n + 1), SENTINEL, dtype=U64))
        eng.keyswitch_async(_dev(rows), d_out, 3)
        _sync()
        _same(_host(d_out)[:3], exp, "device form")
        assert (_host(d_out)[3:] == U64(SENTINEL)).all(), "rows past count were written"
        eng.close()

    assert 229376 * 64 * 128 < 1 << 31 <= 262144 * 64 * 128  # (7, 7) is the last level count the bound takes
    cases.run("(7, 7) key of zero words", lambda: at(7, 0, True))
    cases.run("(7, 7) key of all-one words", lambda: at(7, (1 << 64) - 1, True))
    cases.run("(7, 7) random key", lambda: at(7, None, True))
    cases.run("(7, 8) takes the scalar arm", lambda: at(8, None, False))
    cases.finish()


if __name__ == "__main__":
    from oracle import oracle as O

    O.build()
    {"scalar": _child_scalar, "unsplit": _child_unsplit}[sys.argv[1]](O)
