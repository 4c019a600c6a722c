"""The classic PBS kernel's rotation (negated accumulator + sign/wrap mask words, csrc/rot_mask.h) at
mask elements chosen to sit on every boundary of the mask logic, bit-exact against the oracle.

Row r of a batch carries ONE modulus-switched target a~ in every mask element, so that all n CMUXes
of the row rotate by it; the last row cycles through all targets.  Targets (N = polynomial size):
0, 1, 63, 64, 65 (first lanes start to wrap), N-64, N-63 (hcut reaches 2V for the first lanes),
N-1, N, N+1, N+63, N+64 (the same past a full turn: sign flipped), 2N-65, 2N-63, 2N-1 and 2N
(common.rs:18-25 allows it).  Bodies and LUTs are random.

At 2_2 a 17-row call is served by the latency kernel unless TFHE_MI355_LATENCY_MAX=0, which the
library reads once per process: that case (the throughput kernel's small-batch launch, ciphertexts
spread over the CUs) runs in a child process; the same rows repeated past the latency kernel's
limit run in-process through the persistent ticket launch.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def targets(N):
    return [0, 1, 63, 64, 65, N - 64, N - 63, N - 1, N, N + 1, N + 63, N + 64, 2 * N - 65, 2 * N - 63,
            2 * N - 1, 2 * N]


def mask_element(t, N):
    """A torus element whose modulus switch (fast_pbs_modulus_switch, common.rs:26-43) is t."""
    if t == 2 * N:
        return np.uint64(2 ** 64 - 1)
    return np.uint64(t << (64 - (2 * N).bit_length() + 1))


def rotation_rows(N, n, seed):
    """len(targets) + 1 ciphertexts: row r all a~ = targets[r]; the last row cycles through them."""
    ts = targets(N)
    el = np.array([mask_element(t, N) for t in ts], dtype=np.uint64)
    cts = np.empty((len(ts) + 1, n + 1), dtype=np.uint64)
    cts[:-1, :n] = el[:, None]
    cts[-1, :n] = el[np.arange(n) % len(ts)]
    cts[:, n] = np.random.default_rng(seed).integers(0, 2 ** 64, len(ts) + 1, dtype=np.uint64)
    return cts


def test_mask_elements_switch_to_their_targets():
    for N in (256, 1024, 2048):
        log2n = N.bit_length() - 1
        for t in targets(N):
            x = int(mask_element(t, N))
            assert ((x >> (64 - log2n - 2)) + 1) >> 1 == t


def _random_lut(p, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (1, (p.glwe_dimension + 1) * p.polynomial_size),
                                                dtype=np.uint64)


@pytest.fixture(scope="module")
def rows_2_2(keys_2_2):
    """The 17 rows at 2_2, one random LUT and the oracle's outputs (shared, read-only)."""
    p = keys_2_2.params
    cts = rotation_rows(p.polynomial_size, p.lwe_dimension, 21)
    assert cts.shape[0] == 17
    lut = _random_lut(p, 22)
    exp = keys_2_2.fbsk.pbs(cts, lut, threads=8)
    exp_glwe = keys_2_2.fbsk.blind_rotate(cts[:4], lut, threads=4)
    for a in (cts, lut, exp, exp_glwe):
        a.setflags(write=False)
    return cts, lut, exp, exp_glwe


def _child(work):
    """Child process (TFHE_MI355_LATENCY_MAX=0): the 17 rows through the throughput kernel."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tfhe-rs-odd_amd"))
    from tfhe_mi355 import Engine
    from tfhe_mi355.parameters import PARAM_MESSAGE_2_CARRY_2_KS_PBS as P

    eng = Engine(P, 0)
    eng.upload_bootstrap_key(np.load(os.path.join(work, "bsk.npy")))
    cts, lut = np.load(os.path.join(work, "cts.npy")), np.load(os.path.join(work, "lut.npy"))
    eng.kernel_timing(1)
    np.save(os.path.join(work, "pbs.npy"), eng.programmable_bootstrap(cts, lut))
    np.save(os.path.join(work, "glwe.npy"), eng.blind_rotate(cts[:4], lut))
    with open(os.path.join(work, "kernels.txt"), "w") as f:
        f.write("\n".join(f"{k} {v[1]}" for k, v in eng.kernel_times().items()))


def test_rotation_targets_2_2_small_batch_and_blind_rotate(keys_2_2, rows_2_2, tmp_path):
    """17 rows in one call of the throughput kernel (small-batch launch: ciphertexts spread over
    the CUs), and tfhe_mi355_blind_rotate on the first four rows (no sample extraction: the sign
    of the stored accumulator)."""
    cts, lut, exp, exp_glwe = rows_2_2
    np.save(tmp_path / "bsk.npy", keys_2_2.bsk)
    np.save(tmp_path / "cts.npy", cts)
    np.save(tmp_path / "lut.npy", lut)
    env = dict(os.environ, TFHE_MI355_LATENCY_MAX="0")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env, capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    kernels = dict(line.split() for line in open(tmp_path / "kernels.txt").read().splitlines())
    assert int(kernels.get("pbs_classic_kernel", 0)) == 2 and "pbs_latency_kernel" not in kernels, kernels
    got = np.load(tmp_path / "pbs.npy")
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"rows {bad.tolist()} differ (targets {targets(2048)})"
    assert np.array_equal(np.load(tmp_path / "glwe.npy"), exp_glwe)


def test_rotation_targets_2_2_ticket_launch(keys_2_2, rows_2_2):
    """The same rows repeated to 782 ciphertexts (more than the latency kernel takes): the
    persistent grid with the ciphertext ticket queue."""
    from tfhe_mi355 import Engine

    cts, lut, exp, _ = rows_2_2
    eng = Engine(keys_2_2.params, 0)
    eng.upload_bootstrap_key(keys_2_2.bsk)
    eng.kernel_timing(1)
    got = eng.programmable_bootstrap(np.tile(cts, (46, 1)), lut)
    assert "pbs_classic_kernel" in eng.kernel_times()
    bad = np.flatnonzero((got != np.tile(exp, (46, 1))).any(axis=1))
    assert bad.size == 0, f"rows {bad.tolist()[:20]} differ (row % 17 -> target index)"


def _shape_case(orc, keys):
    from tfhe_mi355 import Engine

    p = keys.params
    eng = Engine(p, 0)
    eng.upload_bootstrap_key(keys.bsk)
    cts = rotation_rows(p.polynomial_size, p.lwe_dimension, 23)
    lut = _random_lut(p, 24)
    eng.kernel_timing(1)
    got = eng.programmable_bootstrap(cts, lut)
    assert "pbs_classic_kernel" in eng.kernel_times()
    exp = keys.fbsk.pbs(cts, lut, threads=8)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"rows {bad.tolist()} differ (targets {targets(p.polynomial_size)})"
    assert np.array_equal(eng.blind_rotate(cts[:4], lut), keys.fbsk.blind_rotate(cts[:4], lut, threads=4))


def test_rotation_targets_manticore(orc, keys_manticore):
    """(N, k, L) = (1024, 1, 2): 2V = 16 coefficients per lane, the two-level digit path."""
    _shape_case(orc, keys_manticore)


def test_rotation_targets_sha3_40(orc):
    """(N, k, L) = (256, 5, 1): 2V = 4, six waves per ciphertext."""
    from conftest import KeySet
    from tfhe_mi355.parameters import GADGET_SHA3_PARAMETERS_40

    _shape_case(orc, KeySet(orc, GADGET_SHA3_PARAMETERS_40, seed=7))


if __name__ == "__main__":
    _child(sys.argv[1])
