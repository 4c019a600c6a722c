"""The classic PBS rotation on a negated accumulator (csrc/rot_mask.h, compiled by pbs_classic.hip and
by scripts/check_rot_mask.cpp alike): wrap count, wrap/sign mask words, gather address and the
carry-free hi32 formula against X^a~ p - p on a random p, for N in {256, 512, 1024, 2048}, every
a~ in [0, 2N], every lane and every h; the hcut = 2V = 32 case (N = 2048) must have been reached."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rot_mask_matches_monomial_mul_and_subtract(tmp_path):
    exe = str(tmp_path / "check_rot_mask")
    subprocess.run(["g++", "-O2", "-fopenmp", os.path.join(ROOT, "scripts", "check_rot_mask.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "identity mismatches 0\n" in out.stdout
    for n in (256, 512, 1024, 2048):
        assert re.search(rf"^N {n} mismatches 0 ", out.stdout, re.M), out.stdout
    reached = int(re.search(r"^N 2048 mismatches 0 hcut32 (\d+)$", out.stdout, re.M).group(1))
    assert reached > 0, "hcut = 2V = 32 never reached"
    assert re.search(r"^N 1024 mismatches 0 hcut32 0$", out.stdout, re.M)  # 2V = 16 there
