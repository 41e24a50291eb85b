"""CPU: the sample range in which K1's autocorrelation uses a fused
multiply-add (csrc/lpc_flat.h) against the Tukey table the engine builds, and
the exactness argument behind it.  tools/lpc_flat_check.cpp, built with g++
and -ffp-contract=off, checks (a) for every N in [14, 4608] and 8192, 16384,
65535, at the margins 8, 12 and 32, that every table entry in the range and the
margin before it is exactly 1.0; (b) for the block lengths 4096 4608 576 256
208 192 160 57, four stereo candidates and five signal kinds, that the 13 sums
with std::fma inside the range equal multiply-then-add everywhere bit for bit
(per sample, in the kernel's 52- then 13-sample groups, and in 13-sample
groups); (c) that widening the range by one sample at either end does change
sums of noise input."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_fma_range_is_flat_and_exact(tmp_path):
    exe = str(tmp_path / "lpc_flat_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tools", "lpc_flat_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    last = p.stdout.splitlines()[-1].split()
    assert last[0] == "cases" and last[2] == "bad" and int(last[3]) == 0
    # (a) 4598 lengths x 3 margins, (b) 8 lengths x 5 kinds x 12 trials x 4
    # candidates x 3 granularities
    assert int(last[1]) >= 4598 * 3 + 8 * 5 * 12 * 4 * 3
    # (c) the widened ranges are seen to fail
    assert last[4] == "wide_lo" and int(last[5]) > 0
    assert last[6] == "wide_hi" and int(last[7]) > 0
