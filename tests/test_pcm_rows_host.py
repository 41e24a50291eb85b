"""CPU: the host part of csrc/pcm_rows.h, what the chain, tensor and compare
kernels share on the PCM side.  tools/pcm_rows_check.cpp, built with g++ under
AddressSanitizer and UBSan, checks the view's split into (aligned pointer,
first sample) at every pointer phase of both formats, the shared view
refusals word for word, the unit range of a tile against a walk over its
samples, the overlap test against the quadratic definition (touching ranges
and no ranges included) and the row table against a prefix sum, with the
tile-count refusal at exactly 2^31 - 1 and 2^31."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pcm_rows_host_part(tmp_path):
    exe = str(tmp_path / "pcm_rows_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "pcm_rows_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    last = p.stdout.splitlines()[-1].split()
    assert last[0] == "cases" and last[2] == "bad" and int(last[3]) == 0
    # split: (8 + 4 phases) x 5 offsets x 5 checks; units: 2 unit sizes x 8
    # channel counts x 3 first frames x 3 counts x (6 and 10 values of lo) x 2
    # checks; overlap: 400 random sets; table: 50 random tables x 2
    assert int(last[1]) >= 12 * 5 * 5 + 8 * 3 * 3 * 16 * 2 + 400 + 100
