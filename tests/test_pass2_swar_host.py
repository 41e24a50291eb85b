"""CPU: the three-op pass-2 step of the K2 search (csrc/pass2_swar.h: one
32-bit shift, one bit-select with two constant words, one 16-bit SAD per
register of two kept samples) equals the reference form, the sum of
(n >> kv) ^ (n >> 15) over both halves.  tools/pass2_swar_check.cpp builds
the header's host form with g++ and runs every value of the half under test
(low and high position) against every 251st value of the other half for kv in
[1, 14], the loud variant (halves = bits 8..23, step at kv - 8) for kv in
[9, 14], and the 32-register lane form with lane 0's warm-up slots."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_swar_step_matches_reference_form(tmp_path):
    exe = str(tmp_path / "pass2_swar_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe,
                    os.path.join(ROOT, "tools", "pass2_swar_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    last = p.stdout.splitlines()[-1].split()
    assert last[0] == "cases" and last[2] == "bad" and int(last[3]) == 0
    # 2 positions x 2^16 x ceil(2^16 / 251) x (14 quiet + 3 x 6 loud kv) + lanes
    assert int(last[1]) >= 2 * 65536 * 262 * 32
