"""CPU: the library's host code under AddressSanitizer.

tools/host_asan_probe.cpp, linked with every object of libatgpu built with
the host side instrumented (`make -C python-audio-tools_amd/csrc host-asan`,
~4 min, so not part of build()): FLAC metadata and ALAC atom walks over the
reference fixtures, every truncation and byte-mutated copies; bounds and
the stream header on edge geometries; md5_cpu.h against the byte-wise MD5;
atg_host_gather against memcpy; the encoder service client against fake
services (mismatched frame counts and sizes, oversized byte counts and error
text, a mute service), guard words past the caller's buffers; the *_host
entries of the handle-less components refused on device -1; the creates of
the two FLAC handles refused on device -1, on device 0 without a GPU and with
out == NULL, *out left null.  Any ASan
report or failed check fails the test; skipped when the probe is not built.
The GPU-side replay of the bench sequence is tools/teardown_probe.cpp.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "bin", "host_asan_probe")


@pytest.mark.skipif(not os.path.exists(PROBE), reason="host ASan probe not built")
def test_host_code_clean_under_asan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    p = subprocess.run([PROBE, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["failures"] == 0
    assert line["flac_metadata_calls"] > 10000 and line["alac_info_calls"] > 1000
    assert line["service_cases"] == 6
    assert line["host_refusals"] == 15
