"""GPU parity: libatgpu's Shorten encoder (shn_encode.hip) against the files
the reference's shnenc wrote (tests/golden/shn_vectors.json: sha256 and
length) and, for what shnenc cannot make (unsigned and big-endian types,
explicit frame sizes), against tests/shn_port.py, which the generator checked
through shndec."""
import hashlib
import json
import os
from collections import defaultdict

import numpy as np
import pytest

import shn_cases
import shn_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "shn_vectors.json")))


def gpu_encode(pcms, channels, bps, block=256, sizes=None, headers=None, footers=None,
               dtype=None, **kw):
    """-> the tracks' images"""
    from audiotools import _atgpu
    enc = _atgpu.shn_encoder()
    tracks, start = [], 0
    for k, p in enumerate(pcms):
        n = len(p) // channels
        tracks.append((start, n, sizes[k] if sizes else None))
        start += n
    pcm = np.concatenate(pcms).astype(dtype or np.int16) if pcms else np.zeros(0, np.int16)
    out, res = enc.encode(pcm, tracks, channels, bps, block, headers=headers, footers=footers,
                          **kw)
    got = []
    for r, p in zip(res, pcms):
        assert r.pcm_frames == len(p) // channels
        assert r.out_offset % 4 == 0 and r.bytes % 4 == 1
        got.append(out[r.out_offset:r.out_offset + r.bytes].tobytes())
    return got


def _groups():
    g = defaultdict(list)
    for case in shn_cases.encoder_cases():
        g[(case[1], case[2], case[3])].append(case)
    return sorted(g.items())


@pytest.mark.parametrize("key,cases", _groups(), ids=lambda x: str(x) if isinstance(x, tuple)
                         else None)
def test_encoder_vectors_batch(key, cases):
    """every vector of one format and block size in one batch: the file the
    reference wrote, header and footer bytes included"""
    ch, bps, block = key
    got = gpu_encode([c[4] for c in cases], ch, bps, block, headers=[c[5] for c in cases],
                     footers=[c[6] for c in cases])
    for case, img in zip(cases, got):
        v = G["encoder"][case[0]]
        assert len(img) == v["bytes"], case[0]
        assert hashlib.sha256(img).hexdigest() == v["sha256"], case[0]


def test_impulse_zero_run():
    """the vector with one full-scale impulse in a silent 4096-frame block
    holds a zero run of a thousand bits or more"""
    case = [c for c in shn_cases.encoder_cases() if c[0] == "impulse_B4096"][0]
    img = gpu_encode([case[4]], 1, 16, 4096)[0]
    assert img == shn_port.encode(case[4], 1, 16, 4096)
    assert b"\x00" * 125 in img


@pytest.mark.parametrize("case", shn_cases.port_cases(), ids=lambda c: c[0])
def test_port_cases(case):
    """unsigned and big-endian file types, explicit frame sizes with
    mid-stream changes"""
    name, ch, bps, block, x, header, footer, be, sgn, sizes = case
    want = shn_port.encode(x, ch, bps, block, be, sgn, header, footer, sizes)
    got = gpu_encode([x], ch, bps, block, sizes=[sizes] if sizes else None, headers=[header],
                     footers=[footer], is_big_endian=be, signed_samples=sgn)[0]
    assert got == want


def test_int32_input_matches_int16():
    x = shn_cases.stepped_shifts(600, 2, 256, 3)
    assert gpu_encode([x], 2, 16, dtype=np.int32) == gpu_encode([x], 2, 16)


def test_mixed_batch_against_port():
    """8 tracks of unequal length (one empty, one a single frame) in one
    call: the bit offsets are scanned per track"""
    pcms = shn_cases.mixed_batch()
    headers = [b"h" * k for k in range(len(pcms))]
    footers = [b"f" * (k % 3) for k in range(len(pcms))]
    got = gpu_encode(pcms, 2, 16, 256, headers=headers, footers=footers)
    for k, (p, img) in enumerate(zip(pcms, got)):
        assert img == shn_port.encode(p, 2, 16, 256, False, True, headers[k], footers[k]), k


def test_capacity_protocol():
    """too small an output: ATG_ERR_CAPACITY and the size needed, with which
    the call then succeeds"""
    from audiotools import _atgpu
    x = shn_cases.stepped_shifts(3000, 2, 256, 5)
    with pytest.raises(_atgpu.ATGError) as e:
        gpu_encode([x], 2, 16, out_cap=64)
    assert e.value.status == _atgpu.ATG_ERR_CAPACITY
    want = shn_port.encode(x, 2, 16)
    assert e.value.needed == (len(want) + 3) // 4 * 4
    assert gpu_encode([x], 2, 16, out_cap=e.value.needed)[0] == want


def test_device_path_capacity_and_output():
    import torch
    from audiotools import _atgpu
    enc = _atgpu.shn_encoder()
    x = shn_cases.stepped_shifts(2000, 2, 256, 6)
    want = shn_port.encode(x, 2, 16, 256, False, True, b"head")
    d_pcm = torch.from_numpy(x.astype(np.int16)).cuda()
    d_out = torch.full((len(want) + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(_atgpu.ATGError) as e:
        enc.encode_device(d_pcm.data_ptr(), _atgpu.PCM_S16, [(0, 2000)], 2, 16,
                          d_out.data_ptr(), 16, headers=[b"head"])
    assert e.value.status == _atgpu.ATG_ERR_CAPACITY and e.value.needed >= len(want)
    torch.cuda.synchronize()
    assert bool((d_out == 0xAA).all())  # nothing written
    res, need = enc.encode_device(d_pcm.data_ptr(), _atgpu.PCM_S16, [(0, 2000)], 2, 16,
                                  d_out.data_ptr(), e.value.needed, headers=[b"head"])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert got[:res[0].bytes].tobytes() == want
    assert bool((got[need:] == 0xAA).all())
    assert set(enc.kernel_times()) == {"shn_size", "shn_scan", "shn_layout", "shn_pack",
                                       "shn_edges", "shn_total"}


@pytest.mark.parametrize("kw,status", [
    (dict(block=4097), "ATG_ERR_UNSUPPORTED"),
    (dict(block=0), "ATG_ERR_INVALID"),
    (dict(bps=24), "ATG_ERR_INVALID"),
    (dict(sizes=[[4097, 3]]), "ATG_ERR_UNSUPPORTED"),
])
def test_refused_options(kw, status):
    from audiotools import _atgpu
    x = np.zeros(4100 * 2, np.int32)
    with pytest.raises(_atgpu.ATGError) as e:
        gpu_encode([x], 2, kw.get("bps", 16), kw.get("block", 256), sizes=kw.get("sizes"),
                   dtype=np.int32)
    assert e.value.status == getattr(_atgpu, status)
    if kw.get("bps") == 24:
        assert "unsupported bits per sample" in str(e.value)
