"""CPU: the True Audio checker (tests/tta_port.py) against the reference
encoder's and decoder's recorded output (tests/golden/tta_vectors.json, made
by tests/golden/make_tta_golden.py), and libatgpu's host-side header and
seektable parser (atg_tta_read_info) against the reference's fixtures and
damaged headers.  No kernel is launched."""
import functools
import hashlib
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import tta_cases
import tta_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "tta_vectors.json")))
TTAENC = os.path.join(ROOT, "oracle", "_ref", "ttaenc")


def fixture(name):
    with open(os.path.join(HERE, "golden", "fixtures", name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def port_images():
    """every encoder case through tta_port, once; the long 44.1 kHz frames in
    a call of their own so that the rest is not padded to their length"""
    cases = tta_cases.encoder_cases()
    out = {}
    for group in ([c for c in cases if c[3] == tta_cases.RATE],
                  [c for c in cases if c[3] != tta_cases.RATE]):
        got = tta_port.encode_many([(x, ch, bps, rate) for _, ch, bps, rate, x in group])
        for c, g in zip(group, got):
            out[c[0]] = g
    return out


def test_vector_set_matches_cases():
    assert sorted(G["encoder"]) == sorted(c[0] for c in tta_cases.encoder_cases())
    assert sorted(G["decoder"]) == sorted(tta_cases.DECODER_CASES + tta_cases.FIXTURES)


def test_port_reproduces_encoder_vectors():
    images = port_images()
    for name, v in sorted(G["encoder"].items()):
        img, sizes = images[name]
        assert len(img) == v["bytes"], name
        assert sizes == v["frame_sizes"], name
        assert hashlib.sha256(img).hexdigest() == v["sha256"], name


def test_port_reproduces_decoder_vectors():
    """what the reference decoder wrote, which is also what was encoded; the
    long 44.1 kHz frames in a group of their own so that the others are not
    padded to their length"""
    images = port_images()
    cases = {c[0]: c for c in tta_cases.encoder_cases()}
    long_ones = [n for n in tta_cases.DECODER_CASES if cases[n][3] != tta_cases.RATE]
    groups = ([n for n in tta_cases.DECODER_CASES if n not in long_ones] +
              list(tta_cases.FIXTURES), long_ones)
    assert sum(len(g) for g in groups) == len(G["decoder"])
    for names in groups:
        data = [images[n][0] if n in images else fixture(n) for n in names]
        for name, res in zip(names, tta_port.decode_many(data)):
            status, _, bad, pcm, info = res
            v = G["decoder"][name]
            assert v["returncode"] == 0 and status == tta_port.OK and bad is None, name
            raw = tta_cases.pcm_bytes(pcm, info["bits_per_sample"])
            assert len(raw) == v["bytes"], name
            assert hashlib.md5(raw).hexdigest() == v["md5"], name
            if name in cases:
                assert np.array_equal(pcm, cases[name][4]), name


# ------------------------------------------------------------ read_info
def read_info(data):
    from audiotools import _atgpu
    return _atgpu.tta_read_info(data)


@pytest.mark.parametrize("name,fields,id3", [
    ("trueaudio.tta", (2, 16, 44100, 10), 0),
    ("tta-id3-2.tta", (2, 16, 96000, 96000), None),
])
def test_read_info_fixtures(name, fields, id3):
    data = fixture(name)
    st, info, sizes = read_info(data)
    pst, pstage, pinfo, psizes = tta_port.read_info(data)
    assert st == 0 and pst == 0 and info.stage == 2
    assert (info.channels, info.bits_per_sample, info.sample_rate,
            info.total_pcm_frames) == fields
    assert (pinfo["channels"], pinfo["bits_per_sample"], pinfo["sample_rate"],
            pinfo["total_pcm_frames"]) == fields
    assert info.block_size == fields[2] * 256 // 245
    assert info.total_tta_frames == len(sizes) == len(psizes)
    assert [int(s) for s in sizes] == psizes
    assert info.id3_bytes == pinfo["id3_bytes"] == tta_port.skip_id3v2(data)
    if id3 is not None:
        assert info.id3_bytes == id3
    else:
        assert info.id3_bytes > 0 and data[info.id3_bytes:info.id3_bytes + 4] == b"TTA1"
    assert info.frames_offset == pinfo["frames_offset"]
    # the seektable accounts for every byte that follows it
    assert info.frames_offset + sum(psizes) == len(data)


def three_frames():
    x = np.arange(3 * tta_cases.BLOCK - 5, dtype=np.int32) % 200 - 100
    return tta_port.build_file([b"\1\2\3\4\5\6\7\10"] * 3, 1, 16, tta_cases.RATE, len(x))


def flip(data, byte, bit=0):
    b = bytearray(data)
    b[byte] ^= 1 << bit
    return bytes(b)


IO, CRC, SIG, FMT = 1, 2, 3, 4

DAMAGE = [
    # (name, image, status, stage)
    ("signature bit", lambda d: flip(d, 2, 3), SIG, 0),
    ("signature TTA2", lambda d: d[:3] + b"2" + d[4:], SIG, 0),
    ("format bit", lambda d: flip(d, 4, 1), FMT, 0),
    ("format 2", lambda d: d[:4] + struct.pack("<H", 2) + d[6:], FMT, 0),
    ("channels bit", lambda d: flip(d, 6, 1), CRC, 0),
    ("bits per sample bit", lambda d: flip(d, 8, 3), CRC, 0),
    ("sample rate bit", lambda d: flip(d, 11, 0), CRC, 0),
    ("total frames bit", lambda d: flip(d, 14, 0), CRC, 0),
    ("header crc bit", lambda d: flip(d, 20, 7), CRC, 0),
    ("seektable entry bit", lambda d: flip(d, 22 + 5, 2), CRC, 1),
    ("seektable crc bit", lambda d: flip(d, 22 + 12, 0), CRC, 1),
    ("header cut in the fields", lambda d: d[:17], IO, 0),
    ("header cut in its crc", lambda d: d[:21], IO, 0),
    ("nothing", lambda d: b"", IO, 0),
    ("seektable cut", lambda d: d[:22 + 9], IO, 1),
]


@pytest.mark.parametrize("name,damage,status,stage", DAMAGE, ids=[d[0] for d in DAMAGE])
def test_read_info_damage(name, damage, status, stage):
    data = damage(three_frames())
    st, info, sizes = read_info(data)
    assert (st, info.stage) == (status, stage)
    assert len(sizes) == 0
    assert tta_port.read_info(data)[:2] == (status, stage)


def test_read_info_recomputed_crc_still_checks_format():
    """a format of 2 under a valid CRC is refused for the format, and a
    signature of TTA2 for the signature: both come before the CRC"""
    d = three_frames()
    for patch, status in ((d[:4] + struct.pack("<H", 2) + d[6:18], FMT),
                          (b"TTA2" + d[4:18], SIG)):
        img = patch + struct.pack("<I", zlib.crc32(patch) & 0xFFFFFFFF) + d[22:]
        assert read_info(img)[0] == status
        assert tta_port.read_info(img)[0] == status


def test_read_info_undamaged():
    st, info, sizes = read_info(three_frames())
    assert st == 0 and [int(s) for s in sizes] == [8, 8, 8] and info.frames_offset == 38


# ------------------------------------------------------ live reference
@pytest.mark.skipif(not os.path.exists(TTAENC), reason="oracle/_ref/ttaenc not built")
@pytest.mark.parametrize("ch,bps,n", [(1, 8, 700), (2, 16, tta_cases.BLOCK + 3), (3, 24, 500)])
def test_port_matches_live_reference(tmp_path, ch, bps, n):
    import signals
    x = signals.make("tone", n, ch, bps, seed=n)
    path = str(tmp_path / "live.tta")
    subprocess.run([TTAENC, "-c", str(ch), "-r", str(tta_cases.RATE), "-b", str(bps), "-T",
                    str(n), path], input=tta_cases.pcm_bytes(x, bps),
                   stdout=subprocess.DEVNULL, check=True)
    with open(path, "rb") as f:
        assert f.read() == tta_port.encode(x, ch, bps, tta_cases.RATE)[0]
