"""GPU: audiotools.tta.TrueAudio, the container class over the GPU codec:
round trips, both from_pcm paths, convert to and from the other formats,
verify, and a file behind an ID3v2 comment."""
import hashlib
import json
import os

import numpy as np
import pytest

import signals
import tta_cases
import tta_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "tta_vectors.json")))
RATE = tta_cases.RATE


def reader(x, ch, bps, rate=RATE, mask=0):
    import audiotools
    return audiotools.FrameListReader(x, rate, ch, bps, mask)


def drain(pcmreader):
    got = []
    while True:
        fl = pcmreader.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    pcmreader.close()
    return np.concatenate(got) if got else np.zeros(0, np.int32)


@pytest.mark.parametrize("ch,bps", [(1, 8), (2, 16), (2, 24), (3, 16), (6, 24)])
def test_round_trip(tmp_path, ch, bps):
    """GPU encode -> GPU decode, and the file is the one tta_port writes"""
    from audiotools import TrueAudio
    n = tta_cases.BLOCK + 321
    x = signals.make("tone", n, ch, bps, seed=ch * bps)
    fn = str(tmp_path / "rt.tta")
    t = TrueAudio.from_pcm(fn, reader(x, ch, bps), total_pcm_frames=n)
    assert (t.channels(), t.bits_per_sample(), t.sample_rate(), t.total_frames()) == \
        (ch, bps, RATE, n)
    assert t.lossless() and int(t.channel_mask()) == {1: 0x4, 2: 0x3}.get(ch, 0)
    data = open(fn, "rb").read()
    assert data == tta_port.encode(x, ch, bps, RATE)[0]
    assert t.data_size() == len(data)
    assert np.array_equal(drain(t.to_pcm()), x)


def test_from_pcm_paths_agree(tmp_path):
    """with total_pcm_frames (seektable rewritten in place) and without
    (frames through a temporary file): identical files"""
    from audiotools import TrueAudio
    n = 2 * tta_cases.BLOCK + 100
    x = signals.make("tone", n, 2, 16, seed=8)
    a, b = str(tmp_path / "a.tta"), str(tmp_path / "b.tta")
    TrueAudio.from_pcm(a, reader(x, 2, 16), total_pcm_frames=n)
    TrueAudio.from_pcm(b, reader(x, 2, 16))
    da = open(a, "rb").read()
    assert da == open(b, "rb").read()
    assert da == tta_port.encode(x, 2, 16, RATE)[0]


@pytest.mark.parametrize("claimed", [999, 1001, 1000 + tta_cases.BLOCK])
def test_wrong_total_pcm_frames(tmp_path, claimed):
    from audiotools import EncodingError, TrueAudio
    x = signals.make("tone", 1000, 2, 16, seed=1)
    fn = str(tmp_path / "bad.tta")
    with pytest.raises(EncodingError):
        TrueAudio.from_pcm(fn, reader(x, 2, 16), total_pcm_frames=claimed)
    assert not os.path.exists(fn)


def test_reader_error_leaves_no_file(tmp_path):
    from audiotools import EncodingError, PCMReaderError, TrueAudio
    for total in (None, 10):
        fn = str(tmp_path / "err.tta")
        with pytest.raises(EncodingError):
            TrueAudio.from_pcm(fn, PCMReaderError("broken", RATE, 2, 0x3, 16),
                               total_pcm_frames=total)
        assert not os.path.exists(fn)


def test_convert_from_wave_and_to_flac(tmp_path):
    from audiotools import FlacAudio, TrueAudio, WaveAudio
    n = 44100 + 777
    x = signals.make("tone", n, 2, 16, seed=12)
    wav = WaveAudio.from_pcm(str(tmp_path / "s.wav"), reader(x, 2, 16, 44100, 0x3))
    tta = wav.convert(str(tmp_path / "s.tta"), TrueAudio)
    assert isinstance(tta, TrueAudio) and tta.total_frames() == n and tta.sample_rate() == 44100
    assert np.array_equal(drain(tta.to_pcm()), x)
    flac = tta.convert(str(tmp_path / "s.flac"), FlacAudio, "8")
    assert flac.total_frames() == n
    assert np.array_equal(drain(flac.to_pcm()), x)
    assert tta == flac and tta == wav


def test_convert_from_alac(tmp_path):
    from audiotools import ALACAudio, TrueAudio
    n = 9000
    x = signals.make("tone", n, 2, 16, seed=13)
    m4a = ALACAudio.from_pcm(str(tmp_path / "s.m4a"), reader(x, 2, 16, 44100, 0x3))
    tta = m4a.convert(str(tmp_path / "s.tta"), TrueAudio)
    assert np.array_equal(drain(tta.to_pcm()), x)


def test_verify(tmp_path):
    from audiotools import InvalidFile, TrueAudio
    n = tta_cases.BLOCK + 50
    x = signals.make("noise", n, 2, 16, seed=14)
    fn = str(tmp_path / "v.tta")
    t = TrueAudio.from_pcm(fn, reader(x, 2, 16), total_pcm_frames=n)
    assert t.verify() is True
    data = bytearray(open(fn, "rb").read())
    for at in (len(data) - 100, 12):  # a frame's payload; the header's rate
        bad = bytearray(data)
        bad[at] ^= 0x10
        fb = str(tmp_path / ("bad%d.tta" % at))
        open(fb, "wb").write(bytes(bad))
        with pytest.raises(InvalidFile):
            TrueAudio(fb).verify()


def test_invalid_files(tmp_path):
    from audiotools import InvalidTTA, TrueAudio
    good = tta_port.build_file([], 2, 16, RATE, 0)
    for name, data in (("sig", b"TTA2" + good[4:]), ("fmt", good[:4] + b"\2\0" + good[6:]),
                       ("short", good[:10])):
        fn = str(tmp_path / (name + ".tta"))
        open(fn, "wb").write(data)
        with pytest.raises(InvalidTTA):
            TrueAudio(fn)
    with pytest.raises(InvalidTTA):
        TrueAudio(str(tmp_path / "absent.tta"))


def test_id3v2_prefix():
    """the reference's fixture: a .tta file behind an ID3v2 comment"""
    from audiotools import TrueAudio
    t = TrueAudio(os.path.join(HERE, "golden", "fixtures", "tta-id3-2.tta"))
    assert (t.channels(), t.bits_per_sample(), t.sample_rate(), t.total_frames()) == \
        (2, 16, 96000, 96000)
    pcm = drain(t.to_pcm())
    v = G["decoder"]["tta-id3-2.tta"]
    raw = tta_cases.pcm_bytes(pcm, 16)
    assert len(raw) == v["bytes"] and hashlib.md5(raw).hexdigest() == v["md5"]
    assert t.verify() is True


def test_class_attributes():
    from audiotools import InvalidFile, InvalidTTA, TrueAudio
    assert TrueAudio.SUFFIX == TrueAudio.NAME == "tta" and TrueAudio.DESCRIPTION
    assert issubclass(InvalidTTA, InvalidFile)
