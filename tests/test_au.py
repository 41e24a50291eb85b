"""CPU: audiotools.au (reference audiotools/au.py) against the stdlib sunau
module both ways at 8, 16 and 24 bits, and the reference's AUFileTest
(test/test_formats.py:2907-3003) restated: channel masks, truncation,
convert() of a cut file; header errors, an annotation field, pcm_split,
unsupported bits per sample."""
import os
import struct

import numpy as np
import pytest

import audiotools
from audiotools import _atgpu, au
from audiotools.m4a import UnsupportedBitsPerSample
from test_aiff import Reader, make_pcm, read_all


def sunau_samples(path):
    sunau = pytest.importorskip("sunau")
    with sunau.open(path, "rb") as a:
        ch, width, rate, n = a.getnchannels(), a.getsampwidth(), a.getframerate(), a.getnframes()
        raw = a.readframes(n)
    u = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width).astype(np.int64)
    v = np.zeros(len(u), dtype=np.int64)
    for k in range(width):
        v = (v << 8) | u[:, k]
    v = np.where(v >= 1 << (8 * width - 1), v - (1 << (8 * width)), v)
    return ch, 8 * width, rate, n, v.astype(np.int32)


@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_from_pcm_read_by_sunau(tmp_path, channels, bits):
    for frames in (0, 1, 333):
        pcm = make_pcm(frames, channels, bits, seed=3)
        path = str(tmp_path / ("f%d.au" % frames))
        src = Reader(pcm, channels, bits, 32000, step=50)
        a = audiotools.AuAudio.from_pcm(path, src)
        assert src.closed
        data = open(path, "rb").read()
        assert len(data) == 24 + frames * channels * bits // 8
        assert struct.unpack(">4s5I", data[:24]) == (
            b".snd", 24, len(data) - 24, {8: 2, 16: 3, 24: 4}[bits], 32000, channels)
        assert (a.channels(), a.bits_per_sample(), a.sample_rate(), a.total_frames()) == (
            channels, bits, 32000, frames)
        assert a.lossless() and a.verify() is True
        assert np.array_equal(read_all(a.to_pcm(), 17), pcm)
        assert sunau_samples(path) == (channels, bits, 32000, frames, pytest.approx(pcm))
        st, info = _atgpu.au_read_info(data)
        assert st == 0 and (info.channels, info.bits_per_sample, info.sample_rate,
                            info.total_pcm_frames, info.data_offset, info.data_size,
                            info.data_bytes) == (channels, bits, 32000, frames, 24,
                                                 len(data) - 24, len(data) - 24)


@pytest.mark.parametrize("channels,width", [(1, 1), (2, 2), (2, 3), (4, 2)])
def test_reads_what_sunau_writes(tmp_path, channels, width):
    sunau = pytest.importorskip("sunau")
    bits = 8 * width
    pcm = make_pcm(257, channels, bits, seed=9)
    raw = audiotools.pcm.FrameList._wrap(pcm, channels, bits).to_bytes(True, True)
    path = str(tmp_path / "w.au")
    with sunau.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(8000)
        w.setcomptype("NONE", "not compressed")
        w.writeframes(raw)
    r = au.AuReader(path)
    assert (r.channels, r.bits_per_sample, r.sample_rate, r.total_pcm_frames) == (
        channels, bits, 8000, 257)
    assert r.channel_mask == {1: 0x4, 2: 0x3}.get(channels, 0)
    assert np.array_equal(read_all(r, 100), pcm)
    r.close()


def test_channel_mask(tmp_path):
    """AUFileTest.test_channel_mask"""
    path = str(tmp_path / "m.au")
    for channels, mask in ((1, 0x4), (2, 0x3)):
        track = audiotools.AuAudio.from_pcm(path, Reader(np.zeros(channels), channels, 16))
        assert track.channels() == channels and track.channel_mask() == mask
        track = audiotools.AuAudio(path)
        assert track.channels() == channels and track.channel_mask() == mask
    for channels in (3, 4, 5, 6):
        track = audiotools.AuAudio.from_pcm(path, Reader(np.zeros(channels), channels, 16))
        assert track.channels() == channels and track.channel_mask() == 0
        track = audiotools.AuAudio(path)
        assert track.channels() == channels and track.channel_mask() == 0


def test_verify_truncated(tmp_path):
    """AUFileTest.test_verify"""
    path, out = str(tmp_path / "t.au"), str(tmp_path / "dummy.wav")
    track = audiotools.AuAudio.from_pcm(path, Reader(make_pcm(44100, 2, 16), 2, 16))
    good = open(path, "rb").read()
    open(path, "wb").write(good[:-10])
    reader = track.to_pcm()
    with pytest.raises(IOError, match="truncated data block"):
        audiotools.transfer_framelist_data(reader, lambda x: x)
    reader.close()
    with pytest.raises(audiotools.InvalidFile):
        track.verify()
    with pytest.raises(audiotools.EncodingError):
        track.convert(out, audiotools.WaveAudio)
    assert not os.path.isfile(out)
    # frame by frame: the error at exactly the first read past the end
    reader = track.to_pcm()
    for _ in range(44100 - 3):
        assert reader.read(1).frames == 1
    with pytest.raises(IOError):
        reader.read(1)
    reader.close()


def _image(magic=b".snd", offset=24, size=12, encoding=3, rate=44100, channels=2, extra=b""):
    return struct.pack(">4s5I", magic, offset, size, encoding, rate, channels) + extra


def test_header_errors(tmp_path):
    path = str(tmp_path / "bad.au")
    for image, message, status in (
            (_image(magic=b".snx"), "invalid Sun AU header", _atgpu.AU_INVALID_HEADER),
            (_image(encoding=1), "unsupported Sun AU format", _atgpu.AU_UNSUPPORTED_FORMAT),
            (_image(encoding=6), "unsupported Sun AU format", _atgpu.AU_UNSUPPORTED_FORMAT)):
        open(path, "wb").write(image + bytes(12))
        with pytest.raises(audiotools.InvalidFile, match=message):
            audiotools.AuAudio(path)
        with pytest.raises(ValueError, match=message):
            au.AuReader(path)
        assert _atgpu.au_read_info(image)[0] == status
    open(path, "wb").write(_image()[:20])
    with pytest.raises(audiotools.InvalidFile):
        audiotools.AuAudio(path)
    assert _atgpu.au_read_info(_image()[:20])[0] == _atgpu.AU_IOERROR


def test_annotation_field_and_pcm_split(tmp_path):
    note = b"a note.\0"
    samples = np.array([1, -2, 300, -400, 32767, -32768], dtype=np.int32)
    raw = audiotools.pcm.FrameList._wrap(samples, 2, 16).to_bytes(True, True)
    path = str(tmp_path / "note.au")
    open(path, "wb").write(_image(offset=24 + len(note), size=len(raw)) + note + raw)
    a = audiotools.AuAudio(path)
    assert a.total_frames() == 3
    r = a.to_pcm()
    assert r.data_offset == 32 and np.array_equal(read_all(r), samples)
    assert r.seek(1) == 1 and np.array_equal(read_all(r), samples[2:])
    assert r.seek(99) == 3 and r.read(1).frames == 0
    with pytest.raises(ValueError, match="cannot seek to negative value"):
        r.seek(-1)
    r.close()
    head, tail = a.pcm_split()
    assert head == open(path, "rb").read()[:32] and tail == b""
    assert a.verify() is True
    st, info = _atgpu.au_read_info(open(path, "rb").read())
    assert st == 0 and (info.data_offset, info.data_size, info.data_bytes) == (32, 12, 12)


def test_unsupported_bits_per_sample(tmp_path):
    path = str(tmp_path / "x.au")
    with pytest.raises(UnsupportedBitsPerSample):
        audiotools.AuAudio.from_pcm(path, Reader(np.zeros(4), 2, 32))
    with pytest.raises(audiotools.EncodingError):
        audiotools.AuAudio.from_pcm(path, Reader(np.zeros(4), 2, 20))
    assert not os.path.isfile(path)
