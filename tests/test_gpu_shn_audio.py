"""GPU: audiotools.shn.ShortenAudio, the container class over the GPU codec,
and the encode_shn / SHNDecoder interfaces under it: both from_pcm paths,
from_wave with foreign chunks, the reference's fixtures, a truncated file and
a refused bit depth."""
import os
import struct

import numpy as np
import pytest

import shn_cases
import shn_port
import signals

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RATE = 44100


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


@pytest.mark.parametrize("ch,bps", [(1, 8), (2, 16), (3, 16)])
def test_from_pcm_with_total(tmp_path, ch, bps):
    """a generated wave header in the VERBATIM command; the file is the one
    shn_port writes"""
    from audiotools import ShortenAudio
    from audiotools.wav import wave_header
    n = 2 * 256 + 99
    x = signals.make("tone", n, ch, bps, seed=ch + bps)
    fn = str(tmp_path / "a.shn")
    mask = {1: 0x4, 2: 0x3, 3: 0x7}[ch]
    s = ShortenAudio.from_pcm(fn, reader(x, ch, bps, mask=mask), total_pcm_frames=n)
    assert (s.channels(), s.bits_per_sample(), s.sample_rate(), s.total_frames()) == \
        (ch, bps, RATE, n)
    assert s.lossless() and int(s.channel_mask()) == mask
    header = wave_header(RATE, ch, mask, bps, n)
    footer = b"\x00" * ((bps // 8 * ch * n) % 2)
    want = shn_port.encode(x, ch, bps, 256, False, bps == 16, header, footer)
    assert open(fn, "rb").read() == want
    assert np.array_equal(drain(s.to_pcm()), x)
    assert s.wave_header_footer() == (header, footer)
    assert not s.has_foreign_wave_chunks()


def test_from_pcm_without_total(tmp_path):
    """through a temporary wave file: the same file as with the total"""
    from audiotools import ShortenAudio
    n = 700
    x = signals.make("noise", n, 2, 16, seed=4)
    a, b = str(tmp_path / "a.shn"), str(tmp_path / "b.shn")
    ShortenAudio.from_pcm(a, reader(x, 2, 16, mask=3), total_pcm_frames=n)
    s = ShortenAudio.from_pcm(b, reader(x, 2, 16, mask=3), block_size=256)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert s.total_frames() == n and np.array_equal(drain(s.to_pcm()), x)


def test_from_wave_foreign_chunks(tmp_path):
    from audiotools import EncodingError, ShortenAudio
    n = 300
    x = signals.make("tone", n, 2, 16, seed=6)
    fmt = struct.pack("<HHIIHH", 1, 2, RATE, RATE * 4, 4, 16)
    foreign = b"LIST" + struct.pack("<I", 4) + b"abcd"
    tail = b"cue " + struct.pack("<I", 2) + b"xy"
    body = (b"WAVE" + foreign + b"fmt " + struct.pack("<I", 16) + fmt + b"data" +
            struct.pack("<I", n * 4))
    header = b"RIFF" + struct.pack("<I", len(body) + n * 4 + len(tail)) + body
    fn = str(tmp_path / "f.shn")
    s = ShortenAudio.from_wave(fn, header, reader(x, 2, 16), tail)
    assert s.wave_header_footer() == (header, tail)
    assert s.has_foreign_wave_chunks()
    assert s.total_frames() == n and s.sample_rate() == RATE
    assert np.array_equal(drain(s.to_pcm()), x)
    # a header whose data chunk names another size is refused, the file removed
    with pytest.raises(EncodingError):
        ShortenAudio.from_wave(fn, header, reader(x[:100], 2, 16), tail)
    assert not os.path.exists(fn)


@pytest.mark.parametrize("name", shn_cases.FIXTURES)
def test_to_pcm_of_fixtures(name):
    from audiotools import ShortenAudio
    path = os.path.join(HERE, "golden", "fixtures", name)
    s = ShortenAudio(path)
    assert (s.channels(), s.bits_per_sample(), s.sample_rate(), s.total_frames()) == \
        (1, 16, 44100, 100)
    want = shn_port.decode(open(path, "rb").read())
    r = s.to_pcm()
    first = r.read(4096)
    assert first.frames == 20  # one block per read
    assert np.array_equal(np.concatenate([first.samples, drain(r)]), want[1])
    head, tail = s.wave_header_footer()
    assert (head, tail) == (want[3], want[4])


def test_decoder_interface_and_errors(tmp_path):
    from audiotools import InvalidShorten, ShortenAudio
    from audiotools.decoders import SHNDecoder, decode_shn_batch
    img = open(os.path.join(HERE, "golden", "fixtures", "shorten-lpc.shn"), "rb").read()
    d = SHNDecoder(img)
    assert (d.sample_rate, d.bits_per_sample, d.channels, d.channel_mask) == (44100, 16, 1, 0x4)
    assert d.pcm_split() == shn_port.pcm_split(img)
    for _ in range(5):
        assert d.read(4096).frames == 20
    assert d.read(4096).frames == 0 and d.read(4096).frames == 0
    d.close()
    with pytest.raises(ValueError):
        d.read(4096)
    # a truncated file: the blocks before the cut, then IOError
    cut, want = None, None
    for k in range(len(img) - 1, 0, -1):
        want = shn_port.decode(img[:k])
        if want[0] == shn_port.IOERROR and 0 < len(want[1]) < 100:
            cut = img[:k]
            break
    assert cut is not None
    fn = str(tmp_path / "cut.shn")
    open(fn, "wb").write(cut)
    r = ShortenAudio(fn).to_pcm()
    got = []
    with pytest.raises(IOError) as e:
        while True:
            got.append(r.read(4096).samples)
    assert str(e.value) == "I/O error reading Shorten file"
    assert np.array_equal(np.concatenate(got) if got else np.zeros(0, np.int32), want[1])
    with pytest.raises(IOError):
        SHNDecoder(cut).pcm_split()
    # header errors, with the reference's messages
    for data, kind, msg in ((b"ajkx" + img[4:], ValueError, "invalid magic number"),
                            (img[:4] + b"\x03" + img[5:], ValueError, "invalid Shorten version"),
                            (img[:9], IOError, "I/O error reading Shorten header")):
        with pytest.raises(kind) as e:
            SHNDecoder(data)
        assert str(e.value) == msg
    bad = shn_port.Builder(7, 1, 4).quit()
    with pytest.raises(ValueError) as e:
        SHNDecoder(bad)
    assert str(e.value) == "unsupported Shorten file type"
    unknown = shn_cases.builder_streams()["unknown_command"]
    d = SHNDecoder(unknown)
    assert d.read(1).frames == 10
    with pytest.raises(ValueError) as e:
        d.read(1)
    assert str(e.value) == "unknown command in Shorten stream"
    open(fn, "wb").write(b"ajk")
    with pytest.raises(InvalidShorten):
        ShortenAudio(fn)
    batch = decode_shn_batch([img, cut])
    assert [b[0] for b in batch] == [shn_port.END_OF_STREAM, shn_port.IOERROR]


def test_encode_shn_interface(tmp_path):
    """the reference's signature; short reads become BLOCKSIZE commands"""
    import audiotools
    from audiotools.encoders import encode_shn, encode_shn_batch
    x = signals.make("tone", 600, 2, 16, seed=12)
    fn = str(tmp_path / "e.shn")
    encode_shn(fn, reader(x, 2, 16), False, True, b"hdr", b"ftr", 100)
    assert open(fn, "rb").read() == shn_port.encode(x, 2, 16, 100, False, True, b"hdr", b"ftr")

    class Short(audiotools.FrameListReader):
        """returns 70, then 30, frames however many are asked for"""
        turn = 0

        def read(self, n):
            self.turn += 1
            return audiotools.FrameListReader.read(self, 70 if self.turn % 2 else 30)

    encode_shn(fn, Short(x, RATE, 2, 16, 0), True, False, b"")
    sizes = [70, 30] * 6
    assert open(fn, "rb").read() == shn_port.encode(x, 2, 16, 256, True, False, b"", b"", sizes)
    a, b = str(tmp_path / "a.shn"), str(tmp_path / "b.shn")
    y = signals.make("noise", 123, 2, 16, seed=1)
    encode_shn_batch([a, b], [reader(x, 2, 16), reader(y, 2, 16)], False, True, [b"A", b""])
    assert open(a, "rb").read() == shn_port.encode(x, 2, 16, header=b"A")
    assert open(b, "rb").read() == shn_port.encode(y, 2, 16)


def test_24_bit_refused(tmp_path):
    from audiotools import ShortenAudio
    from audiotools.encoders import encode_shn
    from audiotools.m4a import UnsupportedBitsPerSample
    x = signals.make("tone", 100, 2, 24, seed=2)
    fn = str(tmp_path / "x.shn")
    with pytest.raises(UnsupportedBitsPerSample):
        ShortenAudio.from_pcm(fn, reader(x, 2, 24), total_pcm_frames=100)
    with pytest.raises(UnsupportedBitsPerSample):
        ShortenAudio.from_pcm(fn, reader(x, 2, 24))
    with pytest.raises(ValueError) as e:
        encode_shn(fn, reader(x, 2, 24), False, True, b"")
    assert str(e.value) == "unsupported bits per sample"
    assert not os.path.exists(fn)
