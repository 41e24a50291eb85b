"""GPU: audiotools.decoders.OggFlacDecoder and audiotools.OggFlacAudio, the
reference's interfaces (src/decoders/oggflac.c:53-283, audiotools/flac.py:
3040-3246) over the GPU decoder: the read loop, error types and messages,
verify, and a convert to FlacAudio that decodes back to the source."""
import numpy as np
import pytest

import oggflac_cases as cases
import oggflac_port as op

pytestmark = pytest.mark.gpu


def write(tmp_path, image, name="a.oga"):
    fn = str(tmp_path / name)
    with open(fn, "wb") as f:
        f.write(image)
    return fn


def test_read_loop(tmp_path):
    from audiotools import decoders
    img = cases.edge_cases()["lacing:junk_tail"]
    want = op.decode(img)
    d = decoders.OggFlacDecoder(write(tmp_path, img), 0x3)
    assert (d.sample_rate, d.bits_per_sample, d.channels, d.channel_mask) == (44100, 16, 2, 0x3)
    got = []
    for _ in range(want["n_frames"]):
        fl = d.read(4096)
        assert fl.frames == 192 and fl.channels == 2 and fl.bits_per_sample == 16
        got.append(fl.samples)
    assert np.array_equal(np.concatenate(got), want["samples"])
    assert len(d.read(4096)) == 0 and len(d.read(4096)) == 0
    d.close()
    with pytest.raises(ValueError, match="cannot read closed stream"):
        d.read(4096)


READ_ERRORS = [
    ("lacing:empty_packet", IOError, "I/O error decoding FLAC frame", 2),
    ("lacing:cut1", IOError, "I/O error decoding FLAC frame", 2),
    ("lacing:two_frames", ValueError, "MD5 mismatch at end of stream", 5),
    ("end:md5_wrong", ValueError, "MD5 mismatch at end of stream", 6),
    ("end:no_eos", IOError, "premature EOF reading Ogg stream", 6),
]


@pytest.mark.parametrize("name,kind,message,frames", READ_ERRORS)
def test_read_errors(tmp_path, name, kind, message, frames):
    from audiotools import decoders
    d = decoders.OggFlacDecoder(write(tmp_path, cases.edge_cases()[name]), 0x3)
    for _ in range(frames):
        assert d.read(4096).frames == 192
    with pytest.raises(kind) as e:
        d.read(4096)
    assert str(e.value) == message and type(e.value) is kind


def test_damaged_frame_and_page_messages(tmp_path):
    from audiotools import decoders
    pk, img = cases.damage_base()
    pk = list(pk)
    a = 1 + op.flac_packets(cases.source("allframes"))[1]  # the first audio packet
    bad = op.mux(pk[:a + 1] + [cases.flip(pk[a + 1], 3)] + pk[a + 2:], segs_per_page=3)
    d = decoders.OggFlacDecoder(write(tmp_path, bad), 0x4)
    d.read(4096)
    with pytest.raises(ValueError, match="invalid sync code"):
        d.read(4096)
    # a page checksum after the header pages
    pages = op.read_pages(img)[0]
    b = bytearray(img)
    b[pages[-1][0] + 30] ^= 1
    d = decoders.OggFlacDecoder(write(tmp_path, bytes(b), "b.oga"), 0x4)
    with pytest.raises(ValueError, match="checksum mismatch"):
        for _ in range(10):
            d.read(4096)


INIT_ERRORS = [
    ("header:page_magic", ValueError, "invalid magic number"),
    ("header:page_version", ValueError, "invalid stream version"),
    ("header:page_crc", ValueError, "checksum mismatch"),
    ("header:empty_file", IOError, "premature EOF reading Ogg stream"),
    ("header:no_packets", IOError, "stream finished"),
    ("header:count_60000", IOError, "stream finished"),
    ("header:packet_byte", ValueError, "invalid packet byte"),
    ("header:signature", ValueError, "invalid Ogg signature"),
    ("header:major", ValueError, "invalid major version"),
    ("header:minor", ValueError, "invalid minor version"),
    ("header:flac_signature", ValueError, "invalid fLaC signature"),
    ("header:block_type", ValueError, "invalid block type"),
    ("header:short20", IOError, "EOF while reading STREAMINFO block"),
]


@pytest.mark.parametrize("name,kind,message", INIT_ERRORS)
def test_init_errors(tmp_path, name, kind, message):
    from audiotools import decoders
    with pytest.raises(kind) as e:
        decoders.OggFlacDecoder(write(tmp_path, cases.header_cases()[name]), 0x3)
    assert str(e.value) == message and type(e.value) is kind


def test_init_arguments(tmp_path):
    from audiotools import decoders
    fn = write(tmp_path, cases.header_cases()["header:good"])
    with pytest.raises(ValueError, match="channel_mask must be >= 0"):
        decoders.OggFlacDecoder(fn, -1)
    with pytest.raises(TypeError):
        decoders.OggFlacDecoder(fn, "3")
    with pytest.raises(TypeError):
        decoders.OggFlacDecoder(fn)
    with pytest.raises(IOError):
        decoders.OggFlacDecoder(str(tmp_path / "missing.oga"), 0)


def test_oggflacaudio(tmp_path):
    import audiotools
    src = cases.source("t2x16")
    pk, _ = op.flac_packets(src)
    a = audiotools.OggFlacAudio(write(tmp_path, op.mux(pk, segs_per_page=40, seed=5)))
    assert (a.channels(), a.bits_per_sample(), a.sample_rate(), a.total_frames()) == \
        (2, 16, 44100, 700 * 192)
    assert a.lossless() and int(a.channel_mask()) == 0x3
    assert a.verify() is True
    want = op.decode(open(a.filename, "rb").read())["samples"]
    r = a.to_pcm()
    got = []
    while True:
        fl = r.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    assert np.array_equal(np.concatenate(got), want)
    # convert to FLAC and back
    flac = a.convert(str(tmp_path / "b.flac"), audiotools.FlacAudio)
    assert isinstance(flac, audiotools.FlacAudio) and flac.total_frames() == a.total_frames()
    assert flac == a
    with pytest.raises(audiotools.EncodingError):
        audiotools.OggFlacAudio.from_pcm(str(tmp_path / "c.oga"), a.to_pcm())
    with pytest.raises(audiotools.EncodingError):
        flac.convert(str(tmp_path / "d.oga"), audiotools.OggFlacAudio)


def test_verify_and_to_pcm_of_damaged_files(tmp_path):
    import audiotools
    e = cases.edge_cases()
    a = audiotools.OggFlacAudio(write(tmp_path, e["end:md5_wrong"]))
    with pytest.raises(audiotools.InvalidFile, match="MD5 mismatch at end of stream"):
        a.verify()
    a = audiotools.OggFlacAudio(write(tmp_path, e["lacing:cut100"], "b.oga"))
    with pytest.raises(audiotools.InvalidFile, match="I/O error decoding FLAC frame"):
        a.verify()
    # a file that changes under the object: to_pcm hands back a PCMReaderError
    fn = write(tmp_path, cases.header_cases()["header:good"], "c.oga")
    a = audiotools.OggFlacAudio(fn)
    write(tmp_path, cases.header_cases()["header:count_60000"], "c.oga")
    r = a.to_pcm()
    assert isinstance(r, audiotools.PCMReaderError) and r.channels == 2
