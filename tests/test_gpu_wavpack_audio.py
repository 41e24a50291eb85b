"""GPU: audiotools.decoders.WavPackDecoder (read set by set, seek, close) and
audiotools.wavpack.WavPackAudio, the container class over the GPU decoder:
fields, verify, convert to the other formats."""
import io
import os

import numpy as np
import pytest

import wavpack_cases as cases
import wavpack_port as port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G, IMAGES = cases.load_vectors()
SRC = {c[0]: c for c in cases.cases()}


def drain(pcmreader):
    got = []
    while True:
        fl = pcmreader.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    pcmreader.close()
    return np.concatenate(got) if got else np.zeros(0, np.int32)


def write(tmp_path, name, data):
    fn = str(tmp_path / name)
    with open(fn, "wb") as f:
        f.write(data)
    return fn


def find_sub_block(img, off, size, function):
    """offset of the payload of a block's first sub-block with this id"""
    pos = off
    while pos < off + size:
        hdr = 4 if img[pos] & 0x80 else 2
        words = img[pos + 1] if hdr == 2 else int.from_bytes(img[pos + 1:pos + 4], "little")
        if img[pos] & 0x3F == function:
            return pos + hdr
        pos += hdr + 2 * words
    raise AssertionError("sub-block not found")


def test_read_set_by_set():
    """three sets of 50, 50 and 20 frames over three channels"""
    from audiotools import decoders
    name = "chan3"
    x = SRC[name][5]
    d = decoders.WavPackDecoder(io.BytesIO(IMAGES[name]))
    assert (d.sample_rate, d.bits_per_sample, d.channels, d.channel_mask) == (44100, 16, 3, 7)
    sizes, got = [], []
    for _ in range(3):
        fl = d.read(4096)
        sizes.append(fl.frames)
        got.append(fl.samples)
        assert fl.channels == 3 and fl.bits_per_sample == 16
    assert sizes == [50, 50, 20]
    assert np.array_equal(np.concatenate(got), x)
    assert len(d.read(4096)) == 0 and len(d.read(4096)) == 0
    d.close()
    with pytest.raises(ValueError, match="cannot read closed stream"):
        d.read(4096)
    with pytest.raises(ValueError, match="cannot seek closed stream"):
        d.seek(0)


def test_error_raised_at_the_bad_set():
    from audiotools import decoders
    img = bytearray(IMAGES[cases.DAMAGE_STEREO])
    st, info, sets, end = port.read_info(bytes(img))
    off, size = sets[1][0]["data"]
    img[off + size - 5] ^= 0x20               # inside the second set's bitstream
    want_status = port.decode(bytes(img))[0]
    assert want_status == port.BLOCK_DATA_CRC_MISMATCH
    d = decoders.WavPackDecoder(bytes(img))
    assert d.read(4096).frames == 200
    with pytest.raises(ValueError, match="block data CRC mismatch"):
        d.read(4096)
    # a file that ends inside a block: IOError at the set it ends in
    cut = IMAGES[cases.DAMAGE_STEREO][:sets[2][0]["offset"] + 40]
    d = decoders.WavPackDecoder(cut)
    assert d.read(1).frames == 200 and d.read(1).frames == 200
    with pytest.raises(IOError, match="I/O error reading block data"):
        d.read(1)
    with pytest.raises(ValueError, match="invalid block header ID"):
        decoders.WavPackDecoder(b"RIFF" + cut[4:])
    with pytest.raises(IOError, match="I/O error"):
        decoders.WavPackDecoder(cut[:20])


def test_md5_mismatch_raised_once_at_the_end():
    """the int32 info patched so that the CRC still holds and the PCM differs"""
    from audiotools import decoders
    img = bytearray(IMAGES["wasted5_c2"])
    st, info, sets, end = port.read_info(bytes(img))
    for blocks in sets:
        off, size = blocks[0]["data"]
        at = find_sub_block(img, off, size, 9)
        img[at + 1] = 4                        # zero bits 5 -> 4
    assert port.decode(bytes(img))[0] == port.MD5_MISMATCH
    d = decoders.WavPackDecoder(bytes(img))
    frames = [d.read(4096).frames for _ in range(3)]
    assert frames == [50, 50, 20]
    with pytest.raises(ValueError, match="MD5 mismatch at end of stream"):
        d.read(4096)
    assert len(d.read(4096)) == 0
    # an 8-bit stream's MD5 is over unsigned bytes: no error
    d = decoders.WavPackDecoder(IMAGES["tone_c2_b8"])
    assert np.array_equal(drain(d), SRC["tone_c2_b8"][5])


@pytest.mark.parametrize("name", ["chan3", "len22050_c2"])
def test_seek(name):
    from audiotools import decoders
    img, x = IMAGES[name], SRC[name][5]
    ch = SRC[name][2]
    d = decoders.WavPackDecoder(img)
    total = len(x) // ch
    first = d.read(4096)
    for offset in (0, 1, 49, 50, 51, 99, 100, 101, total // 2, total - 1, total, total + 1000):
        want, _ = port.seek_position(img, offset)
        assert d.seek(offset) == want, offset
        assert np.array_equal(drain_keep(d), x[want * ch:]), offset
    assert d.seek(0) == 0
    assert np.array_equal(d.read(4096).samples, first.samples)
    with pytest.raises(ValueError, match="cannot seek to negative value"):
        d.seek(-1)


def drain_keep(d):
    got = []
    while True:
        fl = d.read(4096)
        if not len(fl):
            break
        got.append(fl.samples)
    return np.concatenate(got) if got else np.zeros(0, np.int32)


def test_audio_fields_on_fixtures():
    from audiotools import WavPackAudio
    for name, frames in (("silence.wv", 220500), ("wavpack-combo.wv", 44200)):
        t = WavPackAudio(os.path.join(HERE, "golden", "fixtures", name))
        assert (t.channels(), t.bits_per_sample(), t.sample_rate(), t.total_frames()) == \
            (2, 16, 44100, frames)
        assert t.lossless() and int(t.channel_mask()) == 0x3
        assert t.verify() is True
    assert WavPackAudio.SUFFIX == WavPackAudio.NAME == "wv"


def test_audio_fields_multichannel(tmp_path):
    from audiotools import WavPackAudio
    t = WavPackAudio(write(tmp_path, "six.wv", IMAGES["chan6_b24_j"]))
    assert (t.channels(), t.bits_per_sample(), int(t.channel_mask()), t.total_frames()) == \
        (6, 24, 0x3F, 120)
    assert np.array_equal(drain(t.to_pcm()), SRC["chan6_b24_j"][5])
    t = WavPackAudio(write(tmp_path, "odd.wv", IMAGES["rate12345_c3"]))
    assert (t.sample_rate(), t.channels()) == (12345, 3)


def test_verify(tmp_path):
    from audiotools import InvalidFile, WavPackAudio
    good = IMAGES[cases.DAMAGE_STEREO]
    assert WavPackAudio(write(tmp_path, "good.wv", good)).verify() is True
    bad = bytearray(good)
    bad[len(bad) - 200] ^= 0x10                # the last set's bitstream
    assert port.decode(bytes(bad))[0] == port.BLOCK_DATA_CRC_MISMATCH
    with pytest.raises(InvalidFile):
        WavPackAudio(write(tmp_path, "bad.wv", bytes(bad))).verify()


def test_invalid_files(tmp_path):
    from audiotools import InvalidFile, InvalidWavPack, WavPackAudio
    assert issubclass(InvalidWavPack, InvalidFile)
    for name, data in (("sig", b"wvpK" + IMAGES["chan2"][4:]), ("short", IMAGES["chan2"][:16])):
        with pytest.raises(InvalidWavPack):
            WavPackAudio(write(tmp_path, name + ".wv", data))
    with pytest.raises(InvalidWavPack):
        WavPackAudio(str(tmp_path / "absent.wv"))


def test_convert_to_flac_tta_wave(tmp_path):
    from audiotools import FlacAudio, TrueAudio, WaveAudio, WavPackAudio
    name = "len22050_c2"
    x = SRC[name][5]
    wv = WavPackAudio(write(tmp_path, "s.wv", IMAGES[name]))
    flac = wv.convert(str(tmp_path / "s.flac"), FlacAudio, "8")
    assert flac.total_frames() == len(x) // 2
    assert np.array_equal(drain(flac.to_pcm()), x)
    tta = wv.convert(str(tmp_path / "s.tta"), TrueAudio)
    assert np.array_equal(drain(tta.to_pcm()), x)
    wav = wv.convert(str(tmp_path / "s.wav"), WaveAudio)
    assert np.array_equal(drain(wav.to_pcm()), x)
    assert wv == flac


def test_convert_to_alac(tmp_path):
    from audiotools import ALACAudio, WavPackAudio
    wv = WavPackAudio(write(tmp_path, "s.wv", IMAGES["tone_c2_b16"]))
    m4a = wv.convert(str(tmp_path / "s.m4a"), ALACAudio)
    assert np.array_equal(drain(m4a.to_pcm()), SRC["tone_c2_b16"][5])


def test_from_pcm_is_not_available(tmp_path):
    import audiotools
    from audiotools import EncodingError, WavPackAudio
    r = audiotools.FrameListReader(SRC["tone_c2_b16"][5], 44100, 2, 16, 0x3)
    with pytest.raises(EncodingError, match="WavPack encoding is not available"):
        WavPackAudio.from_pcm(str(tmp_path / "x.wv"), r)
    assert not os.path.exists(str(tmp_path / "x.wv"))
