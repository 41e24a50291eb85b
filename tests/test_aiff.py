"""CPU: audiotools.aiff (reference audiotools/aiff.py) against the
reference's seven aiff-*.aiff fixtures, the stdlib aifc module, and the
reference's own AiffFileTest (test/test_formats.py:1919-2042) restated:
the 80-bit sample rate field, COMM parsing (Python and libatgpu's C
parser), AiffReader, from_pcm, header/footer round trip, verify() and its
error cases, seek."""
import io
import os
import struct

import numpy as np
import pytest

import audiotools
from audiotools import _atgpu, aiff

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")
ALL = ["aiff-1ch", "aiff-2ch", "aiff-6ch", "aiff-8bit", "aiff-metadata", "aiff-misordered",
       "aiff-nossnd"]
# what the stdlib aifc module reports for the readable ones
AIFC_FRAMES = {"aiff-1ch": 20, "aiff-2ch": 20, "aiff-6ch": 20, "aiff-8bit": 9,
               "aiff-metadata": 20, "aiff-misordered": 25}

COMM = aiff.AIFF_Chunk(b"COMM", 18,
                       b"\x00\x01\x00\x00\x00\r\x00\x10@\x0e\xacD\x00\x00\x00\x00\x00\x00")
SSND = aiff.AIFF_Chunk(b"SSND", 34,
                       b"\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x01\x00\x02\x00\x03\x00\x02"
                       b"\x00\x01\x00\x00\xff\xff\xff\xfe\xff\xfd\xff\xfe\xff\xff\x00\x00")


def fixture(name):
    return os.path.join(FIX, name + ".aiff")


def read_all(reader, step=4096):
    parts = []
    while True:
        fl = reader.read(step)
        if not fl.frames:
            break
        parts.append(fl.samples)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


def aifc_samples(path):
    """(channels, bits, rate, frames, int32 interleaved samples) by aifc"""
    aifc = pytest.importorskip("aifc")
    with aifc.open(path, "rb") as a:
        ch, width, rate, n = a.getnchannels(), a.getsampwidth(), a.getframerate(), a.getnframes()
        raw = a.readframes(n)
    u = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width).astype(np.int64)
    v = np.zeros(len(u), dtype=np.int64)
    for k in range(width):
        v = (v << 8) | u[:, k]
    v = np.where(v >= 1 << (8 * width - 1), v - (1 << (8 * width)), v)
    return ch, 8 * width, rate, n, v.astype(np.int32)


class Reader(object):
    """a PCMReader over an int32 array, FrameLists of at most `step` frames"""

    def __init__(self, samples, channels, bits, rate=44100, step=1000):
        self.samples = np.asarray(samples, dtype=np.int32)
        self.channels, self.bits_per_sample, self.sample_rate = channels, bits, rate
        self.channel_mask = {1: 0x4, 2: 0x3}.get(channels, 0)
        self.step, self.pos, self.closed = step, 0, False

    def read(self, pcm_frames):
        n = min(max(pcm_frames, 1), self.step) * self.channels
        out = self.samples[self.pos:self.pos + n]
        self.pos += len(out)
        return audiotools.pcm.FrameList._wrap(out, self.channels, self.bits_per_sample)

    def close(self):
        self.closed = True


def make_pcm(frames, channels, bits, seed=0):
    rng = np.random.default_rng(seed + frames + 10 * channels + bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(lo, hi + 1, frames * channels, dtype=np.int64)
    v[:4] = [lo, hi, 0, -1][:len(v[:4])]
    return v.astype(np.int32)


def test_ieee_extended_round_trip():
    """AiffFileTest.test_ieee_extended: every rate 0 .. 192000"""
    for i in range(0, 192000 + 1):
        data = aiff.build_ieee_extended(float(i))
        assert len(data) == 10
        assert aiff.parse_ieee_extended(data) == i
    assert aiff.build_ieee_extended(44100) == bytes.fromhex("400EAC44000000000000")
    assert aiff.parse_ieee_extended(io.BytesIO(bytes.fromhex("400EAC44000000000000"))) == 44100
    with pytest.raises(IOError):
        aiff.parse_ieee_extended(b"\x40\x0e")


@pytest.mark.parametrize("name", ALL)
def test_c_parser_agrees_with_parse_comm(name):
    """the COMM chunk of every fixture: libatgpu's parser and parse_comm"""
    data = open(fixture(name), "rb").read()
    comm = next(c for c in audiotools.AiffAudio(fixture(name)).chunks() if c.id == b"COMM")
    ch, frames, bits, rate, mask = aiff.parse_comm(comm.data())
    st, info = _atgpu.aiff_read_info(data)
    if name == "aiff-nossnd":
        assert st == _atgpu.AIFF_NO_SSND
    else:
        assert st == _atgpu.AIFF_OK
        assert info.ssnd_data_offset + info.ssnd_data_bytes <= len(data)
        assert info.ssnd_data_bytes == frames * ch * bits // 8
        # in aiff-misordered the sound data comes before COMM
        assert info.ssnd_data_offset == (28 if name == "aiff-misordered" else 54)
    assert (info.channels, info.total_pcm_frames, info.bits_per_sample, info.sample_rate,
            info.channel_mask) == (ch, frames, bits, rate, int(mask))


@pytest.mark.parametrize("name", sorted(AIFC_FRAMES))
def test_reader_matches_aifc(name):
    """the fixtures through AiffReader: the parameters and frames aifc gives.
    In aiff-misordered the SSND chunk comes before COMM: the reader goes on
    to COMM and comes back to the sound data (the reference's refuses it)"""
    ch, bits, rate, n, want = aifc_samples(fixture(name))
    assert n == AIFC_FRAMES[name]
    r = aiff.AiffReader(fixture(name))
    assert (r.channels, r.bits_per_sample, r.sample_rate, r.total_pcm_frames) == (ch, bits, rate, n)
    assert r.channel_mask == {1: 0x4, 2: 0x3}.get(ch, 0)
    assert np.array_equal(read_all(r, 7), want)
    r.close()
    a = audiotools.AiffAudio(fixture(name))
    assert (a.channels(), a.bits_per_sample(), a.sample_rate(), a.total_frames()) == (
        ch, bits, rate, n)
    assert a.lossless() and int(a.channel_mask()) == r.channel_mask


def test_ssnd_without_comm_after_it_raises(tmp_path):
    """ "SSND chunk found before fmt" is left for a file with no COMM after
    its SSND chunk; a misordered file seeks, and verify() still refuses it"""
    path = str(tmp_path / "ssnd.aiff")
    with open(path, "wb") as f:
        audiotools.AiffAudio.aiff_from_chunks(f, [SSND])
    with pytest.raises(ValueError, match="SSND chunk found before fmt"):
        aiff.AiffReader(path)
    assert _atgpu.aiff_read_info(open(path, "rb").read())[0] == _atgpu.AIFF_PREMATURE_SSND
    r = aiff.AiffReader(fixture("aiff-misordered"))
    whole = read_all(r)
    assert r.seek(20) == 20 and np.array_equal(read_all(r), whole[20:])
    r.close()
    with pytest.raises(audiotools.InvalidFile, match="SSND chunk found before fmt"):
        audiotools.AiffAudio(fixture("aiff-misordered")).verify()


def test_nossnd_fails_verify():
    a = audiotools.AiffAudio(fixture("aiff-nossnd"))
    with pytest.raises(audiotools.InvalidFile, match="SSND chunk not found"):
        a.verify()
    with pytest.raises(ValueError, match="SSND chunk not found"):
        a.to_pcm()


@pytest.mark.parametrize("name", ["aiff-8bit", "aiff-1ch", "aiff-2ch", "aiff-6ch"])
def test_truncated_files(tmp_path, name):
    """AiffFileTest.test_verify: a cut COMM chunk fails at open, a cut SSND
    chunk at the read that passes the end of the file"""
    data = open(fixture(name), "rb").read()
    path = str(tmp_path / "cut.aiff")
    for i in range(0, 0x25):
        with open(path, "wb") as f:
            f.write(data[:i])
        with pytest.raises(audiotools.InvalidFile):
            audiotools.AiffAudio(path)
    for i in range(0x37, len(data)):
        with open(path, "wb") as f:
            f.write(data[:i])
        reader = audiotools.AiffAudio(path).to_pcm()
        with pytest.raises(IOError, match="premature end of SSND chunk"):
            audiotools.transfer_framelist_data(reader, lambda x: x)
        reader.close()
        # one frame at a time: the error comes at exactly the first read whose
        # bytes pass the end of the file
        reader = audiotools.AiffAudio(path).to_pcm()
        whole = (i - 0x36) // reader.bytes_per_pcm_frame
        for _ in range(whole):
            assert reader.read(1).frames == 1
        with pytest.raises(IOError):
            reader.read(1)
        reader.close()
        with pytest.raises(audiotools.InvalidFile):
            audiotools.AiffAudio(path).verify()
    if name != "aiff-8bit":  # whose odd SSND chunk has no pad byte
        assert audiotools.AiffAudio(fixture(name)).verify() is True


def padded_metadata():
    """aiff-metadata.aiff with the pad byte its last chunk (ID3, 29 bytes)
    lacks"""
    data = open(fixture("aiff-metadata"), "rb").read() + b"\0"
    return data[:4] + struct.pack(">I", len(data) - 8) + data[8:]


def test_verify_bad_chunk_id(tmp_path):
    """AiffFileTest.test_verify: byte 0x89, in the ID3 chunk's ID, zeroed"""
    path = str(tmp_path / "badid.aiff")
    data = bytearray(open(fixture("aiff-metadata"), "rb").read())
    data[0x89] = 0
    open(path, "wb").write(bytes(data))
    with pytest.raises(audiotools.InvalidFile):
        audiotools.AiffAudio(path).verify()
    # and on the well-formed copy, where the chunk ID is all that is wrong
    open(path, "wb").write(padded_metadata())
    assert audiotools.AiffAudio(path).verify() is True
    data = bytearray(padded_metadata())
    data[0x89] = 0
    open(path, "wb").write(bytes(data))
    with pytest.raises(audiotools.InvalidFile, match="invalid AIFF chunk ID"):
        audiotools.AiffAudio(path).verify()


@pytest.mark.parametrize("chunks", [[COMM, COMM, SSND], [COMM, SSND, SSND], [SSND, COMM],
                                    [SSND], [COMM]],
                         ids=["comm-comm-ssnd", "comm-ssnd-ssnd", "ssnd-comm", "ssnd", "comm"])
def test_verify_bad_chunk_orders(tmp_path, chunks):
    path = str(tmp_path / "order.aiff")
    with open(path, "wb") as f:
        audiotools.AiffAudio.aiff_from_chunks(f, chunks)
    with pytest.raises(audiotools.InvalidFile):
        audiotools.AiffAudio(path).verify()


def test_good_chunk_order_verifies(tmp_path):
    path = str(tmp_path / "good.aiff")
    with open(path, "wb") as f:
        audiotools.AiffAudio.aiff_from_chunks(f, [COMM, SSND])
    a = audiotools.AiffAudio(path)
    assert a.verify() is True and a.total_frames() == 13
    assert not a.has_foreign_aiff_chunks()
    assert [c.id for c in a.chunks()] == [b"COMM", b"SSND"]
    assert list(read_all(a.to_pcm())) == [0, 1, 2, 3, 2, 1, 0, -1, -2, -3, -2, -1, 0]


def test_convert_of_a_cut_file_leaves_nothing(tmp_path):
    path, out = str(tmp_path / "cut.aiff"), str(tmp_path / "dummy.wav")
    open(path, "wb").write(open(fixture("aiff-2ch"), "rb").read()[:-10])
    with pytest.raises(audiotools.EncodingError):
        audiotools.AiffAudio(path).convert(out, audiotools.WaveAudio)
    assert not os.path.isfile(out)


@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_from_pcm_read_back(tmp_path, channels, bits):
    for frames in (0, 1, 101, 1000):
        pcm = make_pcm(frames, channels, bits)
        path = str(tmp_path / ("f%d.aiff" % frames))
        src = Reader(pcm, channels, bits, 48000, step=64)
        a = audiotools.AiffAudio.from_pcm(path, src)
        assert src.closed
        data_bytes = frames * channels * bits // 8
        assert bool(aiff.pad_data(frames, channels, bits)) == bool(data_bytes % 2)
        assert os.path.getsize(path) == 54 + data_bytes + data_bytes % 2
        assert struct.unpack(">I", open(path, "rb").read()[4:8])[0] == os.path.getsize(path) - 8
        assert (a.channels(), a.bits_per_sample(), a.sample_rate(), a.total_frames()) == (
            channels, bits, 48000, frames)
        assert np.array_equal(read_all(a.to_pcm()), pcm)
        assert a.verify() is True
        ch, b, rate, n, got = aifc_samples(path)
        assert (ch, b, rate, n) == (channels, bits, 48000, frames)
        assert np.array_equal(got, pcm)
        st, info = _atgpu.aiff_read_info(open(path, "rb").read())
        assert st == 0 and (info.ssnd_data_offset, info.ssnd_data_bytes) == (54, data_bytes)


@pytest.mark.parametrize("channels,width", [(1, 1), (2, 2), (2, 3), (5, 2)])
def test_reads_what_aifc_writes(tmp_path, channels, width):
    aifc = pytest.importorskip("aifc")
    bits = 8 * width
    pcm = make_pcm(333, channels, bits, seed=5)
    raw = audiotools.pcm.FrameList._wrap(pcm, channels, bits).to_bytes(True, True)
    path = str(tmp_path / "w.aiff")
    with aifc.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(22050)
        w.writeframes(raw)
    r = aiff.AiffReader(path)
    assert (r.channels, r.bits_per_sample, r.sample_rate, r.total_pcm_frames) == (
        channels, bits, 22050, 333)
    assert np.array_equal(read_all(r, 100), pcm)
    r.close()


def test_header_footer_restores_the_metadata_fixture(tmp_path):
    """aiff_header_footer + from_aiff on aiff-metadata.aiff itself, whose last
    chunk (ID3, 29 bytes) ends the file without its pad byte: accepted at the
    end of the data (the reference's read of chunk_size + 1 bytes fails)"""
    src = audiotools.AiffAudio(fixture("aiff-metadata"))
    header, footer = src.aiff_header_footer()
    out = str(tmp_path / "restored.aiff")
    audiotools.AiffAudio.from_aiff(out, header, src.to_pcm(), footer)
    assert open(out, "rb").read() == open(fixture("aiff-metadata"), "rb").read()
    assert audiotools.AiffAudio(out).verify() is True
    # only at the very end: with a byte after it the odd chunk needs its pad
    with pytest.raises(ValueError, match="I/O error reading footer data"):
        aiff.validate_footer(footer[:-1] + b"NAME", 80)


def test_header_footer_round_trip(tmp_path):
    data = padded_metadata()
    path = str(tmp_path / "metadata.aiff")
    open(path, "wb").write(data)
    src = audiotools.AiffAudio(path)
    assert src.has_foreign_aiff_chunks()
    assert not audiotools.AiffAudio(fixture("aiff-2ch")).has_foreign_aiff_chunks()
    header, footer = src.aiff_header_footer()
    assert header == data[:len(header)] and footer == data[len(data) - len(footer):]
    assert aiff.validate_header(header) == (len(data), 80)
    assert aiff.validate_footer(footer, 80) is True
    out = str(tmp_path / "restored.aiff")
    audiotools.AiffAudio.from_aiff(out, header, src.to_pcm(), footer)
    assert open(out, "rb").read() == data
    # a reader of another length does not fit the header
    short = Reader(read_all(src.to_pcm())[:-2], 2, 16)
    with pytest.raises(audiotools.EncodingError, match="premature end of SSND chunk"):
        audiotools.AiffAudio.from_aiff(out, header, short, footer)
    assert not os.path.isfile(out)


def _form(body):
    return b"FORM" + struct.pack(">I", len(body) + 4) + b"AIFF" + body


def _chunk(cid, data):
    return cid + struct.pack(">I", len(data)) + data + (b"\0" if len(data) % 2 else b"")


def test_validate_header_messages():
    comm = _chunk(b"COMM", bytes(18))
    ssnd = b"SSND" + struct.pack(">I", 8 + 10) + bytes(8)
    assert aiff.validate_header(_form(comm + ssnd))[1] == 10
    cases = [(b"RIFF" + _form(comm + ssnd)[4:], "not an AIFF file"),
             (_form(comm + ssnd)[:8] + b"AIFC" + comm + ssnd, "invalid AIFF file"),
             (_form(_chunk(b"CO\x01M", bytes(18)) + ssnd), "invalid AIFF chunk"),
             (_form(comm + comm + ssnd), "multiple COMM chunks found"),
             (_form(ssnd), "SSND chunk found before fmt"),
             (_form(comm + ssnd + b"x"), "extra data after SSND chunk header"),
             (_form(comm + ssnd[:-1]), "missing data in SSND chunk header"),
             (_form(comm + _chunk(b"NAME", b"abcd")), "SSND chunk not found"),
             (_form(comm + b"NAME" + struct.pack(">I", 100) + b"ab"),
              "I/O error reading header data")]
    for header, message in cases:
        with pytest.raises(ValueError, match=message):
            aiff.validate_header(header)


def test_validate_footer_messages():
    name = _chunk(b"NAME", b"abc")
    assert aiff.validate_footer(b"", 10) is True
    assert aiff.validate_footer(b"\0" + name, 11) is True
    cases = [(_chunk(b"N\xffME", b"ab"), 10, "invalid AIFF chunk"),
             (_chunk(b"COMM", bytes(18)), 10, "multiple COMM chunks found"),
             (name + _chunk(b"SSND", bytes(8)), 10, "multiple SSND chunks found"),
             (b"NAME" + struct.pack(">I", 9) + b"ab", 10, "I/O error reading footer data"),
             (b"", 11, "I/O error reading footer data")]
    for footer, written, message in cases:
        with pytest.raises(ValueError, match=message):
            aiff.validate_footer(footer, written)


def test_seek():
    ch, bits, rate, n, want = aifc_samples(fixture("aiff-2ch"))
    r = aiff.AiffReader(fixture("aiff-2ch"))
    assert r.seek(0) == 0 and np.array_equal(read_all(r), want)
    assert r.seek(7) == 7 and np.array_equal(read_all(r, 3), want[14:])
    assert r.seek(10 ** 6) == n and r.read(10).frames == 0
    assert r.seek(19) == 19 and np.array_equal(r.read(5).samples, want[38:])
    with pytest.raises(ValueError, match="cannot seek to negative value"):
        r.seek(-1)
    r.close()


class _Sized(bytes):
    """no bytes to write, 2^32 of them to count"""

    def __len__(self):
        return 1 << 32


def test_from_pcm_too_large(tmp_path):
    """the 2^32 limit, with a FrameList that only claims its size"""
    class Huge(object):
        frames = 1 << 30

        def __len__(self):
            return 1 << 31

        def to_bytes(self, big_endian, signed):
            return _Sized()

    class HugeReader(Reader):
        def read(self, pcm_frames):
            self.pos += 1
            return Huge() if self.pos == 1 else audiotools.pcm.empty_framelist(2, 16)

    path = str(tmp_path / "huge.aiff")
    with pytest.raises(audiotools.EncodingError, match="PCM data too large for aiff file"):
        audiotools.AiffAudio.from_pcm(path, HugeReader([], 2, 16))
    assert not os.path.isfile(path)
