"""CPU: atg_oggflac_read_info (host code of libatgpu: the page reader with the
contract's checks, the first packet, the header packets' channel mask) against
tests/oggflac_port.py on the header cases, and the InvalidFLAC messages of
audiotools.OggFlacAudio (reference audiotools/flac.py:3163-3227).  No GPU."""
import pytest

import oggflac_cases as cases
import oggflac_port as op

HEADER = cases.header_cases()
EXPECT = {
    "header:good": op.OGG_OK, "header:packet_byte": op.OGG_PACKET_BYTE,
    "header:signature": op.OGG_SIGNATURE, "header:major": op.OGG_MAJOR,
    "header:minor": op.OGG_MINOR, "header:flac_signature": op.OGG_FLAC_SIGNATURE,
    "header:block_type": op.OGG_BLOCK_TYPE, "header:short20": op.OGG_STREAMINFO_EOF,
    "header:count_plus2": op.OGG_OK, "header:count_60000": op.OGG_OK,
    "header:page_magic": op.OGG_MAGIC, "header:page_version": op.OGG_VERSION,
    "header:page_crc": op.OGG_CHECKSUM, "header:spanning": op.OGG_OK,
    "header:first_spanning": op.OGG_OK, "header:empty_file": op.OGG_EOF,
    "header:no_packets": op.OGG_FINISHED,
}


def port_info(image):
    packets, _, ostat, _, _ = op.read_packets(image)
    if not packets:
        return (ostat if ostat != op.OGG_OK else op.OGG_FINISHED), 0, None
    return op.parse_first_packet(packets[0])


def test_every_header_case_is_expected():
    assert sorted(EXPECT) == sorted(HEADER)


@pytest.mark.parametrize("name", sorted(HEADER))
def test_read_info_matches_port(name):
    from audiotools import _atgpu
    rc, info = _atgpu.oggflac_read_info(HEADER[name])
    want_rc, count, si = port_info(HEADER[name])
    assert rc == want_rc == EXPECT[name]
    if rc != op.OGG_OK:
        return
    assert info.header_packets == count
    assert info.serial_number == 1
    for k in ("min_block_size", "max_block_size", "min_frame_size", "max_frame_size",
              "sample_rate", "channels", "bits_per_sample", "total_samples"):
        assert getattr(info.si, k) == si[k], k
    assert bytes(info.si.md5) == si["md5"]
    assert info.si.channel_mask == 0x3 and not info.has_channel_mask


def test_header_packet_counts():
    from audiotools import _atgpu
    good = _atgpu.oggflac_read_info(HEADER["header:good"])[1].header_packets
    assert _atgpu.oggflac_read_info(HEADER["header:count_plus2"])[1].header_packets == good + 2
    assert _atgpu.oggflac_read_info(HEADER["header:count_60000"])[1].header_packets == 60000


def test_channel_mask_from_comment_packet():
    from audiotools import _atgpu
    rc, info = _atgpu.oggflac_read_info(cases.with_comment(b"0x0030"))
    assert rc == 0 and info.si.channel_mask == 0x30 and info.has_channel_mask
    # a mask whose speaker count differs from the channels is ignored
    rc, info = _atgpu.oggflac_read_info(cases.with_comment(b"0x0007"))
    assert rc == 0 and info.si.channel_mask == 0x3 and not info.has_channel_mask


def test_scrambled_fields_are_ignored():
    from audiotools import _atgpu
    rc, info = _atgpu.oggflac_read_info(cases.edge_cases()["ignored:scrambled"])
    assert rc == 0 and info.serial_number == (0x1234567 * 3) & 0xFFFFFFFF


MESSAGES = {
    "header:packet_byte": "invalid packet byte", "header:signature": "invalid Ogg signature",
    "header:major": "invalid major version", "header:minor": "invalid minor version",
    "header:flac_signature": "invalid FLAC signature",
    "header:page_magic": "invalid Ogg magic number", "header:page_version": "invalid Ogg version",
    "header:page_crc": "Ogg page checksum mismatch",
    "header:short20": "EOF while reading STREAMINFO block",
    "header:empty_file": "premature EOF reading Ogg stream",
}


@pytest.mark.parametrize("name", sorted(MESSAGES))
def test_oggflacaudio_init_messages(tmp_path, name):
    import audiotools
    fn = str(tmp_path / "a.oga")
    with open(fn, "wb") as f:
        f.write(HEADER[name])
    with pytest.raises(audiotools.InvalidFLAC) as e:
        audiotools.OggFlacAudio(fn)
    assert str(e.value) == MESSAGES[name]


def test_oggflacaudio_fields_and_from_pcm(tmp_path):
    import audiotools
    fn = str(tmp_path / "a.oga")
    with open(fn, "wb") as f:
        f.write(HEADER["header:good"])
    a = audiotools.OggFlacAudio(fn)
    assert (a.channels(), a.bits_per_sample(), a.sample_rate(), a.total_frames()) == \
        (2, 16, 44100, 6 * 192)
    assert a.lossless() and int(a.channel_mask()) == 0x3
    assert audiotools.OggFlacAudio.SUFFIX == "oga"
    with pytest.raises(audiotools.InvalidFLAC):
        audiotools.OggFlacAudio(str(tmp_path / "missing.oga"))
    with pytest.raises(audiotools.EncodingError):
        audiotools.OggFlacAudio.from_pcm(str(tmp_path / "b.oga"), None)
