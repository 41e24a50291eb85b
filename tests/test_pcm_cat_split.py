"""audiotools.PCMCat, LimitedPCMReader and pcm_split: what the reference's
own tests of the three ask of them (its test/test_core.py, classes PCMCat,
LimitedPCMReader and Test_pcm_split), for Python 3."""

import io

import pytest

import audiotools
from audiotools.pcm import from_list


def _reader(samples=(), sample_rate=44100, channels=1, channel_mask=0x4, bits_per_sample=16):
    data = from_list(list(samples), channels, bits_per_sample, True).to_bytes(True, True)
    return audiotools.PCMReader(io.BytesIO(data), sample_rate=sample_rate, channels=channels,
                                channel_mask=channel_mask, bits_per_sample=bits_per_sample,
                                signed=True, big_endian=True)


def _drain(reader, at_a_time=2):
    out = []
    f = reader.read(at_a_time)
    while len(f) > 0:
        out.extend(list(f))
        f = reader.read(at_a_time)
    return out


def test_pcmcat_mismatches():
    audiotools.PCMCat([_reader()])
    for other, message in ((dict(sample_rate=96000),
                            "all audio files must have the same sample rate"),
                           (dict(channels=2, channel_mask=0x3),
                            "all audio files must have the same channel count"),
                           (dict(bits_per_sample=24),
                            "all audio files must have the same bits per sample")):
        with pytest.raises(ValueError) as err:
            audiotools.PCMCat([_reader(**other), _reader()])
        assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        audiotools.PCMCat([])
    assert str(err.value) == "you must have at least 1 PCMReader"
    # the channel mask is not compared: the first reader's is reported
    assert audiotools.PCMCat([_reader(channel_mask=0x4), _reader(channel_mask=0x1)]
                             ).channel_mask == 0x4


def test_pcmcat_reads_every_reader_to_its_end():
    main_readers = [_reader(r) for r in (range(-15, -5), range(-5, 5), range(5, 15))]
    reader = audiotools.PCMCat(main_readers)
    assert (reader.sample_rate, reader.channels, reader.channel_mask,
            reader.bits_per_sample) == (44100, 1, 0x4, 16)
    assert _drain(reader) == list(range(-15, 15))
    for _ in range(10):
        assert len(reader.read(2)) == 0
    # the readers behind it are drained, not closed
    for r in main_readers:
        for _ in range(10):
            assert len(r.read(2)) == 0
    reader.close()
    with pytest.raises(ValueError):
        reader.read(2)
    for r in main_readers:
        with pytest.raises(ValueError):
            r.read(2)


def test_pcmcat_skips_empty_readers():
    reader = audiotools.PCMCat([_reader(), _reader([1, 2, 3]), _reader(), _reader(), _reader([4])])
    assert _drain(reader, 4096) == [1, 2, 3, 4]
    assert len(reader.read(1)) == 0


def test_limited_pcm_reader():
    main_reader = _reader(range(-50, 50))
    total = []
    for pcm_frames in (10, 20, 30, 40):
        reader = audiotools.LimitedPCMReader(main_reader, pcm_frames)
        assert (reader.sample_rate, reader.channels, reader.channel_mask,
                reader.bits_per_sample) == (44100, 1, 0x4, 16)
        samples = _drain(reader)
        assert len(samples) == pcm_frames
        total.extend(samples)
        for _ in range(10):
            assert len(reader.read(2)) == 0
        # closing the part closes the part alone
        reader.close()
        with pytest.raises(ValueError):
            reader.read(2)
    assert total == list(range(-50, 50))
    for _ in range(10):
        assert len(main_reader.read(2)) == 0
    main_reader.close()
    with pytest.raises(ValueError):
        main_reader.read(2)


def test_limited_pcm_reader_cuts_a_large_read():
    buffered = audiotools.BufferedPCMReader(_reader(range(100)))
    head = audiotools.LimitedPCMReader(buffered, 7)
    assert list(head.read(4096)) == list(range(7))
    assert len(head.read(4096)) == 0
    assert list(buffered.read(3)) == [7, 8, 9]


def test_pcm_split():
    """the reference's lengths are 5, 10, 15, 4, 16 and 10 seconds of a
    minute of CD audio; here the same proportions of a short stereo stream,
    with one piece above the size from which a temporary file holds it"""
    big = audiotools.FRAMELIST_SIZE * 10 + 3
    lengths = [5, 10, 15, 0, big, 4, 16, 10]
    total = sum(lengths)
    samples = [((n * 7919) % 65536) - 32768 for n in range(2 * total)]
    source = _reader(samples, channels=2, channel_mask=0x3)
    pieces = audiotools.pcm_split(source, lengths)
    at = 0
    for piece, frames in zip(pieces, lengths):
        assert (piece.sample_rate, piece.channels, piece.channel_mask,
                piece.bits_per_sample) == (44100, 2, 0x3, 16)
        got = _drain(piece, 1 << 20)
        assert len(got) == 2 * frames
        assert got == samples[2 * at:2 * (at + frames)]
        at += frames
    # the generator closes the source once its last piece is out
    assert list(pieces) == []
    with pytest.raises(ValueError):
        source.read(1)
