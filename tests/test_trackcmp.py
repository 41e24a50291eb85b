"""CPU: the host side of audiotools.trackcmp -- the windowed readers against
the port's view rule and the close / ValueError behaviour of the reference's
own test (test/test_core.py:338-412), and frame_cmp_value against the
existing host pcm_frame_cmp."""
import io

import numpy as np
import pytest

import audiotools
import pcm_compare_port as port
from audiotools import pcm

F = audiotools.FRAMELIST_SIZE


def main_reader(n=10, channels=1):
    data = pcm.from_list(list(range(1, n * channels + 1)), channels, 16, True)
    return audiotools.PCMReader(io.BytesIO(data.to_bytes(True, True)), sample_rate=44100,
                                channels=channels, channel_mask=0x4 if channels == 1 else 0x3,
                                bits_per_sample=16, signed=True, big_endian=True)


def drain(reader, step=2):
    out = []
    f = reader.read(step)
    while len(f) > 0:
        out.extend(list(f))
        f = reader.read(step)
    return out


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("offset", [-5, 0, 3, 10, 14])
@pytest.mark.parametrize("frames", [0, 4, 10, 17])
def test_window_against_the_view_rule(offset, frames, channels):
    """offsets before, at, inside and beyond the end of a 10-frame stream;
    windows of no, fewer, as many and more frames than it holds"""
    src = main_reader(10, channels)
    reader = audiotools.PCMReaderWindow(src, offset, frames)
    assert (reader.sample_rate, reader.channels, reader.channel_mask,
            reader.bits_per_sample) == (src.sample_rate, src.channels, src.channel_mask,
                                        src.bits_per_sample)
    want = port.view(np.arange(1, 10 * channels + 1), channels, offset, frames)
    assert drain(reader) == want.reshape(-1).tolist()
    for _ in range(3):
        assert len(reader.read(2)) == 0
    reader.close()
    with pytest.raises(ValueError):
        reader.read(2)
    # closing the window closes the reader under it
    with pytest.raises(ValueError):
        src.read(2)


def test_window_every_small_case():
    """the reference's own sweep: offsets -5..4, lengths 5..14"""
    for offset in range(-5, 5):
        for frames in range(5, 15):
            reader = audiotools.PCMReaderWindow(main_reader(), offset, frames)
            want = port.view(np.arange(1, 11), 1, offset, frames).reshape(-1).tolist()
            assert drain(reader) == want, (offset, frames)


def test_window_refuses_a_negative_length():
    with pytest.raises(ValueError):
        audiotools.PCMReaderWindow(main_reader(), 0, -1)
    with pytest.raises(ValueError):
        audiotools.PCMReaderWindow(main_reader(), 3, -1)
    with pytest.raises(ValueError):
        audiotools.PCMReaderHead(main_reader(), -2)


def test_head_and_dehead_alone():
    assert drain(audiotools.PCMReaderHead(main_reader(), 3)) == [1, 2, 3]
    assert drain(audiotools.PCMReaderHead(main_reader(), 12)) == list(range(1, 11)) + [0, 0]
    assert drain(audiotools.PCMReaderDeHead(main_reader(), 7)) == [8, 9, 10]
    assert drain(audiotools.PCMReaderDeHead(main_reader(), -2)) == [0, 0] + list(range(1, 11))
    assert drain(audiotools.PCMReaderDeHead(main_reader(), 25)) == []
    r = audiotools.PCMReaderDeHead(main_reader(), 2)
    r.close()
    with pytest.raises(ValueError):
        r.read(1)


# ---- frame_cmp_value against pcm_frame_cmp ---------------------------------
LENGTHS = [0, 1, F - 1, F, F + 1, 2 * F]
BASE = (np.arange(2 * F, dtype=np.int64) * 7 % 251 - 125).astype(np.int32)  # mono 8-bit


def reader8(samples):
    return audiotools.FrameListReader(samples, 44100, 1, 8, 0x4)


def host_cmp(a, b):
    return audiotools.pcm_frame_cmp(reader8(a), reader8(b))


@pytest.mark.parametrize("nb", LENGTHS)
@pytest.mark.parametrize("na", LENGTHS)
def test_frame_cmp_value_equals_pcm_frame_cmp(na, nb):
    a, b = BASE[:na].copy(), BASE[:nb].copy()
    common = min(na, nb)
    want = host_cmp(a, b)
    got = audiotools.frame_cmp_value(None, na, nb)
    assert got == want, "no difference planted"
    for at in sorted(set([0, common - 1, F - 1, F])):
        if not 0 <= at < common:
            continue
        b2 = b.copy()
        b2[at] += 1
        first = port.first_mismatch(a[:common, None], b2[:common, None])
        assert first == at
        assert audiotools.frame_cmp_value(first, na, nb) == host_cmp(a, b2), at


def test_frame_cmp_value_chunk_argument():
    assert audiotools.frame_cmp_value(None, 8, 12, chunk=4) == 8
    assert audiotools.frame_cmp_value(None, 12, 7, chunk=4) == 6
    assert audiotools.frame_cmp_value(None, 0, 7, chunk=4) == 0
    assert audiotools.frame_cmp_value(None, 7, 7, chunk=4) is None
    assert audiotools.frame_cmp_value(3, 7, 9, chunk=4) == 3


def test_public_names():
    from audiotools import trackcmp
    for name in trackcmp.__all__:
        assert hasattr(trackcmp, name)
    for name in ("PCMReaderHead", "PCMReaderDeHead", "PCMReaderWindow", "frame_cmp_value",
                 "compare_files_batch", "compare_image_batch", "find_offset_batch",
                 "compare_pcm_batch"):
        assert getattr(audiotools, name) is getattr(trackcmp, name)
