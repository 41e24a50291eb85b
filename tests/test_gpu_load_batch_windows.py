"""GPU: load_batch(start=, length=).  Without a target the rows equal
load_batch() of the whole files sliced, bit for bit, for float32, float16 and
int32; with a target they equal convert_pcm_batch over the sliced source PCM
(24 -> 16 bits under a seeded DeviceDither, 6 -> 2 channels, 96 -> 44.1 kHz
under an all-zero dither).  Per-row starts, frames= padding, an empty window
as a zero row, and error rows as load_batch reports them."""
import numpy as np
import pytest
import torch

import signals
import audiotools
from test_gpu_tensors import (KINDS, MASKS, SOURCES, check_rows, classes,  # noqa: F401
                              sources)  # sources is a fixture

pytestmark = pytest.mark.gpu


def zeros(n):
    return b"\0" * n


def cut(x, ch, start, length):
    n = len(x) // ch
    a = min(start, n)
    b = n if length is None else min(n, start + length)
    return x[a * ch:max(a, b) * ch]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int32],
                         ids=["float32", "float16", "int32"])
def test_windows_equal_the_whole_load_sliced(sources, dtype):
    srcs = [sources[k][0] for k in KINDS]
    whole = audiotools.load_batch(srcs, dtype=dtype)
    for start, length in ((0, None), (1, 2), (50, 1000), (2999, None), (97, 5000)):
        got = audiotools.load_batch(srcs, dtype=dtype, start=start, length=length)
        assert got.errors == [None] * len(KINDS)
        assert got.sample_rates == whole.sample_rates
        assert got.bits_per_sample == whole.bits_per_sample
        assert got.channel_masks == whole.channel_masks
        stop = [int(n) if length is None else min(int(n), start + length) for n in whole.lengths]
        want_len = [max(0, b - start) for b in stop]
        assert got.lengths.tolist() == want_len
        assert got.audio.shape[2] == max(want_len) and got.audio.dtype == dtype
        for k, n in enumerate(want_len):
            assert torch.equal(got.audio[k, :, :n], whole.audio[k, :, start:start + n]), KINDS[k]
            assert not got.audio[k, :, n:].any()


def test_length_alone_starts_at_zero(sources):
    got = audiotools.load_batch([sources["wav"][0]], length=10, dtype=torch.int32)
    assert got.lengths.tolist() == [10]
    want = sources["wav"][1][:20].reshape(10, 2).T
    assert np.array_equal(got.audio[0].cpu().numpy(), want)


def test_bits_under_a_seeded_device_dither(sources):
    kinds = ["flac", "wav", "au"]  # 24 bits each
    start, length = 123, 2000
    params = [(2, 0x3, SOURCES[k][2], SOURCES[k][3]) for k in kinds]
    pcms = [cut(sources[k][1], 2, start, length) for k in kinds]
    want = audiotools.convert_pcm_batch(pcms, params, dither=audiotools.DeviceDither(9),
                                        bits_per_sample=16)
    got = audiotools.load_batch([sources[k][0] for k in kinds], dither=audiotools.DeviceDither(9),
                                bits_per_sample=16, start=start, length=length)
    assert got.errors == [None] * 3 and got.bits_per_sample == [16] * 3
    check_rows(got, want, [(2, 16)] * 3, torch.float32)


@pytest.fixture(scope="module")
def surround(tmp_path_factory):
    n = 3000
    x = signals.make("tone", n, 6, 24, seed=91)
    path = str(tmp_path_factory.mktemp("window_6ch") / "six.flac")
    audiotools.FlacAudio.from_pcm(path, audiotools.FrameListReader(x, 96000, 6, 24, 0x3F),
                                  total_pcm_frames=n)
    return path, x


def test_six_channels_to_two(surround):
    path, x = surround
    start, length = 700, 1500
    want = audiotools.convert_pcm_batch([cut(x, 6, start, length)], [(6, 0x3F, 24, 96000)],
                                        channels=2, channel_mask=0x3)
    got = audiotools.load_batch([path], channels=2, channel_mask=0x3, start=start, length=length)
    assert got.errors == [None] and got.channel_masks == [0x3]
    check_rows(got, want, [(2, 24)], torch.float32)


def test_rate_under_an_all_zero_dither(sources, surround):
    kinds = ["flac", "wav"]  # 96 kHz each
    starts, length = [64, 1000], 1400  # the window is taken in source frames
    params = [(2, 0x3, SOURCES[k][2], SOURCES[k][3]) for k in kinds]
    pcms = [cut(sources[k][1], 2, s, length) for k, s in zip(kinds, starts)]
    want = audiotools.convert_pcm_batch(pcms, params, dither=zeros, sample_rate=44100,
                                        bits_per_sample=16)
    got = audiotools.load_batch([sources[k][0] for k in kinds], dither=zeros, sample_rate=44100,
                                bits_per_sample=16, start=starts, length=length)
    assert got.errors == [None] * 2 and got.sample_rates == [44100] * 2
    check_rows(got, want, [(2, 16)] * 2, torch.float32)


def test_per_row_windows_padding_and_empty_rows(sources, tmp_path):
    srcs = [sources["tta"][0], sources["aiff"][0], sources["m4a"][0], b"not audio",
            str(tmp_path / "is-not-there.wv"), sources["shn"][0]]
    starts = [2990, 100, 4000, 0, 5, 1]
    lengths = [100, 50, None, 10, 10, 1]
    got = audiotools.load_batch(srcs, start=starts, length=lengths, frames=128,
                                dtype=torch.int32)
    assert [type(e) for e in got.errors] == [type(None), type(None), type(None),
                                             audiotools.DecodingError, audiotools.DecodingError,
                                             type(None)]
    # TTA: 10 frames left; AIFF: starts at its end, an empty window and no error
    assert got.lengths.tolist() == [10, 0, 96, 0, 0, 1]
    assert tuple(got.audio.shape) == (6, 2, 128)
    assert got.sample_rates == [44100, 44100, 44100, 0, 0, 44100]
    audio = got.audio.cpu().numpy()
    for k, kind in ((0, "tta"), (2, "m4a"), (5, "shn")):
        x = cut(sources[kind][1], 2, starts[k], lengths[k])
        n = len(x) // 2
        assert np.array_equal(audio[k, :, :n], x.reshape(n, 2).T), kind
        assert not audio[k, :, n:].any()
    assert not audio[[1, 3, 4]].any()
    with pytest.raises(ValueError):
        audiotools.load_batch(srcs[:1], start=0, length=200, frames=99)
    with pytest.raises(ValueError):
        audiotools.load_batch(srcs[:1], start=-1)
    with pytest.raises(ValueError):
        audiotools.load_batch(srcs[:2], start=[1, 2, 3])


def test_no_window_takes_todays_path(sources, monkeypatch):
    from audiotools import windows

    def no_windows(*a, **kw):
        raise AssertionError("windowed")
    monkeypatch.setattr(windows, "decode_windows_batch", no_windows)
    got = audiotools.load_batch([sources["aiff"][0]])
    assert got.lengths.tolist() == [100]
