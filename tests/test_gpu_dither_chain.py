"""GPU: DeviceDither through the batch paths.  A call with
dither=DeviceDither(seed) gives what the same call gives with a callable that
hands every reducing track the first bytes of the port's stream
(tests/dither_port.py) for that track's index in the call: the bits are the
definition's, each track reads its own stream from bit 0, and nothing else
of the call changes."""
import numpy as np
import pytest

import dither_port as port
import signals
import audiotools

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0FFEE123457
MASKS = {1: 0x4, 2: 0x3, 6: 0x3F}


class PortDither(object):
    """the callable: the k-th draw gets the head of stream streams[k]"""

    def __init__(self, seed, streams):
        self.seed, self.streams, self.draws = seed, list(streams), 0

    def __call__(self, n):
        stream = self.streams[self.draws]
        self.draws += 1
        return port.stream_bytes(self.seed, stream, n)


# (channels, bits, rate, frames, dtype) per track; the calls' targets below
TO_CD = [
    (6, 24, 44100, 4097, np.int32),   # 5.1 downmixed to stereo, 24 -> 16
    (2, 16, 44100, 100, np.int16),    # keeps its bits: no draw, its stream unused
    (2, 24, 44100, 1, np.int32),
    (1, 24, 44100, 3, np.int32),      # mono duplicated to stereo
    (2, 16, 44100, 5000, np.int32),   # keeps its bits
    (2, 24, 44100, 4095, np.int32),
    (2, 24, 96000, 6000, np.int32),   # behind a resampler
    (2, 24, 44100, 4096, np.int32),
    (6, 24, 44100, 8193, np.int32),
    (2, 24, 44100, 0, np.int32),      # reduces, but has no sample to reduce
    (1, 24, 44100, 4097, np.int32),
    (2, 8, 44100, 77, np.int16),      # widened
]
TO_8 = [
    (1, 16, 44100, 4096, np.int16),   # mono, 16 -> 8, from int16
    (2, 8, 44100, 50, np.int32),      # keeps its bits
    (2, 24, 48000, 4097, np.int32),   # 24 -> 8
    (2, 16, 44100, 8193, np.int16),
    (1, 8, 8000, 9, np.int16),        # keeps its bits
    (6, 24, 96000, 3, np.int32),      # 5.1 kept as it is, 24 -> 8
    (1, 16, 44100, 1, np.int32),
]
CALLS = [("to-cd", TO_CD, dict(sample_rate=44100, channels=2, channel_mask=0x3,
                               bits_per_sample=16)),
         ("to-8-bit", TO_8, dict(bits_per_sample=8))]


def reducing(tracks, bits):
    """the indices of the tracks that draw, in draw order"""
    return [k for k, t in enumerate(tracks) if t[1] > bits and t[3] > 0]


@pytest.mark.parametrize("name,tracks,target", CALLS, ids=[c[0] for c in CALLS])
def test_convert_pcm_batch(name, tracks, target):
    arrays = [signals.make("noise", n, ch, bits, seed=k + 1).astype(dtype)
              for k, (ch, bits, _, n, dtype) in enumerate(tracks)]
    params = [(ch, MASKS[ch], bits, rate) for ch, bits, rate, _, _ in tracks]
    draws = reducing(tracks, target["bits_per_sample"])
    assert draws != list(range(len(draws)))  # stream index and draw order differ
    f = PortDither(SEED, draws)
    want = audiotools.convert_pcm_batch(arrays, params, dither=f, **target)
    assert f.draws == len(draws)
    got = audiotools.convert_pcm_batch(arrays, params, dither=audiotools.DeviceDither(SEED),
                                       **target)
    assert len(got) == len(want) == len(tracks)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), "track %d" % k
    # the bits matter: another seed gives another result, the same seed the same
    other = audiotools.convert_pcm_batch(arrays, params, dither=audiotools.DeviceDither(SEED + 1),
                                         **target)
    assert any(not np.array_equal(g, o) for g, o in zip(got, other))
    again = audiotools.convert_pcm_batch(arrays, params, dither=audiotools.DeviceDither(SEED),
                                         **target)
    assert all(np.array_equal(g, a) for g, a in zip(got, again))


FILES = [("a.wav", audiotools.WaveAudio, 2, 24, 44100, 4097),
         ("b.flac", audiotools.FlacAudio, 2, 16, 44100, 300),   # keeps its bits
         ("c.aiff", audiotools.AiffAudio, 6, 24, 48000, 5000),
         ("d.au", audiotools.AuAudio, 1, 24, 44100, 3)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dither_src")
    out = []
    for k, (name, cls, ch, bits, rate, n) in enumerate(FILES):
        x = signals.make("noise", n, ch, bits, seed=40 + k)
        path = str(d / name)
        cls.from_pcm(path, audiotools.FrameListReader(x, rate, ch, bits, MASKS[ch]),
                     total_pcm_frames=n)
        out.append(path)
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_convert_files_batch_to_flac(files, tmp_path):
    """three files that lose bits and one between them that does not"""
    draws = [0, 2, 3]
    out = {}
    for name, dither in [("port", PortDither(SEED, draws)),
                         ("device", audiotools.DeviceDither(SEED))]:
        targets = [str(tmp_path / ("%s.%d.flac" % (name, k))) for k in range(len(files))]
        got = audiotools.convert_files_batch(files, targets, bits_per_sample=16, dither=dither)
        assert all(isinstance(g, audiotools.FlacAudio) for g in got), got
        out[name] = [read(t) for t in targets]
    assert out["device"] == out["port"]
    # an unreadable source in front moves no stream: a stream is the index in
    # the call's list, and the callable draws for the readable files alone
    targets = [str(tmp_path / ("shifted.%d.flac" % k)) for k in range(3)]
    got = audiotools.convert_files_batch([b"not audio", files[0], files[2]], targets,
                                         bits_per_sample=16,
                                         dither=audiotools.DeviceDither(SEED))
    assert isinstance(got[0], audiotools.DecodingError)
    want = [str(tmp_path / ("shifted.ref.%d.flac" % k)) for k in range(3)]
    audiotools.convert_files_batch([b"not audio", files[0], files[2]], want, bits_per_sample=16,
                                   dither=PortDither(SEED, [1, 2]))
    assert [read(t) for t in targets[1:]] == [read(t) for t in want[1:]]
    assert read(targets[1]) != out["device"][0]  # stream 1 now, stream 0 before


def test_load_batch(files):
    import torch
    from audiotools import tensors
    srcs = [files[0], files[1], files[3]]   # stereo, stereo, mono -> stereo
    kw = dict(channels=2, channel_mask=0x3, bits_per_sample=8, dtype=torch.int32)
    want = tensors.load_batch(srcs, dither=PortDither(SEED, [0, 1, 2]), **kw)
    got = tensors.load_batch(srcs, dither=audiotools.DeviceDither(SEED), **kw)
    assert got.errors == want.errors == [None] * 3
    assert got.bits_per_sample == [8, 8, 8]
    assert torch.equal(got.lengths, want.lengths)
    assert torch.equal(got.audio, want.audio)
    other = tensors.load_batch(srcs, dither=audiotools.DeviceDither(SEED ^ 1), **kw)
    assert not torch.equal(got.audio, other.audio)
