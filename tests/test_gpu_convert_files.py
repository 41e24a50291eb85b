"""GPU: audiotools.convert_files_batch against the reader path it replaces,
FlacAudio.from_pcm(PCMConverter(BufferedPCMReader(source.to_pcm()), ...)),
byte for byte under an all-zero dither."""
import os

import numpy as np
import pytest

import signals
import audiotools
from audiotools import _atgpu, pcmconverter

pytestmark = pytest.mark.gpu

def classes():
    """kind -> (class, from_pcm keywords); the encoders extension is loaded
    here, after the session has brought the GPU runtime up"""
    from audiotools import encoders
    return {
        "flac": (audiotools.FlacAudio, {}),
        "oga": (audiotools.OggFlacAudio, dict(encoding_function=encoders.encode_oggflac)),
        "m4a": (audiotools.ALACAudio, {}),
        "tta": (audiotools.TrueAudio, {}),
        "wv": (audiotools.WavPackAudio, dict(encoding_function=encoders.encode_wavpack)),
        "shn": (audiotools.ShortenAudio, {}),
        "wav": (audiotools.WaveAudio, {}),
        "aiff": (audiotools.AiffAudio, {}),
        "au": (audiotools.AuAudio, {}),
        "long.wav": (audiotools.WaveAudio, {}),
    }


MASKS = {1: 0x4, 2: 0x3, 6: 0x3F}

# one source per format, 3 frames to 3 FLAC blocks long:
# kind -> (frames, channels, bits, rate)
SOURCES = {
    "flac": (4096 * 2 + 100, 2, 24, 96000),
    "oga": (5000, 2, 16, 48000),
    "m4a": (4096, 2, 16, 44100),
    "tta": (3000, 1, 16, 44100),
    "wv": (4097, 2, 16, 48000),
    "shn": (3, 2, 16, 44100),
    "wav": (5000, 6, 24, 96000),
    "aiff": (100, 2, 16, 44100),
    "au": (4500, 2, 24, 44100),
}
KINDS = list(SOURCES)
# and one of more than two SEEKTABLE intervals (10 s each) at a low rate
SOURCES["long.wav"] = (8000 * 25 + 1, 1, 16, 8000)


def zeros(n):
    return b"\0" * n


def drain(reader):
    parts = []
    while True:
        fl = reader.read(4096)
        if fl.frames == 0:
            break
        parts.append(np.asarray(fl.samples, dtype=np.int32))
    reader.close()
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    d = tmp_path_factory.mktemp("convert_src")
    out = {}
    for k, (kind, (n, ch, bits, rate)) in enumerate(SOURCES.items()):
        x = signals.make("tone", n, ch, bits, seed=20 + k)
        cls, kw = classes()[kind]
        path = str(d / ("source." + kind))
        cls.from_pcm(path, audiotools.FrameListReader(x, rate, ch, bits, MASKS[ch]),
                     total_pcm_frames=n, **kw)
        out[kind] = (path, x)
    return out


def converted_frames(kind, sample_rate):
    n, ch, _, rate = SOURCES[kind]
    if sample_rate is None or sample_rate == rate:
        return n
    return _atgpu.resample_output_frames(n, ch, rate, sample_rate)


def reader_path(kind, path, target, sample_rate=None, channels=None, channel_mask=None,
                bits_per_sample=None, compression="8"):
    """the file the readers write today, under an all-zero dither"""
    _, ch, bits, rate = SOURCES[kind]
    pcm = classes()[kind][0](path).to_pcm()
    t_ch = ch if channels is None else channels
    if channel_mask is None:
        channel_mask = int(pcm.channel_mask) if t_ch == ch else 0
    reader = audiotools.PCMConverter(
        audiotools.BufferedPCMReader(pcm), rate if sample_rate is None else sample_rate, t_ch,
        channel_mask, bits if bits_per_sample is None else bits_per_sample)
    if isinstance(reader, pcmconverter.BPSConverter):
        reader._rand = zeros
    audiotools.FlacAudio.from_pcm(target, reader, compression,
                                  total_pcm_frames=converted_frames(kind, sample_rate))
    with open(target, "rb") as f:
        return f.read()


def read(path):
    with open(path, "rb") as f:
        return f.read()


CD = dict(sample_rate=44100, channels=2, channel_mask=0x3, bits_per_sample=16)


def test_nine_formats_to_cd_quality_byte_identical(sources, tmp_path):
    targets = [str(tmp_path / (k + ".flac")) for k in KINDS]
    got = audiotools.convert_files_batch([sources[k][0] for k in KINDS], targets, dither=zeros,
                                         compression="8", **CD)
    for k, g, t in zip(KINDS, got, targets):
        assert isinstance(g, audiotools.FlacAudio), (k, g)
        assert (g.channels(), g.bits_per_sample(), g.sample_rate()) == (2, 16, 44100)
        assert g.total_frames() == converted_frames(k, 44100)
        want = reader_path(k, sources[k][0], str(tmp_path / (k + ".ref.flac")), **CD)
        assert read(t) == want, k  # STREAMINFO MD5, SEEKTABLE and PADDING included


def test_no_target_is_a_plain_transcode(sources, tmp_path):
    targets = [str(tmp_path / (k + ".flac")) for k in KINDS]
    got = audiotools.convert_files_batch([sources[k][0] for k in KINDS], targets)
    for k, g, t in zip(KINDS, got, targets):
        n, ch, bits, rate = SOURCES[k]
        assert isinstance(g, audiotools.FlacAudio), (k, g)
        assert (g.channels(), g.bits_per_sample(), g.sample_rate(), g.total_frames()) == \
            (ch, bits, rate, n)
        assert np.array_equal(drain(g.to_pcm()), sources[k][1]), k
        assert read(t) == reader_path(k, sources[k][0], str(tmp_path / (k + ".ref.flac"))), k
    # the 6-channel 24-bit source kept as it is carries its channel mask
    assert b"WAVEFORMATEXTENSIBLE_CHANNEL_MASK=0x003F" in read(targets[KINDS.index("wav")])
    assert int(got[KINDS.index("wav")].channel_mask()) == 0x3F


MIXED = ["flac", "oga", "tta", "wav", "au"]  # they differ in rate, bits and channels


@pytest.mark.parametrize("target", [dict(sample_rate=48000, bits_per_sample=16),
                                    dict(channels=1, channel_mask=0x4),
                                    dict(channels=2, channel_mask=0x3, compression="0")],
                         ids=["rate-bits", "mono", "stereo-flac0"])
def test_mixed_batch_writes_what_the_one_file_call_writes(sources, tmp_path, target):
    targets = [str(tmp_path / (k + ".flac")) for k in MIXED]
    got = audiotools.convert_files_batch([sources[k][0] for k in MIXED], targets, dither=zeros,
                                         **target)
    for k, g, t in zip(MIXED, got, targets):
        assert isinstance(g, audiotools.FlacAudio), (k, g)
        one = str(tmp_path / (k + ".one.flac"))
        alone = audiotools.convert_files_batch([sources[k][0]], [one], dither=zeros, **target)
        assert isinstance(alone[0], audiotools.FlacAudio)
        assert read(t) == read(one), k


def test_mixed_batch_against_the_readers(sources, tmp_path):
    target = dict(sample_rate=48000, bits_per_sample=16)
    kinds = ["flac", "wav", "tta", "au", "shn"]
    targets = [str(tmp_path / (k + ".flac")) for k in kinds]
    got = audiotools.convert_files_batch([sources[k][0] for k in kinds], targets, dither=zeros,
                                         **target)
    for k, g, t in zip(kinds, got, targets):
        assert isinstance(g, audiotools.FlacAudio), (k, g)
        assert read(t) == reader_path(k, sources[k][0], str(tmp_path / (k + ".ref.flac")),
                                      **target), k


def test_long_track_gets_the_readers_seektable(sources, tmp_path):
    """three seek points: the encoder's frame offsets are walked for them"""
    src = sources["long.wav"][0]
    for name, target in [("same", {}), ("bits", dict(bits_per_sample=8)),
                         ("stereo", dict(channels=2, channel_mask=0x3))]:
        out = str(tmp_path / (name + ".flac"))
        got = audiotools.convert_files_batch([src, sources["aiff"][0]],
                                             [out, str(tmp_path / "short.flac")], dither=zeros,
                                             **target)
        assert isinstance(got[0], audiotools.FlacAudio), got[0]
        want = reader_path("long.wav", src, str(tmp_path / (name + ".ref.flac")), **target)
        assert read(out) == want, name
        # the SEEKTABLE block (type 3) follows STREAMINFO: 3 points of 18 bytes
        assert want[4 + 4 + 34] & 0x7F == 3
        assert int.from_bytes(want[4 + 4 + 34 + 1:4 + 4 + 34 + 4], "big") == 3 * 18


def test_failed_files_return_their_errors_and_stop_nothing(sources, tmp_path):
    whole = read(sources["flac"][0])
    cut = whole[:len(whole) // 2]
    names = ["good1", "cut", "missing", "junk", "nowhere", "good2"]
    srcs = [sources["wav"][0], cut, str(tmp_path / "is-not-there.flac"), b"not audio at all",
            sources["oga"][0], sources["shn"][0]]
    targets = [str(tmp_path / (n + ".flac")) for n in names]
    targets[4] = str(tmp_path / "no-such-directory" / "nowhere.flac")
    got = audiotools.convert_files_batch(srcs, targets, dither=zeros, **CD)
    assert [type(g) for g in got] == [audiotools.FlacAudio, audiotools.DecodingError,
                                      audiotools.DecodingError, audiotools.DecodingError,
                                      audiotools.EncodingError, audiotools.FlacAudio]
    assert [os.path.exists(t) for t in targets] == [True, False, False, False, False, True]
    assert read(targets[0]) == reader_path("wav", sources["wav"][0],
                                           str(tmp_path / "wav.ref.flac"), **CD)
    assert read(targets[5]) == reader_path("shn", sources["shn"][0],
                                           str(tmp_path / "shn.ref.flac"), **CD)


def test_ogg_flac_and_native_flac_share_one_call(sources, tmp_path):
    """both go through one decoder handle; each keeps its own PCM"""
    kinds = ["flac", "oga", "flac", "oga"]
    srcs = [sources["flac"][0], sources["oga"][0], read(sources["flac"][0]),
            read(sources["oga"][0])]
    targets = [str(tmp_path / ("%d.flac" % k)) for k in range(4)]
    got = audiotools.convert_files_batch(srcs, targets)
    for k, g in zip(kinds, got):
        assert isinstance(g, audiotools.FlacAudio), (k, g)
        assert np.array_equal(drain(g.to_pcm()), sources[k][1]), k


def test_seeded_dither_reproduces_a_call(sources, tmp_path):
    class Stream(object):
        def __init__(self):
            self.rng = np.random.RandomState(5)

        def __call__(self, n):
            return self.rng.bytes(n)

    kinds = ["flac", "au", "wav"]
    out = []
    for run in range(2):
        targets = [str(tmp_path / ("%s.%d.flac" % (k, run))) for k in kinds]
        got = audiotools.convert_files_batch([sources[k][0] for k in kinds], targets,
                                             bits_per_sample=16, dither=Stream())
        assert all(isinstance(g, audiotools.FlacAudio) for g in got)
        out.append([read(t) for t in targets])
    assert out[0] == out[1]
    zero = str(tmp_path / "zero.flac")
    audiotools.convert_files_batch([sources["au"][0]], [zero], bits_per_sample=16, dither=zeros)
    assert read(zero) != out[0][1]
    # without a resampler the seeded bits are the readers' bits
    n, ch, _, _ = SOURCES["flac"]
    source = audiotools.FlacAudio(sources["flac"][0])
    reader = audiotools.PCMConverter(audiotools.BufferedPCMReader(source.to_pcm()), 96000, 2, 0x3,
                                     16)
    reader._rand = Stream()
    ref = str(tmp_path / "seeded.ref.flac")
    audiotools.FlacAudio.from_pcm(ref, reader, "8", total_pcm_frames=n)
    assert read(ref) == out[0][0]
