"""GPU: convert_files_batch with target_types against the reader path it
replaces, cls.from_pcm(PCMConverter(BufferedPCMReader(source.to_pcm()), ...)),
byte for byte under an all-zero dither, for the nine types the engine writes.

Two things from_pcm takes from its surroundings are pinned for the
comparison: the reference call for an Ogg FLAC file is given the serial
number the batch drew, and the clock ALACAudio stamps an .m4a with stands
still."""
import functools
import os
import types

import pytest

import signals
import audiotools
from audiotools import pcmconverter
from test_gpu_convert_files import (CD, KINDS, SOURCES, classes, converted_frames, read,
                                    sources, zeros)  # noqa: F401  (sources is a fixture)

pytestmark = pytest.mark.gpu

TYPES = ["flac", "oga", "m4a", "tta", "wv", "shn", "wav", "aiff", "au"]


@pytest.fixture(autouse=True)
def still_clock(monkeypatch):
    monkeypatch.setattr(audiotools.m4a, "time", types.SimpleNamespace(time=lambda: 1.7e9))


def from_pcm_kw(suffix, got_path=None):
    """the keywords of the reference call for a type"""
    from audiotools import encoders
    if suffix == "oga":
        serial = int.from_bytes(read(got_path)[14:18], "little") if got_path else 0
        return dict(encoding_function=functools.partial(encoders.encode_oggflac,
                                                        serial_number=serial))
    if suffix == "wv":
        return dict(encoding_function=encoders.encode_wavpack)
    return {}


def reader_path(kind, path, target, suffix, got_path=None, compression=None, sample_rate=None,
                channels=None, channel_mask=None, bits_per_sample=None, frames=None):
    """what the readers write today under an all-zero dither: the file's
    bytes, or the exception from_pcm raises"""
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
    cls = audiotools.targets.SUFFIXES[suffix]
    try:
        cls.from_pcm(target, reader, compression,
                     total_pcm_frames=converted_frames(kind, sample_rate) if frames is None
                     else frames, **from_pcm_kw(suffix, got_path))
    except (audiotools.EncodingError, audiotools.InvalidFile) as err:
        return err
    return read(target)


def same(got, target, want, what):
    """a result of the batch against the reader path's"""
    if isinstance(want, Exception):
        assert type(got) is type(want) and str(got) == str(want).replace(".ref", ""), what
        assert not os.path.exists(target), what
    else:
        assert not isinstance(got, Exception), (what, got)
        assert read(target) == want, what


@pytest.mark.parametrize("suffix", TYPES)
def test_nine_formats_to_cd_quality(sources, tmp_path, suffix):
    cls = audiotools.targets.SUFFIXES[suffix]
    targets = [str(tmp_path / ("%s.%s" % (k, suffix))) for k in KINDS]
    got = audiotools.convert_files_batch([sources[k][0] for k in KINDS], targets, dither=zeros,
                                         target_types=cls, **CD)
    for k, g, t in zip(KINDS, got, targets):
        assert isinstance(g, cls), (k, g)
        assert (g.channels(), g.bits_per_sample(), g.sample_rate()) == (2, 16, 44100)
        assert g.total_frames() == converted_frames(k, 44100)
        want = reader_path(k, sources[k][0], str(tmp_path / ("%s.ref.%s" % (k, suffix))), suffix,
                           t, **CD)
        same(g, t, want, k)


@pytest.mark.parametrize("suffix", TYPES)
def test_plain_transcode(sources, tmp_path, suffix):
    """no target parameters: what the type holds is written, what it cannot
    hold comes back as from_pcm's own exception and the rest are unharmed"""
    targets = [str(tmp_path / ("%s.%s" % (k, suffix))) for k in KINDS]
    got = audiotools.convert_files_batch([sources[k][0] for k in KINDS], targets,
                                         target_types=suffix)
    refused = 0
    for k, g, t in zip(KINDS, got, targets):
        ref = str(tmp_path / ("%s.ref.%s" % (k, suffix)))
        want = reader_path(k, sources[k][0], ref, suffix, t if os.path.exists(t) else None)
        if isinstance(want, Exception):
            refused += 1
            assert type(g) is type(want), (k, g)
            assert str(g) == str(want).replace(ref, t), k
            assert not os.path.exists(t), k
        else:
            same(g, t, want, k)
            n, ch, bits, rate = SOURCES[k]
            assert (g.channels(), g.bits_per_sample(), g.sample_rate(), g.total_frames()) == \
                (ch, bits, rate, n)
    # the three 24-bit sources cannot go into Shorten; everything goes into the others
    assert refused == (3 if suffix == "shn" else 0)


def test_nine_types_in_one_call_by_suffix(sources, tmp_path):
    targets = [str(tmp_path / ("%s.to.%s" % (k, s))) for k, s in zip(KINDS, TYPES)]
    targets[TYPES.index("aiff")] = str(tmp_path / "x.to.aif")
    got = audiotools.convert_files_batch([sources[k][0] for k in KINDS], targets, dither=zeros,
                                         target_types="suffix", **CD)
    for k, s, g, t in zip(KINDS, TYPES, got, targets):
        assert type(g) is audiotools.targets.SUFFIXES[s], (k, g)
        want = reader_path(k, sources[k][0], str(tmp_path / ("%s.ref.%s" % (k, s))), s, t, **CD)
        same(g, t, want, k)


def test_compression_per_target(sources, tmp_path):
    src = sources["flac"][0]
    modes = ["0", "8", "veryfast", "veryhigh", None, "nonsense"]
    suffixes = ["flac", "flac", "wv", "wv", "wv", "flac"]
    targets = [str(tmp_path / ("%d.%s" % (i, s))) for i, s in enumerate(suffixes)]
    got = audiotools.convert_files_batch([src] * 6, targets, dither=zeros, compression=modes,
                                         target_types="suffix", bits_per_sample=16)
    sizes = []
    for i, (m, s, g, t) in enumerate(zip(modes, suffixes, got, targets)):
        want = reader_path("flac", src, str(tmp_path / ("%d.ref.%s" % (i, s))), s, t,
                           compression=m, bits_per_sample=16)
        same(g, t, want, i)
        sizes.append(len(want))
    assert sizes[0] != sizes[1] and sizes[2] != sizes[3]


@pytest.fixture(scope="module")
def short(tmp_path_factory):
    """a 0-frame and a 1-frame 16-bit stereo source"""
    d = tmp_path_factory.mktemp("short_src")
    out = []
    for n in (0, 1):
        path = str(d / ("%d.wav" % n))
        x = signals.make("noise", n, 2, 16, seed=3)
        audiotools.WaveAudio.from_pcm(path, audiotools.FrameListReader(x, 44100, 2, 16, 0x3),
                                      total_pcm_frames=n)
        out.append(path)
    return out


def plain_from_pcm(path, target, suffix, got_path, frames, compression=None):
    cls = audiotools.targets.SUFFIXES[suffix]
    reader = audiotools.BufferedPCMReader(audiotools.WaveAudio(path).to_pcm())
    try:
        cls.from_pcm(target, reader, compression, total_pcm_frames=frames,
                     **from_pcm_kw(suffix, got_path))
    except (audiotools.EncodingError, audiotools.InvalidFile) as err:
        return err
    return read(target)


@pytest.mark.parametrize("suffix", TYPES)
def test_empty_and_one_frame_sources(short, tmp_path, suffix):
    targets = [str(tmp_path / ("%d.%s" % (n, suffix))) for n in (0, 1)]
    got = audiotools.convert_files_batch(short, targets, target_types=suffix)
    for n, g, t in zip((0, 1), got, targets):
        want = plain_from_pcm(short[n], str(tmp_path / ("%d.ref.%s" % (n, suffix))), suffix,
                              t if os.path.exists(t) else None, n)
        if isinstance(want, Exception):
            # from_pcm's own refusal of the case is the batch's result for it
            assert type(g) is type(want) and str(g) == str(want), (n, g)
            assert not os.path.exists(t)
        else:
            same(g, t, want, n)
            assert g.total_frames() == n
    if suffix == "m4a":
        # ALACAudio does not open an .m4a of no frames: from_pcm's last step fails
        assert isinstance(got[0], audiotools.InvalidFile)
    else:
        assert not any(isinstance(g, Exception) for g in got), got


def test_long_track_seek_tables(sources, tmp_path):
    """25 s at 8 kHz: three SEEKTABLE points in FLAC, 24 frames in True
    Audio's seektable"""
    src = sources["long.wav"][0]
    n = SOURCES["long.wav"][0]
    suffixes = ["flac", "oga", "tta", "m4a"]
    targets = [str(tmp_path / ("long." + s)) for s in suffixes]
    got = audiotools.convert_files_batch([src] * 4, targets, target_types="suffix")
    files = {}
    for s, g, t in zip(suffixes, got, targets):
        want = plain_from_pcm(src, str(tmp_path / ("long.ref." + s)), s, t, n)
        same(g, t, want, s)
        files[s] = want
    flac = files["flac"]
    assert flac[4 + 4 + 34] & 0x7F == 3
    assert int.from_bytes(flac[4 + 4 + 34 + 1:4 + 4 + 34 + 4], "big") == 3 * 18
    block = 8000 * 256 // 245
    assert (n + block - 1) // block == 24
    assert len(got[2].__frame_lengths__) == 24


def test_an_unreadable_source_among_good_ones(sources, tmp_path):
    whole = read(sources["flac"][0])
    srcs = [sources["wav"][0], whole[:len(whole) // 2], b"not audio at all", sources["shn"][0],
            sources["aiff"][0]]
    suffixes = ["wv", "m4a", "tta", "au", "oga"]
    targets = [str(tmp_path / ("%d.%s" % (i, s))) for i, s in enumerate(suffixes)]
    targets[4] = str(tmp_path / "no-such-directory" / "x.oga")
    got = audiotools.convert_files_batch(srcs, targets, dither=zeros, target_types="suffix",
                                         **CD)
    assert [type(g) for g in got] == [audiotools.WavPackAudio, audiotools.DecodingError,
                                      audiotools.DecodingError, audiotools.AuAudio,
                                      audiotools.EncodingError]
    assert [os.path.exists(t) for t in targets] == [True, False, False, True, False]
    same(got[0], targets[0], reader_path("wav", sources["wav"][0], str(tmp_path / "r.wv"), "wv",
                                         **CD), "wv")
    same(got[3], targets[3], reader_path("shn", sources["shn"][0], str(tmp_path / "r.au"), "au",
                                         **CD), "au")
