"""CPU: the parts of convert_files_batch's target types that need no GPU --
how target_types and compression are read, and that every stream a target
type cannot hold is refused with the exception, class and message, that the
type's own from_pcm raises, before any GPU work and with no file left."""
import os

import pytest

import signals
import audiotools
from audiotools import targets as tg

NINE = [audiotools.FlacAudio, audiotools.OggFlacAudio, audiotools.ALACAudio,
        audiotools.TrueAudio, audiotools.WavPackAudio, audiotools.ShortenAudio,
        audiotools.WaveAudio, audiotools.AiffAudio, audiotools.AuAudio]
SUFFIXES = ["flac", "oga", "m4a", "tta", "wv", "shn", "wav", "aiff", "au"]


# ------------------------------------------------------------- target_types
def test_the_nine_classes_and_their_suffixes():
    assert list(tg.CLASSES) == NINE
    assert [c.SUFFIX for c in NINE] == SUFFIXES


def test_one_value_for_all_targets():
    names = ["a.x", "b.y", "c"]
    for cls, suffix in zip(NINE, SUFFIXES):
        assert tg.resolve_types(cls, names) == [cls] * 3
        assert tg.resolve_types(suffix, names) == [cls] * 3


def test_one_value_per_target():
    mixed = [audiotools.WaveAudio, "tta", "suffix"]
    assert tg.resolve_types(mixed, ["a", "b", "c.m4a"]) == [
        audiotools.WaveAudio, audiotools.TrueAudio, audiotools.ALACAudio]
    assert tg.resolve_types(tuple(NINE), SUFFIXES) == NINE


def test_suffix_takes_the_type_from_the_file_name():
    names = ["/x/y.z/t.%s" % s for s in SUFFIXES]
    assert tg.resolve_types("suffix", names) == NINE
    assert tg.resolve_types("suffix", ["a.aif", "B.AIFF", "c.FLAC"]) == [
        audiotools.AiffAudio, audiotools.AiffAudio, audiotools.FlacAudio]
    assert tg.resolve_types("aif", ["x"]) == [audiotools.AiffAudio]


@pytest.mark.parametrize("types,names", [
    ("suffix", ["a.flac", "b.mp3"]),
    ("suffix", ["no-suffix"]),
    ("suffix", ["dir.flac/name"]),
    ("mp3", ["a.flac"]),
    (audiotools.AudioFile, ["a.flac"]),
    (int, ["a.flac"]),
    (["flac"], ["a.flac", "b.flac"]),
    (["flac", "wav", "au"], ["a", "b"]),
    ([], ["a"]),
])
def test_what_is_no_target_type(types, names):
    with pytest.raises(ValueError):
        tg.resolve_types(types, names)
    # and from the public call, before any file is opened or any GPU work
    with pytest.raises(ValueError):
        audiotools.convert_files_batch([b"not audio"] * len(names), names, target_types=types)
    assert not any(os.path.exists(n) for n in names)


def test_none_is_flac_and_lengths_are_checked():
    # an unreadable source with the default type: today's result
    got = audiotools.convert_files_batch([b"junk"], ["x.wav"])
    assert isinstance(got[0], audiotools.DecodingError)
    with pytest.raises(ValueError):
        audiotools.convert_files_batch([b"junk"], ["a", "b"], target_types="wav")


# -------------------------------------------------------------- compression
def test_compression_falls_back_to_the_class_default():
    f, w, a = audiotools.FlacAudio, audiotools.WavPackAudio, audiotools.ALACAudio
    assert tg.resolve_compression(None, [f, w, a, audiotools.OggFlacAudio]) == [
        "8", "standard", None, "8"]
    assert tg.resolve_compression("0", [f, w, a]) == ["0", "standard", None]
    assert tg.resolve_compression("veryhigh", [f, w]) == ["8", "veryhigh"]
    assert tg.resolve_compression(["0", "veryfast", "5"], [f, w, w]) == ["0", "veryfast",
                                                                         "standard"]
    assert tg.resolve_compression([None, "nonsense"], [f, w]) == ["8", "standard"]
    assert tg.resolve_compression(8, [f]) == ["8"]  # not the string "8": unknown
    with pytest.raises(ValueError):
        tg.resolve_compression(["0"], [f, w])
    for cls in NINE:  # what each from_pcm itself falls back to
        modes = getattr(cls, "COMPRESSION_MODES", ())
        assert tg.resolve_compression("?", [cls]) == [getattr(cls, "DEFAULT_COMPRESSION", None)]
        for m in modes:
            assert tg.resolve_compression(m, [cls]) == [m]


# ----------------------------------------------------------------- refusals
class Stream(object):
    """a reader from_pcm refuses before it reads"""

    def __init__(self, channels, channel_mask, bits_per_sample, sample_rate=44100):
        self.channels, self.channel_mask = channels, channel_mask
        self.bits_per_sample, self.sample_rate = bits_per_sample, sample_rate

    def read(self, n):
        raise AssertionError("a refused stream is never read")

    def close(self):
        pass


def never(*args, **kw):
    raise AssertionError("a refused stream is never encoded")


KW = {audiotools.OggFlacAudio: dict(encoding_function=never),
      audiotools.WavPackAudio: dict(encoding_function=never)}

# (class, channels, mask, bits): what the issue names and every other
# refusal a from_pcm makes from the stream's parameters
REFUSED = [
    (audiotools.ALACAudio, 2, 0x3, 8),
    (audiotools.ALACAudio, 2, 0x30, 16),        # side pair alone
    (audiotools.ALACAudio, 4, 0x33, 24),        # quad: no ALAC layout
    (audiotools.ShortenAudio, 2, 0x3, 24),
    (audiotools.ShortenAudio, 6, 0x3F, 24),
    (audiotools.FlacAudio, 9, 0x1FF, 16),
    (audiotools.FlacAudio, 2, 0x30, 16),
    (audiotools.FlacAudio, 4, 0x0F, 24),
    (audiotools.OggFlacAudio, 9, 0, 16),
    (audiotools.OggFlacAudio, 2, 0x30, 16),
]


@pytest.mark.parametrize("cls,ch,mask,bits", REFUSED,
                         ids=["%s-%dch-%#x-%d" % (c.SUFFIX, ch, m, b) for c, ch, m, b in REFUSED])
def test_prepare_raises_what_from_pcm_raises(cls, ch, mask, bits, tmp_path):
    name = str(tmp_path / ("refused." + cls.SUFFIX))
    with pytest.raises(audiotools.EncodingError) as want:
        cls.from_pcm(name, Stream(ch, mask, bits), total_pcm_frames=10, **KW.get(cls, {}))
    with pytest.raises(audiotools.EncodingError) as got:
        tg.prepare(cls, name, ch, mask, bits, 44100, 10)
    assert type(got.value) is type(want.value)
    assert str(got.value) == str(want.value) and str(got.value)
    assert not os.path.exists(name)


def test_what_every_type_holds_is_prepared():
    for cls in NINE:
        bits = 16
        tg.prepare(cls, "x." + cls.SUFFIX, 2, 0x3, bits, 44100, 10)
        tg.prepare(cls, "x." + cls.SUFFIX, 1, 0x4, bits, 8000, 0)
    for cls in NINE:
        if cls is not audiotools.ShortenAudio:
            tg.prepare(cls, "x", 6, 0x3F, 24, 96000, 1)
    for cls in NINE:
        if cls is not audiotools.ALACAudio:
            tg.prepare(cls, "x", 2, 0x3, 8, 44100, 1)
    # what the writers take from it
    assert tg.prepare(audiotools.FlacAudio, "x", 6, 0, 16, 44100, 1) == 0x3F
    assert tg.prepare(audiotools.OggFlacAudio, "x", 2, 0x3, 16, 44100, 1) == 0
    assert tg.prepare(audiotools.OggFlacAudio, "x", 2, 0x3, 24, 44100, 1) == 0x3
    header, footer = tg.prepare(audiotools.ShortenAudio, "x", 1, 0x4, 8, 8000, 3)
    assert header[:4] == b"RIFF" and header[-4:] == (3).to_bytes(4, "little") and footer == b"\0"
    assert tg.prepare(audiotools.WaveAudio, "x", 1, 0x4, 8, 8000, 3) == header


@pytest.fixture(scope="module")
def wav24(tmp_path_factory):
    """a 24-bit stereo wave file and an 8-bit one, written without a GPU"""
    d = tmp_path_factory.mktemp("targets_src")
    out = []
    for bits in (24, 8):
        path = str(d / ("s%d.wav" % bits))
        x = signals.make("tone", 50, 2, bits, seed=bits)
        audiotools.WaveAudio.from_pcm(path, audiotools.FrameListReader(x, 44100, 2, bits, 0x3),
                                      total_pcm_frames=50)
        out.append(path)
    return out


def test_refused_sources_keep_from_pcms_error_and_leave_no_file(wav24, tmp_path):
    """every source of the call is refused or unreadable, so the call needs no GPU"""
    s24, s8 = wav24
    names = [str(tmp_path / n) for n in ("a.shn", "b.m4a", "c.flac", "d.oga")]
    got = audiotools.convert_files_batch([s24, s8, b"junk", s24], names,
                                         target_types=["suffix", "m4a", audiotools.FlacAudio,
                                                       "suffix"],
                                         channels=4, channel_mask=0x0F)
    # 24 bits into Shorten, 8 into ALAC, a mask Ogg FLAC cannot write: from_pcm's own words
    for g, cls, bits, name in [(got[0], audiotools.ShortenAudio, 24, names[0]),
                               (got[1], audiotools.ALACAudio, 8, names[1]),
                               (got[3], audiotools.OggFlacAudio, 24, names[3])]:
        with pytest.raises(audiotools.EncodingError) as want:
            cls.from_pcm(name, Stream(4, 0x0F, bits), total_pcm_frames=50, **KW.get(cls, {}))
        assert type(g) is type(want.value) and str(g) == str(want.value), name
    assert [type(g).__name__ for g in got] == ["UnsupportedBitsPerSample",
                                               "UnsupportedBitsPerSample", "DecodingError",
                                               "UnsupportedChannelMask"]
    assert not any(os.path.exists(n) for n in names)
