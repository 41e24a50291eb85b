"""audiotools.cdimage's planning: the cuts of an image and the checks of an
album, every refusal with its message, and the argument errors of
split_image_batch and join_tracks_batch, which come before the GPU library
is so much as loaded.  No GPU."""

import json
import os
from fractions import Fraction

import pytest

import audiotools
from audiotools import Sheet, SheetException, SheetIndex, SheetTrack, cdimage, read_sheet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sheets")
with open(os.path.join(GOLDEN, "expected.json")) as _f:
    EXPECTED = json.load(_f)
NAMES = ["sheet%d.%s" % (n + 1, suffix) for suffix in ("cue", "toc") for n in range(4)]


def _sheet(*starts, **kw):
    """tracks whose index 1 is at the given CD frames"""
    return Sheet([SheetTrack(n + 1, [SheetIndex(1, Fraction(at, 75))])
                  for n, at in enumerate(starts)], **kw)


@pytest.mark.parametrize("name", NAMES)
def test_plan_split_golden(name):
    want = EXPECTED[int(name[5]) - 1]["pcm_lengths"]
    sheet = read_sheet(os.path.join(GOLDEN, name))
    total = sum(want)
    cuts = cdimage.plan_split(sheet, total, 44100)
    assert [n for _, n in cuts] == want
    assert [at for at, _ in cuts] == [sum(want[:k]) for k in range(len(want))]
    # at 44100 Hz a track starts on its index 1, 588 samples a CD frame
    firsts = [[i for i in t.indexes() if i.number() == 1][0] for t in sheet.tracks()]
    assert [at for at, _ in cuts] == [int(i.offset() * 75) * 588 for i in firsts]
    # one frame short of the last track's start is too long a sheet
    assert len(cdimage.plan_split(sheet, total - want[-1] + 1, 44100)) == len(want)
    with pytest.raises(SheetException) as err:
        cdimage.plan_split(sheet, total - want[-1], 44100)
    assert str(err.value) == "cuesheet too long for track being split"
    # an album of those files passes trackcat's check, up to a last length of 0
    params = [(44100, 2, 0x3, 16)] * 3
    assert cdimage.plan_join(params, [total - want[-1], 0, 0], sheet) == total - want[-1]
    with pytest.raises(ValueError) as err:
        cdimage.plan_join(params, [total - want[-1] - 1, 0, 0], sheet)
    assert str(err.value) == "cuesheet too long for track being split"


def test_plan_split_by_hand():
    # 8000 Hz: the differences of 1, 1 and 2 CD frames cut to 106, 106, 213
    sheet = _sheet(0, 1, 2, 4)
    assert cdimage.plan_split(sheet, 1000, 8000) == [(0, 106), (106, 106), (212, 213), (425, 575)]
    exact = Sheet([SheetTrack(n + 1, [SheetIndex(1, Fraction(at, 8000))])
                   for n, at in enumerate((0, 106, 213, 426))])
    assert cdimage.plan_split(exact, 1000, 8000) == [(0, 106), (106, 107), (213, 213), (426, 574)]
    # the offsets add up from frame 0: a first track that starts at 00:00:01
    # shifts every cut by its 588 frames, as the reference's tracksplit does
    assert cdimage.plan_split(_sheet(1, 3), 44100, 44100) == [(0, 1176), (1176, 42924)]
    # one track takes the whole image
    assert cdimage.plan_split(_sheet(0), 5, 44100) == [(0, 5)]
    # index 0 does not move a cut
    pregap = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))]),
                    SheetTrack(2, [SheetIndex(0, Fraction(1, 75)), SheetIndex(1, Fraction(2, 75))])])
    assert cdimage.plan_split(pregap, 2000, 44100) == [(0, 1176), (1176, 824)]


def test_plan_split_refusals():
    for sheet in (None, Sheet([])):
        with pytest.raises(SheetException) as err:
            cdimage.plan_split(sheet, 1000, 44100)
        assert str(err.value) == "you must specify a cuesheet to split audio file"
    with pytest.raises(SheetException) as err:
        cdimage.plan_split(_sheet(0, 0), 1000, 44100)
    assert str(err.value) == "cuesheet not formatted for disc images"
    with pytest.raises(SheetException) as err:
        cdimage.plan_split(_sheet(5, 2), 10 ** 6, 44100)
    assert str(err.value) == "cuesheet not formatted for disc images"
    for total in (588, 587, 0):
        with pytest.raises(SheetException) as err:
            cdimage.plan_split(_sheet(0, 1), total, 44100)
        assert str(err.value) == "cuesheet too long for track being split"
    # tracks ordered by their first index whose index 1 runs backwards
    crossed = Sheet([SheetTrack(1, [SheetIndex(0, Fraction(0)), SheetIndex(1, Fraction(9, 75))]),
                     SheetTrack(2, [SheetIndex(1, Fraction(5, 75))]),
                     SheetTrack(3, [SheetIndex(1, Fraction(20, 75))])])
    assert crossed.image_formatted()
    with pytest.raises(SheetException) as err:
        cdimage.plan_split(crossed, 10 ** 6, 44100)
    assert str(err.value) == "cuesheet not formatted for disc images"
    with pytest.raises(SheetException):
        cdimage.plan_split(Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))]),
                                  SheetTrack(2, [SheetIndex(2, Fraction(1))])]), 10 ** 6, 44100)


def test_a_track_without_an_index_is_a_sheet_error(no_library, tmp_path):
    """the cue reader takes a TRACK with no INDEX line; the planners refuse
    the sheet as a SheetException, which is one image's or album's error"""
    sheet = audiotools.cue.read_cuesheet_string(
        'FILE "a.wav" WAVE\nTRACK 01 AUDIO\nINDEX 01 00:00:00\nTRACK 02 AUDIO\n')
    assert [len(list(t.indexes())) for t in sheet.tracks()] == [1, 0]
    with pytest.raises(SheetException) as err:
        cdimage.plan_split(sheet, 10 ** 6, 44100)
    assert str(err.value) == "a track of the cuesheet has no index"
    with pytest.raises(SheetException) as err:
        cdimage.plan_join([(44100, 2, 0x3, 16)], [10 ** 6], sheet)
    assert str(err.value) == "a track of the cuesheet has no index"


def test_plan_join():
    cd = (44100, 2, 0x3, 16)
    assert cdimage.plan_join([cd, cd, cd], [1, 588, 4097]) == 4686
    for other, message in (((48000, 2, 0x3, 16), "all audio files must have the same sample rate"),
                           ((44100, 1, 0x4, 16), "all audio files must have the same channel count"),
                           ((44100, 2, 0x0, 16),
                            "all audio files must have the same channel assignment"),
                           ((44100, 2, 0x3, 24),
                            "all audio files must have the same bits per sample")):
        with pytest.raises(ValueError) as err:
            cdimage.plan_join([cd, other], [10, 10])
        assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        cdimage.plan_join([], [])
    assert str(err.value) == "you must specify at least 1 supported audio file"
    with pytest.raises(ValueError) as err:
        cdimage.plan_join([cd], [1000], _sheet(0, 0))
    assert str(err.value) == "cuesheet not formatted for disc images"
    # trackcat lets a last track of no frames through, tracksplit does not
    assert cdimage.plan_join([cd, cd], [588, 0], _sheet(0, 1)) == 588
    with pytest.raises(ValueError) as err:
        cdimage.plan_join([cd, cd], [500, 87], _sheet(0, 1))
    assert str(err.value) == "cuesheet too long for track being split"


@pytest.fixture
def no_library(monkeypatch):
    """any use of the GPU library fails the test"""
    from audiotools import _atgpu

    def refuse(*args, **kw):
        raise AssertionError("the GPU library was asked for")
    monkeypatch.setattr(_atgpu, "load_library", refuse)
    monkeypatch.setattr(_atgpu, "engine", refuse)


def test_split_argument_errors(no_library, tmp_path):
    image = str(tmp_path / "a.flac")
    sheet = _sheet(0, 1)
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image, image], [["a", "b"]], [sheet, sheet])
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet, sheet])
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet], target_types="mp3")
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet], target_types=[["flac"]])
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet], target_types=["flac", "wav"])
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet], compression=[["8"]])
    with pytest.raises(ValueError):
        audiotools.split_image_batch([image], [["a", "b"]], [sheet], max_offset=-1)
    assert audiotools.split_image_batch([], []) == []
    # an unreadable sheet is that image's error, and nothing is decoded for it
    out = audiotools.split_image_batch([image, image], [["a"], ["b"]],
                                       [str(tmp_path / "missing.cue"), 5])
    assert isinstance(out[0], SheetException) and isinstance(out[1], ValueError)
    assert not isinstance(out[1], SheetException)


def test_join_argument_errors(no_library, tmp_path):
    a = str(tmp_path / "a.flac")
    with pytest.raises(ValueError):
        audiotools.join_tracks_batch([[a], [a]], ["x.flac"])
    with pytest.raises(ValueError):
        audiotools.join_tracks_batch([[a]], ["x.flac"], sheets=[None, None])
    with pytest.raises(ValueError):
        audiotools.join_tracks_batch([[a]], ["x.flac"], target_types="mp3")
    with pytest.raises(ValueError):
        audiotools.join_tracks_batch([[a]], ["x.flac"], target_types=["flac", "flac"])
    with pytest.raises(ValueError):
        audiotools.join_tracks_batch([[a]], ["x.flac"], compression=["8", "8"])
    assert audiotools.join_tracks_batch([], []) == []
    # an empty album is its own ValueError, with trackcat's words
    out = audiotools.join_tracks_batch([[]], ["x.flac"])
    assert isinstance(out[0], ValueError)
    assert str(out[0]) == "you must specify at least 1 supported audio file"
    # a file that is not there is its album's DecodingError
    out = audiotools.join_tracks_batch([[a]], ["x.flac"])
    assert isinstance(out[0], audiotools.DecodingError)


def test_public_names():
    for name in ("SheetException", "Sheet", "SheetTrack", "SheetIndex", "read_sheet",
                 "parse_timestamp", "build_timestamp", "PCMCat", "LimitedPCMReader", "pcm_split",
                 "split_image_batch", "join_tracks_batch", "cue", "toc"):
        assert hasattr(audiotools, name), name
