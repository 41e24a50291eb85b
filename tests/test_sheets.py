"""audiotools.sheets / cue / toc: the reference's four cue and four toc test
sheets (tests/golden/sheets, the texts its test suite carries) parse to the
values its tests expect (expected.json), convert into each other, and every
refusal of the cue reader carries its message and line number."""

import io
import json
import os
from fractions import Fraction

import pytest

import audiotools
from audiotools import (Sheet, SheetException, SheetIndex, SheetTrack, build_timestamp, cue,
                        parse_timestamp, read_sheet, toc)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sheets")
with open(os.path.join(GOLDEN, "expected.json")) as _f:
    EXPECTED = json.load(_f)
NAMES = ["sheet%d.%s" % (n + 1, suffix) for suffix in ("cue", "toc") for n in range(4)]


def _expected(name):
    return EXPECTED[int(name[5]) - 1]


@pytest.mark.parametrize("name", NAMES)
def test_read_sheet(name):
    want = _expected(name)
    sheet = read_sheet(os.path.join(GOLDEN, name))
    assert sheet.catalog() == want["catalog"]
    assert [t.ISRC() for t in sheet.tracks()] == want["ISRCs"]
    assert [[int(i.offset() * 75) for i in t.indexes()] for t in sheet.tracks()] == want["indexes"]
    assert [t.number() for t in sheet.tracks()] == list(range(1, len(want["ISRCs"]) + 1))
    assert all(t.audio() for t in sheet.tracks())
    assert all(isinstance(i.offset(), Fraction) for t in sheet.tracks() for i in t.indexes())
    assert list(sheet.pcm_lengths(sum(want["pcm_lengths"]), 44100)) == want["pcm_lengths"]
    assert sheet.image_formatted()
    assert sheet.track(2).number() == 2
    with pytest.raises(KeyError):
        sheet.track(99)
    with pytest.raises(KeyError):
        sheet.track(1).index(77)


@pytest.mark.parametrize("n", range(4))
def test_cue_and_toc_of_one_disc_agree(n):
    a = read_sheet(os.path.join(GOLDEN, "sheet%d.cue" % (n + 1)))
    b = read_sheet(os.path.join(GOLDEN, "sheet%d.toc" % (n + 1)))
    assert ([[i.offset() for i in t.indexes()] for t in a.tracks()] ==
            [[i.offset() for i in t.indexes()] for t in b.tracks()])


@pytest.mark.parametrize("name", NAMES)
def test_convert_sheet(name, tmp_path):
    """cue -> toc -> cue and toc -> cue -> toc compare equal"""
    sheet = read_sheet(os.path.join(GOLDEN, name))
    cue_file = str(tmp_path / "a.cue")
    with open(cue_file, "w", newline="") as f:
        cue.write_cuesheet(sheet, "a.wav", f)
    from_cue = read_sheet(cue_file)
    assert from_cue == sheet and not (from_cue != sheet)
    toc_file = str(tmp_path / "a.toc")
    with open(toc_file, "w") as f:
        toc.write_tocfile(from_cue, "a.wav", f)
    from_toc = read_sheet(toc_file)
    for t1, t2 in zip(sheet.tracks(), from_toc.tracks()):
        assert t1 == t2
    assert from_toc == sheet
    back = io.StringIO()
    cue.write_cuesheet(from_toc, "a.wav", back)
    assert cue.read_cuesheet_string(back.getvalue()) == sheet
    assert isinstance(toc.read_tocfile(toc_file), Sheet)
    assert isinstance(cue.read_cuesheet(cue_file), Sheet)


def test_written_forms():
    sheet = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0, 75))], True, "JPG750800183"),
                   SheetTrack(2, [SheetIndex(0, Fraction(150, 75)), SheetIndex(1, Fraction(225, 75)),
                                  SheetIndex(2, Fraction(4500, 75))])], "4580226563955")
    out = io.StringIO()
    cue.write_cuesheet(sheet, "cd.wav", out)
    assert out.getvalue() == ('CATALOG 4580226563955\r\nFILE "cd.wav" WAVE\r\n'
                              "  TRACK 01 AUDIO\r\n    ISRC JPG750800183\r\n"
                              "    INDEX 01 00:00:00\r\n  TRACK 02 AUDIO\r\n"
                              "    INDEX 00 00:02:00\r\n    INDEX 01 00:03:00\r\n"
                              "    INDEX 02 01:00:00\r\n")
    out = io.StringIO()
    toc.write_tocfile(sheet, "cd.wav", out)
    assert out.getvalue() == ('CD_DA\n\nCATALOG "4580226563955"\n\nTRACK AUDIO\n'
                              '  ISRC "JPG750800183"\n  AUDIOFILE "cd.wav" 00:00:00 00:02:00\n'
                              'TRACK AUDIO\n  AUDIOFILE "cd.wav" 00:02:00\n  START 00:01:00\n'
                              "  INDEX 01:00:00\n")


# --------------------------------------------------------------- cue refusals
T = "TRACK 01 AUDIO\n"
CUE_ERRORS = [
    ("TRACK AUDIO\n", "invalid track number at line 1"),
    ("TRACK 01 01\n", "invalid track type at line 1"),
    ("TRACK 01 AUDIO EXTRA\n", "excess data at line 1"),
    # the line end that stands where the value should carries the next line's number
    ("CATALOG\n", "missing value at line 2"),
    ('REM x\nTITLE\n', "missing value at line 3"),
    ("CATALOG 123 456\n", "excess data at line 1"),
    ("FILE WAVE\n", "missing filename at line 1"),
    ('FILE "a.wav" 12\n', "missing file type at line 1"),
    ('FILE "a.wav" WAVE 12\n', "excess data at line 1"),
    ("BOGUS x\n", "invalid tag BOGUS at line 1"),
    (T + "BOGUS\n", "invalid tag BOGUS at line 2"),
    (T + 'TITLE "a" "b"\n', "invalid data at line 2"),
    (T + "ISRC JPG750800183 1\n", "invalid data at line 2"),
    (T + 'ISRC "abc"\n', "missing value at line 2"),
    (T + "FLAGS 12\n", "invalid flag at line 2"),
    (T + "INDEX 01 12\n", "invalid timestamp at line 2"),
    (T + "PREGAP 12\n", "invalid timestamp at line 2"),
    (T + "POSTGAP 00:02:00 7\n", "excess data at line 2"),
    (T + "INDEX AA 00:00:00\n", "invalid index number at line 2"),
    (T + "INDEX 01 00:00:00 9\n", "excess data at line 2"),
    ('"quoted"\n', "missing tag at line 1"),
    (T + "\n12\n", "missing tag at line 2"),
    # a tab fits no token; the character is counted from the start of the text
    ('FILE "a.wav" WAVE\r\n\tTRACK 01 AUDIO\r\n', "invalid token at char 19"),
    (b"\xef\xbb\xbfREM x\n\tTRACK", "invalid token at char 9"),
]


@pytest.mark.parametrize("text,message", CUE_ERRORS)
def test_cue_errors(text, message):
    with pytest.raises(cue.CueException) as err:
        cue.read_cuesheet_string(text)
    assert str(err.value) == message
    assert isinstance(err.value, SheetException) and isinstance(err.value, ValueError)


def test_cue_unreadable(tmp_path):
    with pytest.raises(cue.CueException) as err:
        cue.read_cuesheet(str(tmp_path / "missing.cue"))
    assert str(err.value) == "unable to read cuesheet"
    assert cue.ERR_CUE_INVALID_FORMAT == "cuesheet not formatted for disc images"


def test_cue_token_rules():
    text = ('REM GENRE "x" 12 00:00:00\r\nCATALOG 0000000000017\r\nPERFORMER JPG750800183\r\n'
            'CDTEXTFILE "a.cdt"\r\nFILE "a b.wav" WAVE\r\n'
            "  TRACK 01 AUDIO\r\n    FLAGS DCP PRE\r\n    TITLE 12\r\n"
            "    ISRC JPG750800183\r\n    PREGAP 00:02:00\r\n    INDEX 01 00:00:00\r\n"
            "    POSTGAP 00:01:00\r\n"
            '  TRACK 02 MODE1/2352\r\n    ISRC 000000000000\r\n    FILE "b.wav" WAVE\r\n'
            "    INDEX 00 03:00:10\r\n    INDEX 01 03:02:10")
    want = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))], True, "JPG750800183"),
                  SheetTrack(2, [SheetIndex(0, Fraction(13510, 75)),
                                 SheetIndex(1, Fraction(13660, 75))], False, None)],
                 "17")
    got = cue.read_cuesheet_string(text)
    assert got == want
    # the catalog is the number's value, as the reference reads it
    assert got.catalog() == "17"
    # a byte order mark in front changes nothing, in bytes or in text
    assert cue.read_cuesheet_string(b"\xef\xbb\xbf" + text.encode("ascii")) == want
    assert cue.read_cuesheet_string(u"\ufeff" + text) == want
    # an ISRC where any value may stand is taken as one token
    assert cue.read_cuesheet_string("TITLE JPG750800183\n" + T) == Sheet(
        [SheetTrack(1, [], True, None)])


def test_toc_rules(tmp_path):
    p = str(tmp_path / "x.toc")
    with open(p, "w") as f:
        f.write('CATALOG "1234567890123"\nTRACK AUDIO\nFILE "a.wav" 0\n')
    with pytest.raises(toc.TOCException) as err:
        toc.read_tocfile(p)
    assert str(err.value) == "no CD_DA TOC header found"
    assert isinstance(err.value, SheetException)
    # read_sheet then tries the cue reader, whose refusal comes out
    with pytest.raises(cue.CueException):
        read_sheet(p)
    with pytest.raises(toc.TOCException):
        toc.read_tocfile(str(tmp_path / "missing.toc"))
    with open(p, "w") as f:
        f.write('CD_DA\nCATALOG "1234567890123"\n\nTRACK AUDIO\nISRC "JPG750800183"\n'
                'AUDIOFILE "a.wav" 0 00:04:00\nINDEX 00:02:00\n'
                'TRACK AUDIO\nFILE "a.wav" 00:04:00 100\nSTART 00:01:30\nINDEX 00:10:00\n')
    assert toc.read_tocfile(p) == Sheet(
        [SheetTrack(1, [SheetIndex(1, Fraction(0)), SheetIndex(2, Fraction(150, 75))], True,
                    "JPG750800183"),
         SheetTrack(2, [SheetIndex(0, Fraction(300, 75)), SheetIndex(1, Fraction(405, 75)),
                        SheetIndex(2, Fraction(750, 75))], True, None)], "1234567890123")


def test_timestamps():
    assert parse_timestamp("01:02:03") == (62 * 75) + 3
    assert parse_timestamp("417") == 417
    assert build_timestamp(4653) == "01:02:03"
    assert build_timestamp(0) == "00:00:00"
    for i in (1, 74, 75, 4499, 4500, 360000):
        assert parse_timestamp(build_timestamp(i)) == i


def test_pcm_lengths_by_hand():
    """8000 Hz, index 1 at CD frames 0, 1, 2 and 4.  A CD frame is 106 2/3
    samples: the gaps of 1, 1 and 2 frames are cut to 106, 106 and 213, the
    difference truncated and not each offset (that would give 106, 107,
    213, the offsets being 106, 213 and 426).  A sheet whose offsets are
    whole samples at 106, 213 and 426 does give 106, 107, 213."""
    sheet = cue.read_cuesheet_string(
        'FILE "a.wav" WAVE\nTRACK 01 AUDIO\nINDEX 01 00:00:00\nTRACK 02 AUDIO\n'
        "INDEX 01 00:00:01\nTRACK 03 AUDIO\nINDEX 01 00:00:02\nTRACK 04 AUDIO\nINDEX 01 00:00:04\n")
    assert list(sheet.pcm_lengths(1000, 8000)) == [106, 106, 213, 575]
    # the last length is what remains and may be 0 or less
    assert list(sheet.pcm_lengths(425, 8000)) == [106, 106, 213, 0]
    assert list(sheet.pcm_lengths(400, 8000)) == [106, 106, 213, -25]
    exact = Sheet([SheetTrack(n + 1, [SheetIndex(1, Fraction(at, 8000))])
                   for n, at in enumerate((0, 106, 213, 426))])
    assert list(exact.pcm_lengths(1000, 8000)) == [106, 107, 213, 574]
    assert list(Sheet([]).pcm_lengths(5, 8000)) == []


def test_image_formatted_and_equality():
    a = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))]),
               SheetTrack(2, [SheetIndex(0, Fraction(3)), SheetIndex(1, Fraction(5))])])
    assert a.image_formatted()
    # every track starting at 0 is a sheet of separate files
    b = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))]),
               SheetTrack(2, [SheetIndex(1, Fraction(0))])])
    assert not b.image_formatted()
    assert Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))])]).image_formatted()
    assert a != b and a == Sheet(list(a.tracks()))
    assert a != Sheet(list(a.tracks()), "1") and a != 5
    assert SheetTrack(1, [], True, "X") != SheetTrack(1, [], True, None)
    assert SheetIndex(1, Fraction(1, 75)) == SheetIndex(1, Fraction(2, 150))
    assert audiotools.sheets.Sheet is Sheet
