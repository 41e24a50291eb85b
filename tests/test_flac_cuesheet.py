"""FlacAudio.set_cuesheet / get_cuesheet: the CUESHEET block against a
struct-only builder (tests/flac_cuesheet_port.py) and against the field
values of the reference's own Flac_CUESHEET test objects, its place among the
blocks, and what happens to PADDING and to the frames."""

import json
import os
import shutil
from fractions import Fraction

import pytest

import flac_cuesheet_port as port
from audiotools import FlacAudio, Sheet, SheetIndex, SheetTrack, read_sheet

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sheets")
FIXTURES = os.path.join(HERE, "golden", "fixtures")
with open(os.path.join(GOLDEN, "expected.json")) as _f:
    EXPECTED = json.load(_f)
NAMES = ["sheet%d.%s" % (n + 1, suffix) for suffix in ("cue", "toc") for n in range(4)]
FILES = ["flac-allframes.flac", "flac-seektable.flac"]
STREAMINFO, PADDING, SEEKTABLE, CUESHEET = 0, 1, 3, 5


def _layout(name):
    """the port's plain layout of a golden sheet, from expected.json"""
    e = EXPECTED[int(name[5]) - 1]
    tracks = []
    for n, (isrc, offsets) in enumerate(zip(e["ISRCs"], e["indexes"])):
        # a second index in front of the track's start is index 0 there
        # (INDEX 00 in the cue files, START in the toc files); the sheets of
        # discs 2 to 4 number from 1
        first = 0 if _has_pregap(name, n) else 1
        tracks.append((n + 1, isrc, True, [(first + k, at) for k, at in enumerate(offsets)]))
    return e["catalog"], tracks


def _has_pregap(name, n):
    """by a scan of the text, not by the reader under test: a cue track
    whose first INDEX line is INDEX 00, a toc track with a START line"""
    import re
    with open(os.path.join(GOLDEN, name)) as f:
        text = f.read()
    if name.endswith(".cue"):
        part = re.split(r"\n\s*TRACK ", text)[n + 1]
        return re.search(r"INDEX (\d+)", part).group(1) == "00"
    return "START" in text.split("TRACK AUDIO")[n + 1]


def _copy(tmp_path, fixture, padding=None):
    path = str(tmp_path / fixture)
    shutil.copy(os.path.join(FIXTURES, fixture), path)
    if padding is not None:
        with open(path, "rb") as f:
            data = f.read()
        with open(path, "wb") as f:
            f.write(port.with_padding(data, padding))
    return path


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("fixture", FILES)
@pytest.mark.parametrize("name", NAMES)
def test_round_trip_and_block_bytes(tmp_path, fixture, name):
    path = _copy(tmp_path, fixture)
    before = _read(path)
    old_blocks, old_at = port.blocks(before)
    sheet = read_sheet(os.path.join(GOLDEN, name))
    track = FlacAudio(path)
    assert track.get_cuesheet() is None
    track.set_cuesheet(sheet)
    track = FlacAudio(path)
    assert track.get_cuesheet() == sheet
    after = _read(path)
    blocks, at = port.blocks(after)
    # STREAMINFO, SEEKTABLE, CUESHEET, then whatever followed
    kinds = [k for k, _ in blocks]
    assert kinds == [k for k, _ in old_blocks if k in (STREAMINFO, SEEKTABLE)] + [CUESHEET] + \
        [k for k, _ in old_blocks if k not in (STREAMINFO, SEEKTABLE)]
    body = dict(blocks)[CUESHEET]
    catalog, tracks = _layout(name)
    cdda = (track.sample_rate(), track.channels(), track.bits_per_sample()) == (44100, 2, 16)
    assert body == port.block_body(catalog, tracks, track.total_frames(), track.sample_rate(), cdda)
    # every other block and every frame byte as they were; without PADDING
    # the frames move by the block and its header
    assert [b for b in blocks if b[0] != CUESHEET] == old_blocks
    assert after[at:] == before[old_at:]
    assert at == old_at + 4 + len(body)
    # None changes nothing, and a second sheet takes the first one's place
    track.set_cuesheet(None)
    assert _read(path) == after
    other = read_sheet(os.path.join(GOLDEN, NAMES[(NAMES.index(name) + 1) % 8]))
    track.set_cuesheet(other)
    assert [k for k, _ in port.blocks(_read(path))[0]].count(CUESHEET) == 1
    assert FlacAudio(path).get_cuesheet() == other


def test_known_fields(tmp_path):
    """the first sheet's block, field by field: the values of the
    reference's own Flac_CUESHEET test object for this sheet (lead-in 88200,
    track 2 at 12280380, track 3 at 24807132 with index 1 at +130536, track
    4 at 28954296 with index 1 at +135828), and the general rule of a 44100
    Hz image: a CD frame is 588 samples"""
    path = _copy(tmp_path, "flac-seektable.flac")
    track = FlacAudio(path)
    track.set_cuesheet(read_sheet(os.path.join(GOLDEN, "sheet1.cue")))
    catalog, lead_in, cdda, tracks = port.parse_body(dict(port.blocks(_read(path))[0])[CUESHEET])
    assert catalog == b"4580226563955" + b"\0" * 115
    assert lead_in == 88200 and cdda == 1
    assert len(tracks) == 23
    assert tracks[0] == (0, 1, b"JPG750800183", 0, [(0, 1)])
    assert tracks[1] == (12280380, 2, b"JPG750800212", 0, [(0, 1)])
    assert tracks[2] == (24807132, 3, b"JPG750800214", 0, [(0, 0), (130536, 1)])
    assert tracks[3] == (28954296, 4, b"JPG750800704", 0, [(0, 0), (135828, 1)])
    assert tracks[-1] == (track.total_frames(), 170, b"\0" * 12, 0, [])
    for (offset, number, _, _, indexes), want in zip(tracks, EXPECTED[0]["indexes"]):
        assert [offset + o for o, _ in indexes] == [588 * w for w in want]
    # a mono stream is no CD audio: the flag stays clear
    path = _copy(tmp_path, "flac-allframes.flac")
    FlacAudio(path).set_cuesheet(read_sheet(os.path.join(GOLDEN, "sheet3.toc")))
    catalog, lead_in, cdda, tracks = port.parse_body(dict(port.blocks(_read(path))[0])[CUESHEET])
    assert catalog == b"\0" * 128 and lead_in == 88200 and cdda == 0
    assert tracks[0][2] == b"\0" * 12
    assert tracks[1][0] == 11628 * 588 and tracks[1][4] == [
        (0, 0), ((11760 - 11628) * 588, 1), ((20323 - 11628) * 588, 2),
        ((36644 - 11628) * 588, 3), ((45795 - 11628) * 588, 4)]


def test_each_offset_truncated_alone(tmp_path):
    """an index offset that is no whole sample is cut on its own, and the
    indexes of a track count from its first one's cut"""
    path = _copy(tmp_path, "flac-seektable.flac")
    sheet = Sheet([SheetTrack(1, [SheetIndex(1, Fraction(0))]),
                   SheetTrack(2, [SheetIndex(0, Fraction(10, 44100 * 3)),
                                  SheetIndex(1, Fraction(17, 44100 * 3))], False, "AB")], "12")
    FlacAudio(path).set_cuesheet(sheet)
    catalog, _, _, tracks = port.parse_body(dict(port.blocks(_read(path))[0])[CUESHEET])
    assert catalog == b"12" + b"\0" * 126
    assert tracks[1] == (3, 2, b"AB" + b"\0" * 10, 1, [(0, 0), (2, 1)])
    got = FlacAudio(path).get_cuesheet()
    assert got.catalog() == "12" and got.track(2).ISRC() == "AB" and not got.track(2).audio()
    assert [i.offset() for i in got.track(2).indexes()] == [Fraction(3, 44100), Fraction(5, 44100)]


@pytest.mark.parametrize("fixture", FILES)
def test_padding_absorbs_the_block(tmp_path, fixture):
    sheet = read_sheet(os.path.join(GOLDEN, "sheet4.cue"))
    # room enough: the file keeps its size and the frames their place
    path = _copy(tmp_path, fixture, padding=4096)
    before = _read(path)
    old_blocks, old_at = port.blocks(before)
    FlacAudio(path).set_cuesheet(sheet)
    after = _read(path)
    blocks, at = port.blocks(after)
    assert len(after) == len(before) and at == old_at
    assert after[at:] == before[old_at:]
    body = dict(blocks)[CUESHEET]
    assert blocks[-1] == (PADDING, b"\0" * (4096 - 4 - len(body)))
    assert [k for k, _ in blocks] == [k for k, _ in old_blocks[:-1]] + [CUESHEET, PADDING]
    assert FlacAudio(path).get_cuesheet() == sheet
    # too little room: PADDING stays as it is, the file grows and the frames move
    path = _copy(tmp_path, fixture, padding=100)
    before = _read(path)
    old_blocks, old_at = port.blocks(before)
    FlacAudio(path).set_cuesheet(sheet)
    after = _read(path)
    blocks, at = port.blocks(after)
    assert blocks[-1] == (PADDING, b"\0" * 100)
    assert at == old_at + 4 + len(body) and len(after) == len(before) + 4 + len(body)
    assert after[at:] == before[old_at:]
    assert FlacAudio(path).get_cuesheet() == sheet


def test_id3_prefix_kept(tmp_path):
    """a file with an ID3v2 tag in front keeps it, and the block goes in
    behind the fLaC marker"""
    path = _copy(tmp_path, "flac-id3.flac")
    before = _read(path)
    marker = before.index(b"fLaC")
    assert marker > 0
    sheet = read_sheet(os.path.join(GOLDEN, "sheet2.cue"))
    FlacAudio(path).set_cuesheet(sheet)
    after = _read(path)
    assert after[:marker + 4] == before[:marker + 4]
    assert FlacAudio(path).get_cuesheet() == sheet
