"""audiotools.toc — cdrdao's .toc files read into Sheets and written from
them (reference audiotools/toc.py:35-205).

The reader goes line by line and takes what it knows: the CD_DA header (a
file without that line is no toc file), CATALOG before the first track, and
inside a track its AUDIOFILE / FILE start, START, INDEX and ISRC lines.
Everything else (CD_TEXT blocks, comments) is passed over.
"""

import re
from fractions import Fraction

from .sheets import (Sheet, SheetException, SheetIndex, SheetTrack, build_timestamp,
                     parse_timestamp)

ERR_TOC_NO_HEADER = u"no CD_DA TOC header found"

_STAMP = r"(\d+:\d+:\d+|\d+)"
_CATALOG = re.compile(r'CATALOG\s*"(.*?)"')
_AUDIOFILE = re.compile(r'(AUDIO)?FILE\s*".*?"\s*' + _STAMP + r"\s*" + _STAMP + "?")
_ISRC = re.compile(r'ISRC\s*"(.*)"')
_START = re.compile(r"START\s*" + _STAMP)
_INDEX = re.compile(r"INDEX\s*" + _STAMP)


class TOCException(SheetException):
    """a toc file that cannot be read or parsed"""


def _parse(lines):
    lines = [line.strip() for line in lines]
    if "CD_DA" not in lines:
        raise TOCException(ERR_TOC_NO_HEADER)
    tracks, catalog = [], None
    number, isrc = None, None
    first, offsets = 1, []  # the number of the track's first index; CD frames

    def close_track():
        tracks.append(SheetTrack(number, [SheetIndex(n, Fraction(o, 75))
                                          for n, o in enumerate(offsets, first)], True, isrc))

    for line in lines:
        if not line:
            continue
        if line == "TRACK AUDIO":
            if number is None:
                number = 1
            else:
                close_track()
                number, isrc = number + 1, None
            continue
        if number is None:
            m = _CATALOG.match(line)
            if m:
                catalog = m.group(1)
            continue
        m = _AUDIOFILE.match(line)
        if m:
            # the track's first index, number 1 until a START line says 0
            first, offsets = 1, [parse_timestamp(m.group(2))]
            continue
        m = _START.match(line)
        if m:
            # the file began with the pregap: what was read is index 0 and
            # index 1 lies START past it
            assert len(offsets) == 1
            first = 0
            offsets.append(offsets[0] + parse_timestamp(m.group(1)))
            continue
        m = _INDEX.match(line)
        if m:
            offsets.append(parse_timestamp(m.group(1)))
            continue
        m = _ISRC.match(line)
        if m:
            isrc = m.group(1)
    if number is not None:
        close_track()
    return Sheet(tracks, catalog)


def read_tocfile(filename):
    """the Sheet of a .toc file; TOCException if it cannot be read or
    parsed"""
    try:
        with open(filename, "rb") as f:
            data = f.read()
    except (IOError, OSError) as err:
        raise TOCException(str(err))
    return _parse(data.decode("latin-1").splitlines())


def write_tocfile(sheet, filename, file):
    """sheet written as a .toc file that names `filename`, to the text file
    object `file`"""
    file.write("CD_DA\n\n")
    if sheet.catalog() is not None and len(sheet.catalog()) > 0:
        file.write("CATALOG \"%s\"\n\n" % (sheet.catalog(),))
    tracks = list(sheet.tracks())

    def stamp(seconds):
        return build_timestamp(int(seconds * 75))

    for track, following in zip(tracks, tracks[1:] + [None]):
        file.write("TRACK AUDIO\n")
        if track.ISRC() is not None:
            file.write("  ISRC \"%s\"\n" % (track.ISRC(),))
        indexes = list(track.indexes())
        if following is not None:
            # the track runs from its earliest index to the next track's
            length = (min(i.offset() for i in following.indexes()) -
                      min(i.offset() for i in indexes))
            file.write("  AUDIOFILE \"%s\" %s %s\n" % (filename, stamp(indexes[0].offset()),
                                                     stamp(length)))
        else:
            file.write("  AUDIOFILE \"%s\" %s\n" % (filename, stamp(indexes[0].offset())))
        rest = indexes[1:]
        if indexes[0].number() == 0:
            file.write("  START %s\n" % (stamp(indexes[1].offset() - indexes[0].offset()),))
            rest = indexes[2:]
        for index in rest:
            file.write("  INDEX %s\n" % (stamp(index.offset()),))
