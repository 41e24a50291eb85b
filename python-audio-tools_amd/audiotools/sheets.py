"""audiotools.sheets — the layout of a CD as a .cue or .toc file gives it.

A Sheet is a list of SheetTracks, each a list of SheetIndexes whose offsets
are Fractions of seconds from the start of the disc image (reference
audiotools/__init__.py:4265-4479).  audiotools.cue and audiotools.toc read
and write the two text formats; FlacAudio.get_cuesheet / set_cuesheet carry
a Sheet in a FLAC file's CUESHEET block.  Host code only.
"""

__all__ = ["SheetException", "Sheet", "SheetTrack", "SheetIndex", "read_sheet",
           "parse_timestamp", "build_timestamp"]


class SheetException(ValueError):
    """the parent of CueException and TOCException"""


def read_sheet(filename):
    """the Sheet of a .toc or .cue file; SheetException if it parses as
    neither.  The toc reader goes first: its CD_DA header tells a toc file
    apart at once."""
    from . import cue, toc
    try:
        return toc.read_tocfile(filename)
    except SheetException:
        return cue.read_cuesheet(filename)


def _same(a, b, methods):
    """b answers every method of `methods` as a does"""
    for m in methods:
        f = getattr(b, m, None)
        if not callable(f) or getattr(a, m)() != f():
            return False
    return True


class Sheet(object):
    """a CD layout: SheetTracks in order and an optional catalog number"""

    def __init__(self, sheet_tracks, catalog_number=None):
        self.__tracks__ = list(sheet_tracks)
        self.__catalog_number__ = catalog_number

    def __repr__(self):
        return "Sheet(%r, %r)" % (self.__tracks__, self.__catalog_number__)

    def __eq__(self, sheet):
        if not _same(self, sheet, ["catalog"]):
            return False
        if callable(getattr(sheet, "tracks", None)):
            return list(self.tracks()) == list(sheet.tracks())
        return False

    def __ne__(self, sheet):
        return not self.__eq__(sheet)

    __hash__ = None

    def track(self, track_number):
        """the SheetTrack of that number; KeyError without one"""
        for t in self.__tracks__:
            if t.number() == track_number:
                return t
        raise KeyError(track_number)

    def tracks(self):
        return iter(self.__tracks__)

    def catalog(self):
        """the catalog number as a string, or None"""
        return self.__catalog_number__

    def image_formatted(self):
        """True for the sheet of one disc image: every track's earliest
        index lies past that of the track before"""
        firsts = [min(i.offset() for i in t.indexes()) for t in self.__tracks__]
        return all(b > a for a, b in zip(firsts, firsts[1:]))

    def pcm_lengths(self, total_pcm_frames, sample_rate):
        """the tracks' lengths in PCM frames, index 1 to index 1: the
        difference of two offsets times the rate is cut to an integer, not
        each offset, and the last track gets what remains of
        total_pcm_frames (0 or less where the sheet outruns the stream)"""
        if not self.__tracks__:
            return
        for prev, track in zip(self.__tracks__, self.__tracks__[1:]):
            n = int((track.index(1).offset() - prev.index(1).offset()) * sample_rate)
            total_pcm_frames -= n
            yield n
        yield total_pcm_frames


class SheetTrack(object):
    def __init__(self, number, indexes, audio=True, ISRC=None):
        self.__number__ = number
        self.__indexes__ = list(indexes)
        self.__audio__ = audio
        self.__ISRC__ = ISRC

    def __repr__(self):
        return "SheetTrack(%r, %r, %r, %r)" % (self.__number__, self.__indexes__,
                                               self.__audio__, self.__ISRC__)

    def __eq__(self, track):
        if not _same(self, track, ["number", "audio", "ISRC"]):
            return False
        if callable(getattr(track, "indexes", None)):
            return list(self.indexes()) == list(track.indexes())
        return False

    def __ne__(self, track):
        return not self.__eq__(track)

    __hash__ = None

    def index(self, index_number):
        """the SheetIndex of that number; KeyError without one"""
        for i in self.__indexes__:
            if i.number() == index_number:
                return i
        raise KeyError(index_number)

    def indexes(self):
        return iter(self.__indexes__)

    def number(self):
        return self.__number__

    def ISRC(self):
        """the ISRC as a string, or None"""
        return self.__ISRC__

    def audio(self):
        return self.__audio__


class SheetIndex(object):
    def __init__(self, number, offset):
        """offset: seconds from the start of the stream, a Fraction"""
        self.__number__ = number
        self.__offset__ = offset

    def __repr__(self):
        return "SheetIndex(%r, %r)" % (self.__number__, self.__offset__)

    def __eq__(self, index):
        return _same(self, index, ["number", "offset"])

    def __ne__(self, index):
        return not self.__eq__(index)

    __hash__ = None

    def number(self):
        return self.__number__

    def offset(self):
        return self.__offset__


def parse_timestamp(s):
    """"MM:SS:FF" (75 frames a second) or a plain number -> CD frames; the
    caller's pattern has checked the form"""
    if ":" in s:
        m, sec, f = [int(x) for x in s.split(":")]
        return (m * 60 + sec) * 75 + f
    return int(s)


def build_timestamp(i):
    """CD frames -> "MM:SS:FF" """
    return "%2.2d:%2.2d:%2.2d" % (i // 75 // 60, i // 75 % 60, i % 75)
