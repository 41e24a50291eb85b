"""audiotools.cue — .cue files read into Sheets and written from them
(reference audiotools/cue.py:49-360, messages text.py:550-565).

The reader is a tokenizer and a parser over its tokens, as the reference's
is, so that the same files are taken and refused with the same words.  What
a sheet says beyond catalog, tracks, ISRCs and indexes (titles, performers,
flags, gaps, file names) is read and dropped.
"""

import re
from fractions import Fraction

from .sheets import Sheet, SheetException, SheetIndex, SheetTrack, build_timestamp

SPACE, TAG, NUMBER, EOL, STRING, ISRC, TIMESTAMP = 0x0, 0x1, 0x2, 0x4, 0x8, 0x10, 0x20

ERR_CUE_INVALID_TOKEN = u"invalid token at char %d"
ERR_CUE_ERROR = u"%(error)s at line %(line)d"
ERR_CUE_INVALID_TRACK_NUMBER = u"invalid track number"
ERR_CUE_INVALID_TRACK_TYPE = u"invalid track type"
ERR_CUE_MISSING_VALUE = u"missing value"
ERR_CUE_EXCESS_DATA = u"excess data"
ERR_CUE_MISSING_FILENAME = u"missing filename"
ERR_CUE_MISSING_FILETYPE = u"missing file type"
ERR_CUE_INVALID_TAG = u"invalid tag %(tag)s at line %(line)d"
ERR_CUE_INVALID_DATA = u"invalid data"
ERR_CUE_INVALID_FLAG = u"invalid flag"
ERR_CUE_INVALID_TIMESTAMP = u"invalid timestamp"
ERR_CUE_INVALID_INDEX_NUMBER = u"invalid index number"
ERR_CUE_MISSING_TAG = u"missing tag at line %d"
ERR_CUE_IOERROR = u"unable to read cuesheet"
ERR_CUE_INVALID_FORMAT = u"cuesheet not formatted for disc images"


class CueException(SheetException):
    """a cuesheet that cannot be read or parsed"""


# tried in this order at the head of what is left: an ISRC wins over a
# number, a timestamp over a number, a newline run over a bare word
_PATTERNS = [(re.compile(p), kind) for p, kind in (
    (r"[A-Z]{2}[A-Za-z0-9]{3}[0-9]{7}", ISRC),
    (r"[0-9]{1,3}:[0-9]{1,2}:[0-9]{1,2}", TIMESTAMP),
    (r"[0-9]+", NUMBER),
    (r"[\r\n]+", EOL),
    (r'".+?"', STRING),
    (r"\S+", STRING),
    (r"[ ]+", SPACE))]
_ALL_CAPS = re.compile(r"^[A-Z]+$")
_BOM = u"\xef\xbb\xbf"  # the UTF-8 byte order mark in a latin-1 reading


def _text(data):
    """cuesheet data as a string with one character per byte"""
    if isinstance(data, (bytes, bytearray)):
        return bytes(data).decode("latin-1")
    return _BOM + data[1:] if data.startswith(u"\ufeff") else data


def _tokens(data):
    """(value, kind, line number) of every token of the sheet.  A run of
    line ends is one EOL token that counts one line and carries the number
    of the line it opens.  CueException where no pattern fits."""
    full = len(data)
    data = data.lstrip(_BOM)
    pos, line = 0, 1
    while pos < len(data):
        for pattern, kind in _PATTERNS:
            m = pattern.match(data, pos)
            if m is not None:
                break
        else:
            raise CueException(ERR_CUE_INVALID_TOKEN % (full - (len(data) - pos)))
        text = m.group()
        pos = m.end()
        if kind == NUMBER:
            yield (int(text), NUMBER, line)
        elif kind == EOL:
            line += 1
            yield (text, EOL, line)
        elif kind == STRING:
            if _ALL_CAPS.match(text):
                yield (text, TAG, line)
            else:
                yield (text.strip('"'), STRING, line)
        elif kind == TIMESTAMP:
            m_, s_, f_ = [int(x) for x in text.split(":")]
            yield ((m_ * 60 + s_) * 75 + f_, TIMESTAMP, line)
        elif kind == ISRC:
            yield (text, ISRC, line)


def _take(tokens, accept, error):
    """the next token's value if its kind is among `accept` (kinds or-ed
    together), else CueException "<error> at line <n>"; StopIteration at the
    end of the sheet"""
    value, kind, line = next(tokens)
    if kind & accept:
        return value
    raise CueException(ERR_CUE_ERROR % {"error": error, "line": line})


def _skip_line(tokens):
    while next(tokens)[1] != EOL:
        pass


_ANY_VALUE = STRING | TAG | NUMBER | ISRC


def _parse(tokens):
    tracks, catalog = [], None
    number, indexes, audio, isrc = None, [], False, None

    def close_track():
        if number is not None:
            tracks.append(SheetTrack(number, indexes, audio, isrc))

    try:
        while True:
            token, kind, line = next(tokens)
            if kind != TAG:
                raise CueException(ERR_CUE_MISSING_TAG % (line,))
            if token == "REM":
                _skip_line(tokens)
            elif token == "TRACK":
                close_track()
                number = _take(tokens, NUMBER, ERR_CUE_INVALID_TRACK_NUMBER)
                indexes, isrc = [], None
                audio = _take(tokens, TAG | STRING, ERR_CUE_INVALID_TRACK_TYPE) == "AUDIO"
                _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
            elif number is None:
                # the sheet's head, before any track
                if token == "CATALOG":
                    catalog = str(_take(tokens, STRING | NUMBER, ERR_CUE_MISSING_VALUE))
                    _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
                elif token in ("CDTEXTFILE", "PERFORMER", "SONGWRITER", "TITLE"):
                    _take(tokens, _ANY_VALUE, ERR_CUE_MISSING_VALUE)
                    _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
                elif token == "FILE":
                    _take(tokens, STRING, ERR_CUE_MISSING_FILENAME)
                    _take(tokens, STRING | TAG, ERR_CUE_MISSING_FILETYPE)
                    _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
                else:
                    raise CueException(ERR_CUE_INVALID_TAG % {"tag": token, "line": line})
            elif token == "ISRC":
                isrc = _take(tokens, ISRC | NUMBER, ERR_CUE_MISSING_VALUE)
                if isinstance(isrc, int):
                    isrc = None  # a run of digits (mostly zeroes) is no ISRC
                _take(tokens, EOL, ERR_CUE_INVALID_DATA)
            elif token in ("PERFORMER", "SONGWRITER", "TITLE"):
                _take(tokens, _ANY_VALUE, ERR_CUE_MISSING_VALUE)
                _take(tokens, EOL, ERR_CUE_INVALID_DATA)
            elif token == "FLAGS":
                flag = _take(tokens, STRING | TAG | EOL, ERR_CUE_INVALID_FLAG)
                while "\n" not in flag and "\r" not in flag:
                    flag = _take(tokens, STRING | TAG | EOL, ERR_CUE_INVALID_FLAG)
            elif token in ("PREGAP", "POSTGAP"):
                _take(tokens, TIMESTAMP, ERR_CUE_INVALID_TIMESTAMP)
                _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
            elif token == "INDEX":
                n = _take(tokens, NUMBER, ERR_CUE_INVALID_INDEX_NUMBER)
                at = _take(tokens, TIMESTAMP, ERR_CUE_INVALID_TIMESTAMP)
                indexes.append(SheetIndex(n, Fraction(at, 75)))
                _take(tokens, EOL, ERR_CUE_EXCESS_DATA)
            elif token == "FILE":
                _skip_line(tokens)
            else:
                raise CueException(ERR_CUE_INVALID_TAG % {"tag": token, "line": line})
    except StopIteration:
        # the sheet ended, in the middle of a line or not
        close_track()
        return Sheet(tracks, catalog)


def read_cuesheet(filename):
    """the Sheet of a .cue file; CueException if it cannot be read or
    parsed"""
    try:
        with open(filename, "rb") as f:
            data = f.read()
    except (IOError, OSError):
        raise CueException(ERR_CUE_IOERROR)
    return read_cuesheet_string(data)


def read_cuesheet_string(cuesheet):
    """the Sheet of cuesheet text (str or bytes); CueException if it does
    not parse"""
    return _parse(_tokens(_text(cuesheet)))


def write_cuesheet(sheet, filename, file):
    """sheet written as a .cue file that names `filename`, to the text file
    object `file`"""
    if sheet.catalog() is not None:
        file.write("CATALOG %s\r\n" % (sheet.catalog(),))
    file.write("FILE \"%s\" WAVE\r\n" % (filename,))
    for track in sheet.tracks():
        file.write("  TRACK %2.2d %s\r\n" % (track.number(),
                                             "AUDIO" if track.audio() else "BINARY"))
        if track.ISRC() is not None:
            file.write("    ISRC %s\r\n" % (track.ISRC(),))
        for index in track.indexes():
            file.write("    INDEX %2.2d %s\r\n" % (index.number(),
                                                   build_timestamp(int(index.offset() * 75))))
