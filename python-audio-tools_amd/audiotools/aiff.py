"""audiotools.aiff — AIFF on either side of the transcode path.

`AiffReader` (reference audiotools/aiff.py:350-482) walks the chunks to
"COMM" and "SSND" and hands out pcm.FrameLists of the big-endian signed
samples; `parse_comm` (:327-347) decodes the COMM chunk, whose sample rate
is an 80-bit IEEE extended value (`parse_ieee_extended` /
`build_ieee_extended`, :25-59).

`AiffAudio` (:491-1050) carries what track2track / trackverify call on an
AIFF file: `to_pcm`, `convert` (AudioFile's), `from_pcm` (:756-855),
`chunks` / `aiff_from_chunks`, `aiff_header_footer` / `from_aiff` and
`verify` with the header validators they use (:69-203).  Not covered:
ID3 metadata (get_metadata and friends), clean(), AIFF-C.

Two files the reference refuses are read: one whose SSND chunk comes before
COMM (AiffReader walks on to COMM and returns to the sound data), and one
whose last, odd-sized chunk ends the file without its pad byte
(aiff_header_footer and validate_footer accept that at the very end).

Host byte work here: one file at a time the samples are converted by
pcm.FrameList, with no GPU.  Batches of files go through
decoders.decode_pcm_batch / encoders.encode_aiff_batch, which unpack and
pack the bytes on the device (csrc/pcm_bytes.hip).
"""

import io
import struct
from math import frexp

from . import pcm as _pcm
from . import AudioFile, ChannelMask, EncodingError, DecodingError, InvalidFile
from . import FRAMELIST_SIZE

ERR_AIFF_NOT_AIFF = u"not an AIFF file"
ERR_AIFF_INVALID_AIFF = u"invalid AIFF file"
ERR_AIFF_INVALID_CHUNK_ID = u"invalid AIFF chunk ID"
ERR_AIFF_INVALID_CHUNK = u"invalid AIFF chunk"
ERR_AIFF_MULTIPLE_COMM_CHUNKS = u"multiple COMM chunks found"
ERR_AIFF_PREMATURE_SSND_CHUNK = u"SSND chunk found before fmt"
ERR_AIFF_MULTIPLE_SSND_CHUNKS = u"multiple SSND chunks found"
ERR_AIFF_NO_SSND_CHUNK = u"SSND chunk not found"
ERR_AIFF_HEADER_EXTRA_SSND = u"extra data after SSND chunk header"
ERR_AIFF_HEADER_MISSING_SSND = u"missing data in SSND chunk header"
ERR_AIFF_HEADER_IOERROR = u"I/O error reading header data"
ERR_AIFF_FOOTER_IOERROR = u"I/O error reading footer data"
ERR_AIFF_TRUNCATED_SSND_CHUNK = u"premature end of SSND chunk"
ERR_AIFF_INVALID_SIZE = u"total aiff file size mismatch"
ERR_AIFF_TOO_LARGE = u"PCM data too large for aiff file"
ERR_NEGATIVE_SEEK = u"cannot seek to negative value"

PRINTABLE_ASCII = frozenset(range(0x20, 0x7E + 1))


def _printable(chunk_id):
    return frozenset(chunk_id).issubset(PRINTABLE_ASCII)


def parse_ieee_extended(data):
    """the value of a 10-byte IEEE extended field (bytes, or a file object
    it is read from; IOError if short): 0, the largest double for an
    infinity or NaN exponent, else a float (reference aiff.py:25-36)"""
    if hasattr(data, "read"):
        data = data.read(10)
    if len(data) < 10:
        raise IOError("I/O error reading IEEE extended value")
    head, mantissa = struct.unpack(">HQ", data[:10])
    signed, exponent = head >> 15, head & 0x7FFF
    if exponent == 0 and mantissa == 0:
        return 0
    if exponent == 0x7FFF:
        return 1.79769313486231e+308
    try:
        f = mantissa * (2.0 ** (exponent - 16383 - 63))
    except OverflowError:
        f = float("inf")
    if f == float("inf"):
        # beyond a double, where the reference's expression raises or int()
        # of its result does: the value it gives for an infinity serves
        f = 1.79769313486231e+308
    return -f if signed else f


def build_ieee_extended(value):
    """value -> its 10 bytes as an IEEE extended field (reference
    aiff.py:39-59, which writes them to a BitstreamWriter)"""
    signed = 1 if value < 0 else 0
    fmant, exponent = frexp(abs(value))
    if exponent > 16384 or fmant >= 1:
        exponent, mantissa = 0x7FFF, 0
    else:
        exponent += 16382
        mantissa = int(fmant * (2 ** 64))
    return struct.pack(">HQ", (signed << 15) | exponent, mantissa)


def pad_data(pcm_frames, channels, bits_per_sample):
    """nonzero if a stream of these dimensions needs a pad byte after its
    sound data (reference aiff.py:62-66)"""
    return (pcm_frames * channels * (bits_per_sample // 8)) % 2


class _Reader(object):
    """big-endian field reader over bytes; IOError past the end (the
    BitstreamReader behaviour the validators rely on)"""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def chunk_body(self, chunk_size):
        """a chunk's data with its pad byte.  The pad byte of an odd chunk
        that ends the data exactly may be missing (files in the wild, and
        the reference's own aiff-metadata.aiff, end so; the reference's
        read of chunk_size + 1 bytes fails on them)"""
        if chunk_size % 2 and self.pos + chunk_size == len(self.data):
            return self.take(chunk_size)
        return self.take(chunk_size + chunk_size % 2)

    def take(self, n):
        if self.pos + n > len(self.data):
            raise IOError("I/O error")
        b = self.data[self.pos:self.pos + n]
        self.pos += n
        return b

    def chunk_header(self):
        return struct.unpack(">4sI", self.take(8))


def validate_header(header):
    """header bytes as aiff_header_footer returns them -> (total size, SSND
    sound data size); ValueError if invalid (reference aiff.py:69-154)"""
    header_size = len(header)
    r = _Reader(header)
    try:
        form, remaining_size, aiff = struct.unpack(">4sI4s", r.take(12))
        if form != b"FORM":
            raise ValueError(ERR_AIFF_NOT_AIFF)
        if aiff != b"AIFF":
            raise ValueError(ERR_AIFF_INVALID_AIFF)
        total_size = remaining_size + 8
        header_size -= 12
        comm_found = False
        while header_size > 0:
            chunk_id, chunk_size = r.chunk_header()
            if not _printable(chunk_id):
                raise ValueError(ERR_AIFF_INVALID_CHUNK)
            header_size -= 8
            if chunk_id == b"COMM":
                if comm_found:
                    raise ValueError(ERR_AIFF_MULTIPLE_COMM_CHUNKS)
                comm_found = True
                r.take(chunk_size + chunk_size % 2)
                header_size -= chunk_size + chunk_size % 2
            elif chunk_id == b"SSND":
                if not comm_found:
                    raise ValueError(ERR_AIFF_PREMATURE_SSND_CHUNK)
                if header_size > 8:
                    raise ValueError(ERR_AIFF_HEADER_EXTRA_SSND)
                if header_size < 8:
                    raise ValueError(ERR_AIFF_HEADER_MISSING_SSND)
                return (total_size, chunk_size - 8)
            else:
                r.take(chunk_size + chunk_size % 2)
                header_size -= chunk_size + chunk_size % 2
        raise ValueError(ERR_AIFF_NO_SSND_CHUNK)
    except IOError:
        raise ValueError(ERR_AIFF_HEADER_IOERROR)


def validate_footer(footer, ssnd_bytes_written):
    """True if the footer after the SSND chunk is valid; ValueError
    otherwise (reference aiff.py:157-203)"""
    total_size = len(footer)
    r = _Reader(footer)
    try:
        if ssnd_bytes_written % 2:
            r.take(1)
            total_size -= 1
        while total_size > 0:
            chunk_id, chunk_size = r.chunk_header()
            if not _printable(chunk_id):
                raise ValueError(ERR_AIFF_INVALID_CHUNK)
            total_size -= 8
            if chunk_id == b"COMM":
                raise ValueError(ERR_AIFF_MULTIPLE_COMM_CHUNKS)
            if chunk_id == b"SSND":
                raise ValueError(ERR_AIFF_MULTIPLE_SSND_CHUNKS)
            total_size -= len(r.chunk_body(chunk_size))
        return True
    except IOError:
        raise ValueError(ERR_AIFF_FOOTER_IOERROR)


class AIFF_Chunk(object):
    """a raw AIFF chunk: id, declared size, data (reference aiff.py:211-265)"""

    def __init__(self, chunk_id, chunk_size, chunk_data):
        self.id = chunk_id
        self.__size = chunk_size
        self.__data = chunk_data

    def __repr__(self):
        return "AIFF_Chunk(%r)" % (self.id,)

    def size(self):
        return self.__size

    def total_size(self):
        return 8 + self.__size + (self.__size % 2)

    def data(self):
        return io.BytesIO(self.__data)

    def verify(self):
        return self.__size == len(self.__data)

    def write(self, f):
        f.write(self.id)
        f.write(struct.pack(">I", self.__size))
        f.write(self.__data)
        if self.__size % 2:
            f.write(b"\0")
        return self.total_size()


def parse_comm(comm):
    """a COMM chunk's data (bytes, or a file object it is read from) ->
    (channels, total sample frames, bits_per_sample, sample_rate,
    ChannelMask); IOError when it ends early (reference aiff.py:327-347)"""
    if hasattr(comm, "read"):
        comm = comm.read(18)
    if len(comm) < 18:
        raise IOError("I/O error reading COMM chunk")
    channels, total_sample_frames, bits_per_sample = struct.unpack(">HIH", comm[:8])
    sample_rate = int(parse_ieee_extended(comm[8:18]))
    channel_mask = (ChannelMask.from_channels(channels) if 1 <= channels <= 2
                    else ChannelMask(0))
    return (channels, total_sample_frames, bits_per_sample, sample_rate, channel_mask)


def aiff_header(sample_rate, channels, bits_per_sample, total_pcm_frames, data_size):
    """everything before an AIFF file's sound data as from_pcm writes it:
    FORM, an 18-byte COMM, the SSND header and its two zero words;
    data_size counts those two words"""
    total_size = 4 + 8 + 18 + 8 + data_size + data_size % 2
    return (struct.pack(">4sI4s", b"FORM", total_size, b"AIFF") +
            struct.pack(">4sIHIH", b"COMM", 18, channels, total_pcm_frames, bits_per_sample) +
            build_ieee_extended(sample_rate) +
            struct.pack(">4sIII", b"SSND", data_size, 0, 0))


class AiffReader(object):
    """PCMReader over an AIFF file's "SSND" chunk
    (reference audiotools/aiff.py:350-482)"""

    def __init__(self, aiff_filename):
        self.file = open(aiff_filename, "rb")
        try:
            self._open()
        except Exception:
            self.file.close()
            raise

    def _open(self):
        head = self.file.read(12)
        if len(head) < 12:
            raise InvalidAIFF(ERR_AIFF_INVALID_AIFF)
        form, total_size, aiff = struct.unpack(">4sI4s", head)
        if form != b"FORM":
            raise ValueError(ERR_AIFF_NOT_AIFF)
        if aiff != b"AIFF":
            raise ValueError(ERR_AIFF_INVALID_AIFF)
        total_size -= 4
        comm_read = False
        early_ssnd = None
        # walk the chunks until "SSND" (aiff.py:380-432).  Where the reference
        # refuses an SSND chunk that comes before COMM, the walk goes on here
        # to the COMM chunk and comes back to the sound data, as the usual
        # AIFF readers do; with no COMM after it the reference's error stands.
        while total_size > 0:
            hdr = self.file.read(8)
            if len(hdr) < 8:
                raise ValueError(ERR_AIFF_INVALID_AIFF)
            chunk_id, chunk_size = struct.unpack(">4sI", hdr)
            if not _printable(chunk_id):
                raise ValueError(ERR_AIFF_INVALID_CHUNK_ID)
            total_size -= 8
            if chunk_id == b"COMM":
                # the 18 bytes of its fields are read, whatever its size says
                (self.channels, self.total_pcm_frames, self.bits_per_sample,
                 self.sample_rate, channel_mask) = parse_comm(self.file)
                self.channel_mask = int(channel_mask)
                self.bytes_per_pcm_frame = (self.bits_per_sample // 8) * self.channels
                self.remaining_pcm_frames = self.total_pcm_frames
                comm_read = True
                if early_ssnd is not None:
                    self.ssnd_chunk_offset = early_ssnd
                    self.file.seek(early_ssnd, 0)
                    return
            elif chunk_id == b"SSND":
                # the offset / block-size words are skipped, not applied
                self.file.read(8)
                if comm_read:
                    self.ssnd_chunk_offset = self.file.tell()
                    return
                if early_ssnd is None:
                    early_ssnd = self.file.tell()
                self.file.read(max(chunk_size - 8, 0))
            else:
                self.file.read(chunk_size)
            if chunk_size % 2:
                if len(self.file.read(1)) < 1:
                    raise ValueError(ERR_AIFF_INVALID_CHUNK)
                total_size -= chunk_size + 1
            else:
                total_size -= chunk_size
        if early_ssnd is not None:
            raise ValueError(ERR_AIFF_PREMATURE_SSND_CHUNK)
        raise ValueError(ERR_AIFF_NO_SSND_CHUNK)

    def read(self, pcm_frames):
        """a FrameList of min(max(pcm_frames, 1), remaining) frames
        (aiff.py:434-456); IOError if the SSND chunk ends early"""
        requested = min(max(pcm_frames, 1), self.remaining_pcm_frames)
        nbytes = self.bytes_per_pcm_frame * requested
        data = self.file.read(nbytes)
        if len(data) < nbytes:
            raise IOError(ERR_AIFF_TRUNCATED_SSND_CHUNK)
        self.remaining_pcm_frames -= requested
        return _pcm.FrameList(data, self.channels, self.bits_per_sample, True, True)

    def seek(self, pcm_frame_offset):
        """position at a PCM frame; returns the frames actually skipped
        (aiff.py:458-477)"""
        if pcm_frame_offset < 0:
            raise ValueError(ERR_NEGATIVE_SEEK)
        pcm_frame_offset = min(pcm_frame_offset, self.total_pcm_frames)
        self.file.seek(self.ssnd_chunk_offset +
                       pcm_frame_offset * self.bytes_per_pcm_frame, 0)
        self.remaining_pcm_frames = self.total_pcm_frames - pcm_frame_offset
        return pcm_frame_offset

    def close(self):
        self.file.close()


class InvalidAIFF(InvalidFile):
    """reference audiotools/aiff.py:485-488"""


class AiffAudio(AudioFile):
    """an AIFF file (reference audiotools/aiff.py:491-1050)"""

    SUFFIX = "aiff"
    NAME = SUFFIX
    DESCRIPTION = u"Audio Interchange File Format"
    PRINTABLE_ASCII = PRINTABLE_ASCII

    def __init__(self, filename):
        """the stream attributes from the first "COMM" chunk that parses; a
        truncated one is passed over (aiff.py:500-529)"""
        AudioFile.__init__(self, filename)
        self.__channels = 0
        self.__bits_per_sample = 0
        self.__sample_rate = 0
        self.__channel_mask = ChannelMask(0)
        self.__total_sample_frames = 0
        try:
            for chunk in self.chunks():
                if chunk.id == b"COMM":
                    try:
                        (self.__channels, self.__total_sample_frames,
                         self.__bits_per_sample, self.__sample_rate,
                         self.__channel_mask) = parse_comm(chunk.data())
                        break
                    except IOError:
                        continue
        except IOError:
            raise InvalidAIFF("I/O error reading wave")

    def bits_per_sample(self):
        return self.__bits_per_sample

    def channels(self):
        return self.__channels

    def channel_mask(self):
        return self.__channel_mask

    def lossless(self):
        return True

    def total_frames(self):
        return self.__total_sample_frames

    def sample_rate(self):
        return self.__sample_rate

    def chunks(self):
        """AIFF_Chunk for every chunk, data read as far as the file goes
        (aiff.py:561-616; the reference defers chunks of 1 MiB or more to a
        file-backed chunk, here they are read the same way); InvalidAIFF on
        a broken header, chunk id or missing pad byte"""
        with open(self.filename, "rb") as aiff_file:
            head = aiff_file.read(12)
            if len(head) < 12:
                raise InvalidAIFF(ERR_AIFF_INVALID_AIFF)
            form, total_size, aiff = struct.unpack(">4sI4s", head)
            if form != b"FORM":
                raise InvalidAIFF(ERR_AIFF_NOT_AIFF)
            if aiff != b"AIFF":
                raise InvalidAIFF(ERR_AIFF_INVALID_AIFF)
            total_size -= 4
            while total_size > 0:
                hdr = aiff_file.read(8)
                if len(hdr) < 8:
                    raise InvalidAIFF(ERR_AIFF_INVALID_AIFF)
                chunk_id, chunk_size = struct.unpack(">4sI", hdr)
                if not _printable(chunk_id):
                    raise InvalidAIFF(ERR_AIFF_INVALID_CHUNK_ID)
                total_size -= 8
                yield AIFF_Chunk(chunk_id, chunk_size, aiff_file.read(chunk_size))
                if chunk_size % 2:
                    if len(aiff_file.read(1)) < 1:
                        raise InvalidAIFF(ERR_AIFF_INVALID_CHUNK)
                    total_size -= chunk_size + 1
                else:
                    total_size -= chunk_size

    @classmethod
    def aiff_from_chunks(cls, aiff_file, chunk_iter):
        """an AIFF file written to the seekable file object from
        AIFF_Chunk-like objects (aiff.py:618-639)"""
        start = aiff_file.tell()
        aiff_file.write(struct.pack(">4sI4s", b"FORM", 4, b"AIFF"))
        total_size = 4
        for chunk in chunk_iter:
            total_size += chunk.write(aiff_file)
        aiff_file.seek(start)
        aiff_file.write(struct.pack(">4sI4s", b"FORM", total_size, b"AIFF"))

    def to_pcm(self):
        return AiffReader(self.filename)

    @classmethod
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None):
        """write pcmreader's data as an AIFF file (aiff.py:756-855): a
        placeholder header, the big-endian samples, a pad byte after an odd
        amount of data, then the header again with the counted sizes"""
        try:
            f = open(filename, "wb")
        except IOError as err:
            raise EncodingError(str(err))
        try:
            f.write(aiff_header(pcmreader.sample_rate, pcmreader.channels,
                                pcmreader.bits_per_sample, 0, 0))
            data_size = 8
            frames = 0
            try:
                framelist = pcmreader.read(FRAMELIST_SIZE)
                while len(framelist) > 0:
                    data = framelist.to_bytes(True, True)
                    f.write(data)
                    data_size += len(data)
                    frames += framelist.frames
                    framelist = pcmreader.read(FRAMELIST_SIZE)
            except (IOError, ValueError) as err:
                cls.__unlink__(filename)
                raise EncodingError(str(err))
            except Exception:
                cls.__unlink__(filename)
                raise
            if data_size % 2:
                f.write(b"\0")
            try:
                pcmreader.close()
            except DecodingError as err:
                cls.__unlink__(filename)
                raise EncodingError(err.error_message)
            f.flush()
            if 4 + 8 + 18 + 8 + data_size + data_size % 2 >= (1 << 32):
                cls.__unlink__(filename)
                raise EncodingError(ERR_AIFF_TOO_LARGE)
            f.seek(0, 0)
            f.write(aiff_header(pcmreader.sample_rate, pcmreader.channels,
                                pcmreader.bits_per_sample, frames, data_size))
        finally:
            f.close()
        return AiffAudio(filename)

    def has_foreign_aiff_chunks(self):
        return set([b"COMM", b"SSND"]) != set(c.id for c in self.chunks())

    def aiff_header_footer(self):
        """(everything up to the SSND chunk's sound data, everything after
        it) (aiff.py:862-926); InvalidAIFF on a broken header or chunk id,
        IOError if the file ends inside a chunk"""
        with open(self.filename, "rb") as f:
            r = _Reader(f.read())
        head, tail = [], []
        cur = head
        form, size, aiff = struct.unpack(">4sI4s", r.take(12))
        if form != b"FORM":
            raise InvalidAIFF(ERR_AIFF_NOT_AIFF)
        if aiff != b"AIFF":
            raise InvalidAIFF(ERR_AIFF_INVALID_AIFF)
        cur.append(struct.pack(">4sI4s", form, size, aiff))
        total_size = size - 4
        while total_size > 0:
            chunk_id, chunk_size = r.chunk_header()
            if not _printable(chunk_id):
                raise InvalidAIFF(ERR_AIFF_INVALID_CHUNK_ID)
            cur.append(struct.pack(">4sI", chunk_id, chunk_size))
            total_size -= 8
            if chunk_id != b"SSND":
                cur.append(r.chunk_body(chunk_size))
                total_size -= chunk_size + chunk_size % 2
            else:
                # the two alignment words belong to the header
                cur.append(r.take(8))
                if chunk_size < 8:
                    raise IOError("I/O error")
                r.take(chunk_size - 8)
                cur = tail
                if chunk_size % 2:
                    cur.append(r.take(1))
                    total_size -= chunk_size + 1
                else:
                    total_size -= chunk_size
        return (b"".join(head), b"".join(tail))

    @classmethod
    def from_aiff(cls, filename, header, pcmreader, footer, compression=None):
        """header + pcmreader's big-endian bytes + footer written as a new
        file, which restores the file they were taken from
        (aiff.py:928-997); EncodingError if they do not fit together"""
        try:
            (total_size, ssnd_size) = validate_header(header)
        except ValueError as err:
            raise EncodingError(str(err))
        try:
            with open(filename, "wb") as f:
                f.write(header)
                written = 0
                s = pcmreader.read(FRAMELIST_SIZE).to_bytes(True, True)
                while len(s) > 0:
                    written += len(s)
                    f.write(s)
                    s = pcmreader.read(FRAMELIST_SIZE).to_bytes(True, True)
                if ssnd_size != written:
                    cls.__unlink__(filename)
                    raise EncodingError(ERR_AIFF_TRUNCATED_SSND_CHUNK)
                try:
                    validate_footer(footer, written)
                    f.write(footer)
                except ValueError as err:
                    cls.__unlink__(filename)
                    raise EncodingError(str(err))
            if len(header) + ssnd_size + len(footer) != total_size:
                cls.__unlink__(filename)
                raise EncodingError(ERR_AIFF_INVALID_SIZE)
            return cls(filename)
        except EncodingError:
            raise
        except DecodingError as err:
            cls.__unlink__(filename)
            raise EncodingError(err.error_message)
        except IOError as err:
            cls.__unlink__(filename)
            raise EncodingError(str(err))

    def verify(self, progress=None):
        """True if header, SSND chunk and footer are consistent; InvalidAIFF
        otherwise (aiff.py:999-1050)"""
        from . import CounterPCMReader, to_pcm_progress, transfer_framelist_data
        try:
            (header, footer) = self.aiff_header_footer()
        except InvalidAIFF:
            raise
        except (IOError, ValueError) as err:
            raise InvalidAIFF(str(err))
        try:
            (total_size, data_size) = validate_header(header)
        except ValueError as err:
            raise InvalidAIFF(str(err))
        try:
            counter = CounterPCMReader(to_pcm_progress(self, progress))
        except (IOError, ValueError) as err:
            raise InvalidAIFF(str(err))
        try:
            transfer_framelist_data(counter, lambda f: f)
        except IOError:
            raise InvalidAIFF(ERR_AIFF_TRUNCATED_SSND_CHUNK)
        finally:
            counter.close()
        data_bytes_written = counter.bytes_written()
        if data_size != data_bytes_written:
            raise InvalidAIFF(ERR_AIFF_TRUNCATED_SSND_CHUNK)
        try:
            validate_footer(footer, data_bytes_written)
        except ValueError:
            raise InvalidAIFF(ERR_AIFF_INVALID_SIZE)
        if len(header) + data_size + len(footer) != total_size:
            raise InvalidAIFF(ERR_AIFF_INVALID_SIZE)
        return True
