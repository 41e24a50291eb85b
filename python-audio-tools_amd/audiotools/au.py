"""audiotools.au — Sun AU on either side of the transcode path.

`AuReader` (reference audiotools/au.py:34-102) reads the 24-byte big-endian
header (magic ".snd", data offset, data size, encoding, sample rate,
channels; encodings 2, 3, 4 are 8, 16, 24-bit signed linear PCM) and hands
out pcm.FrameLists; `AuAudio` (:105-285) carries `to_pcm`, `from_pcm`,
`pcm_split`, `channel_mask` and AudioFile's `convert` / `verify`.

Host byte work here, with no GPU; batches of files go through
decoders.decode_pcm_batch / encoders.encode_au_batch, which unpack and pack
the bytes on the device (csrc/pcm_bytes.hip).
"""

import struct

from . import pcm as _pcm
from . import AudioFile, ChannelMask, EncodingError, DecodingError, InvalidFile
from . import FRAMELIST_SIZE
from .m4a import UnsupportedBitsPerSample

ERR_AU_INVALID_HEADER = u"invalid Sun AU header"
ERR_AU_UNSUPPORTED_FORMAT = u"unsupported Sun AU format"
ERR_AU_TRUNCATED_DATA = u"truncated data block"
ERR_AU_TOO_LARGE = u"PCM data too large for Sun AU file"
ERR_NEGATIVE_SEEK = u"cannot seek to negative value"

_ENCODING_BITS = {2: 8, 3: 16, 4: 24}
_BITS_ENCODING = {8: 2, 16: 3, 24: 4}


class InvalidAU(InvalidFile):
    """reference audiotools/au.py:25-26"""


def parse_header(header):
    """the 24 header bytes -> (data_offset, data_size, bits_per_sample,
    sample_rate, channels); IOError if short, ValueError with the
    reference's message on a bad magic number or encoding"""
    if len(header) < 24:
        raise IOError("I/O error reading Sun AU header")
    (magic, data_offset, data_size, encoding, sample_rate,
     channels) = struct.unpack(">4s5I", header[:24])
    if magic != b".snd":
        raise ValueError(ERR_AU_INVALID_HEADER)
    if encoding not in _ENCODING_BITS:
        raise ValueError(ERR_AU_UNSUPPORTED_FORMAT)
    return data_offset, data_size, _ENCODING_BITS[encoding], sample_rate, channels


def au_header(data_size, bits_per_sample, sample_rate, channels):
    """the 24-byte header from_pcm writes: the data follows it directly"""
    return struct.pack(">4s5I", b".snd", 24, data_size, _BITS_ENCODING[bits_per_sample],
                       sample_rate, channels)


class AuReader(object):
    """PCMReader over a Sun AU file's data (reference au.py:34-102)"""

    def __init__(self, au_filename):
        self.file = open(au_filename, "rb")
        try:
            (self.data_offset, data_size, self.bits_per_sample, self.sample_rate,
             self.channels) = parse_header(self.file.read(24))
        except Exception:
            self.file.close()
            raise
        self.channel_mask = {1: 0x4, 2: 0x3}.get(self.channels, 0)
        self.bytes_per_pcm_frame = (self.bits_per_sample // 8) * self.channels
        self.total_pcm_frames = data_size // self.bytes_per_pcm_frame
        self.remaining_pcm_frames = self.total_pcm_frames
        # the reference reads on from the end of the header and so takes an
        # annotation field for samples; the data begins at data_offset
        self.file.seek(self.data_offset, 0)

    def read(self, pcm_frames):
        """a FrameList of min(max(pcm_frames, 1), remaining) frames
        (au.py:61-81); IOError if the data ends early"""
        requested = min(max(pcm_frames, 1), self.remaining_pcm_frames)
        nbytes = self.bytes_per_pcm_frame * requested
        data = self.file.read(nbytes)
        if len(data) < nbytes:
            raise IOError(ERR_AU_TRUNCATED_DATA)
        self.remaining_pcm_frames -= requested
        return _pcm.FrameList(data, self.channels, self.bits_per_sample, True, True)

    def seek(self, pcm_frame_offset):
        """position at a PCM frame; returns the frames actually skipped
        (au.py:83-99)"""
        if pcm_frame_offset < 0:
            raise ValueError(ERR_NEGATIVE_SEEK)
        pcm_frame_offset = min(pcm_frame_offset, self.total_pcm_frames)
        self.file.seek(self.data_offset + pcm_frame_offset * self.bytes_per_pcm_frame, 0)
        self.remaining_pcm_frames = self.total_pcm_frames - pcm_frame_offset
        return pcm_frame_offset

    def close(self):
        self.file.close()


class AuAudio(AudioFile):
    """a Sun AU file (reference audiotools/au.py:105-285)"""

    SUFFIX = "au"
    NAME = SUFFIX
    DESCRIPTION = u"Sun Au"

    def __init__(self, filename):
        AudioFile.__init__(self, filename)
        try:
            with open(filename, "rb") as f:
                (self.__data_offset, self.__data_size, self.__bits_per_sample,
                 self.__sample_rate, self.__channels) = parse_header(f.read(24))
        except (IOError, ValueError) as err:
            raise InvalidAU(str(err))

    def lossless(self):
        return True

    def bits_per_sample(self):
        return self.__bits_per_sample

    def channels(self):
        return self.__channels

    def channel_mask(self):
        """front center for 1 channel, front left + right for 2, otherwise
        undefined"""
        if 1 <= self.__channels <= 2:
            return ChannelMask.from_channels(self.__channels)
        return ChannelMask(0)

    def sample_rate(self):
        return self.__sample_rate

    def total_frames(self):
        return self.__data_size // (self.__bits_per_sample // 8) // self.__channels

    def to_pcm(self):
        return AuReader(self.filename)

    def pcm_split(self):
        """(everything before the PCM data, everything after it): the header
        with its annotation field, and nothing (au.py:180-192)"""
        with open(self.filename, "rb") as f:
            magic, data_offset = struct.unpack(">4sI", f.read(8))
            return (struct.pack(">4sI", magic, data_offset) + f.read(data_offset - 8), b"")

    @classmethod
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None):
        """write pcmreader's data as a Sun AU file (au.py:195-266): a
        placeholder header, the big-endian samples, then the header again
        with the counted size; UnsupportedBitsPerSample for anything but 8,
        16 or 24 bits"""
        if pcmreader.bits_per_sample not in _BITS_ENCODING:
            raise UnsupportedBitsPerSample(filename, pcmreader.bits_per_sample)
        try:
            f = open(filename, "wb")
        except IOError as err:
            raise EncodingError(str(err))
        try:
            f.write(au_header(0, pcmreader.bits_per_sample, pcmreader.sample_rate,
                              pcmreader.channels))
            data_size = 0
            try:
                framelist = pcmreader.read(FRAMELIST_SIZE)
                while len(framelist) > 0:
                    data = framelist.to_bytes(True, True)
                    f.write(data)
                    data_size += len(data)
                    framelist = pcmreader.read(FRAMELIST_SIZE)
            except (IOError, ValueError) as err:
                cls.__unlink__(filename)
                raise EncodingError(str(err))
            except Exception:
                cls.__unlink__(filename)
                raise
            if data_size >= (1 << 32):
                cls.__unlink__(filename)
                raise EncodingError(ERR_AU_TOO_LARGE)
            f.seek(0, 0)
            f.write(au_header(data_size, pcmreader.bits_per_sample, pcmreader.sample_rate,
                              pcmreader.channels))
        finally:
            f.close()
        try:
            pcmreader.close()
        except DecodingError as err:
            cls.__unlink__(filename)
            raise EncodingError(err.error_message)
        return AuAudio(filename)
