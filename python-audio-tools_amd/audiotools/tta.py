"""audiotools.tta — True Audio files on the MI355X engine.

Mirrors the slice of the reference's audiotools/tta.py that the transcode
path uses:

  TrueAudio(filename)                                   tta.py:46-80
    - an ID3v2 comment in front of "TTA1" is stepped over
    - header fields and seektable are read, their CRCs are not looked at
      (the decoder checks them): InvalidTTA for a wrong signature, a format
      other than 1, or a file too short
  .bits_per_sample() .channels() .channel_mask() .lossless()
  .total_frames() .sample_rate() .data_size()           tta.py:82-117, 256-262
  .to_pcm() -> audiotools.decoders.TTADecoder (GPU), or a PCMReaderError
    when the decoder refuses the stream                 tta.py:119-141
  TrueAudio.from_pcm(filename, pcmreader, compression=None,
                     total_pcm_frames=None)             tta.py:143-254
    - with total_pcm_frames: header, a zero seektable, the frames, then the
      seektable rewritten at offset 0x16
    - without: frames to a temporary file, then header, seektable, frames
  convert / verify are AudioFile's.

Tags (ID3 / APEv2), cuesheets, ReplayGain tags and clean() are out of scope.
The container is host byte work; the frames are encoded and decoded by
libatgpu (tta_encode.hip / tta_decode.hip).
"""

import struct
import zlib

from . import (AudioFile, BufferedPCMReader, ChannelMask, CounterPCMReader, EncodingError,
               InvalidFile, PCMReaderError, transfer_data)


def div_ceil(n, d):
    return n // d + (1 if n % d else 0)


def tta_frame_count(total_pcm_frames, sample_rate):
    """frames the encoder writes and the decoder reads: blocks of
    sample_rate * 256 // 245 (src/encoders/tta.c:495-497).  The reference's
    Python divides by the unrounded 256 / 245 instead (tta.py:74-76), which
    is one frame short for some long streams; the codec's count is used."""
    block = (sample_rate * 256) // 245
    return div_ceil(total_pcm_frames, block) if total_pcm_frames else 0


class InvalidTTA(InvalidFile):
    """reference audiotools/tta.py:35-36"""


def _crc(data):
    return struct.pack("<I", zlib.crc32(data) & 0xFFFFFFFF)


def tta_header(channels, bits_per_sample, sample_rate, total_pcm_frames):
    """write_header (tta.py): 18 bytes + their CRC-32"""
    h = b"TTA1" + struct.pack("<HHHII", 1, channels, bits_per_sample, sample_rate,
                              total_pcm_frames)
    return h + _crc(h)


def tta_seektable(frame_sizes):
    """write_seektable (tta.py): one u32 per frame + their CRC-32"""
    t = b"".join(struct.pack("<I", s) for s in frame_sizes)
    return t + _crc(t)


class TrueAudio(AudioFile):
    """the reference's TrueAudio (tta.py:39-262), transcode slice"""

    SUFFIX = "tta"
    NAME = SUFFIX
    DESCRIPTION = u"True Audio"
    BINARIES = ()

    def __init__(self, filename):
        from .id3 import skip_id3v2_comment
        AudioFile.__init__(self, filename)
        try:
            with open(filename, "rb") as f:
                self.__stream_offset__ = skip_id3v2_comment(f)
                head = f.read(22)
                if len(head) < 22:
                    raise IOError("I/O error reading stream")
                (signature, format_, self.__channels__, self.__bits_per_sample__,
                 self.__sample_rate__, self.__total_pcm_frames__) = struct.unpack(
                    "<4sHHHII", head[:18])
                if signature != b"TTA1":
                    raise InvalidTTA("invalid signature")
                if format_ != 1:
                    raise InvalidTTA("unsupported format")
                if self.__sample_rate__ * 256 < 245 and self.__total_pcm_frames__:
                    raise InvalidTTA("unsupported format")
                self.__total_tta_frames__ = tta_frame_count(self.__total_pcm_frames__,
                                                            self.__sample_rate__)
                table = f.read(4 * self.__total_tta_frames__ + 4)
                if len(table) < 4 * self.__total_tta_frames__ + 4:
                    raise IOError("I/O error reading stream")
                self.__frame_lengths__ = list(struct.unpack(
                    "<%dI" % self.__total_tta_frames__, table[:-4]))
        except IOError as msg:
            raise InvalidTTA(str(msg))

    def bits_per_sample(self):
        return self.__bits_per_sample__

    def channels(self):
        return self.__channels__

    def channel_mask(self):
        return ChannelMask({1: 0x4, 2: 0x3}.get(self.__channels__, 0))

    def lossless(self):
        return True

    def total_frames(self):
        return self.__total_pcm_frames__

    def sample_rate(self):
        return self.__sample_rate__

    def data_size(self):
        """header + seektable + frames, from the header and the seektable"""
        return 22 + len(self.__frame_lengths__) * 4 + 4 + sum(self.__frame_lengths__)

    def to_pcm(self):
        from . import decoders
        try:
            with open(self.filename, "rb") as tta:
                if self.__stream_offset__ > 0:
                    tta.seek(self.__stream_offset__)
                return decoders.TTADecoder(tta)
        except (IOError, ValueError) as msg:
            return PCMReaderError(error_message=str(msg), sample_rate=self.sample_rate(),
                                  channels=self.channels(),
                                  channel_mask=int(self.channel_mask()),
                                  bits_per_sample=self.bits_per_sample())

    @classmethod
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None,
                 encoding_function=None):
        """encode pcmreader to a new True Audio file (tta.py:143-254); the
        frames come from encode_tta on the GPU, header and seektable from
        here"""
        import tempfile
        from .encoders import encode_tta
        encode = encode_tta if encoding_function is None else encoding_function
        try:
            file = open(filename, "wb")
        except IOError as err:
            raise EncodingError(str(err))
        counter = CounterPCMReader(pcmreader)
        rate = pcmreader.sample_rate
        if total_pcm_frames is not None:
            file.write(tta_header(pcmreader.channels, pcmreader.bits_per_sample, rate,
                                  total_pcm_frames))
            total_tta_frames = tta_frame_count(total_pcm_frames, rate)
            file.write(tta_seektable([0] * total_tta_frames))
            try:
                frame_sizes = encode(file, BufferedPCMReader(counter))
            except (IOError, ValueError) as err:
                file.close()
                cls.__unlink__(filename)
                raise EncodingError(str(err))
            if counter.frames_written != total_pcm_frames:
                file.close()
                cls.__unlink__(filename)
                raise EncodingError("total PCM frames mismatch")
            file.seek(0x16, 0)
            file.write(tta_seektable(frame_sizes))
        else:
            frames = tempfile.TemporaryFile()
            try:
                frame_sizes = encode(frames, BufferedPCMReader(counter))
            except (IOError, ValueError) as err:
                frames.close()
                file.close()
                cls.__unlink__(filename)
                raise EncodingError(str(err))
            file.write(tta_header(pcmreader.channels, pcmreader.bits_per_sample, rate,
                                  counter.frames_written))
            file.write(tta_seektable(frame_sizes))
            frames.seek(0, 0)
            transfer_data(frames.read, file.write)
            frames.close()
        file.close()
        return cls(filename)
