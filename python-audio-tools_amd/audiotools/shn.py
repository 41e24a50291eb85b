"""audiotools.shn — Shorten files on the MI355X engine.

Mirrors the slice of the reference's audiotools/shn.py that the transcode
path uses:

  ShortenAudio(filename)                                   shn.py:37-161
    - magic "ajkg", version 2, the six header fields; the sample rate, the
      channel mask and the total PCM frames from a RIFF/WAVE or AIFF header
      in the first VERBATIM command (44100 Hz and a mask by channel count
      otherwise): InvalidShorten for a wrong header or an unsupported file
      type
  .bits_per_sample() .channels() .channel_mask() .lossless()
  .total_frames() .sample_rate()                            shn.py:163-191
  .to_pcm() -> audiotools.decoders.SHNDecoder (GPU), or a PCMReaderError
    when the decoder refuses the stream                     shn.py:193-209
  ShortenAudio.from_pcm(filename, pcmreader, compression=None,
                        total_pcm_frames=None, block_size=256)
    - with total_pcm_frames: from_wave with a generated wave header
    - without: through a temporary wave file                shn.py:211-272
  ShortenAudio.from_wave(filename, header, pcmreader, footer, ...)
                                                            shn.py:340-422
  .wave_header_footer() .has_foreign_wave_chunks()          shn.py:274-338
  convert / verify are AudioFile's.

There is no aiff.py in this package, so from_aiff, aiff_header_footer and
has_foreign_aiff_chunks are out of scope, as are tags and seek tables (a
Shorten file has neither).  The container is host byte work; the audio
commands are encoded and decoded by libatgpu (shn_encode.hip /
shn_decode.hip).
"""

import os
import struct

from . import (AudioFile, BufferedPCMReader, ChannelMask, CounterPCMReader, EncodingError,
               InvalidFile, PCMReaderError)
from .m4a import UnsupportedBitsPerSample


class InvalidShorten(InvalidFile):
    """reference audiotools/shn.py:26-27"""


def wave_parts(sample_rate, channels, channel_mask, bits_per_sample, total_pcm_frames):
    """the wave header from_pcm generates for a stream of known length and
    the pad byte behind an odd amount of data: the bytes of the two VERBATIM
    commands (shn.py:211-240)"""
    from .wav import wave_header
    data_bytes = (bits_per_sample // 8) * channels * total_pcm_frames
    return (wave_header(sample_rate, channels, channel_mask, bits_per_sample, total_pcm_frames),
            b"\x00" * (data_bytes % 2))


class ShortenAudio(AudioFile):
    """the reference's ShortenAudio (shn.py:30-610), transcode slice"""

    SUFFIX = "shn"
    NAME = SUFFIX
    DESCRIPTION = u"Shorten"
    BINARIES = ()

    def __init__(self, filename):
        from . import _atgpu
        AudioFile.__init__(self, filename)
        try:
            with open(filename, "rb") as f:
                data = f.read()
        except IOError as msg:
            raise InvalidShorten(str(msg))
        st, info = _atgpu.shn_read_info(data)
        if st == _atgpu.SHN_UNSUPPORTED_FILE_TYPE:
            raise InvalidShorten("unsupported Shorten file type")
        if st in (_atgpu.SHN_INVALID_MAGIC_NUMBER, _atgpu.SHN_INVALID_SHORTEN_VERSION) or \
                (st and len(data) < 5):
            raise InvalidShorten("invalid Shorten header")
        if st:
            raise InvalidShorten(str(_atgpu.SHN_HEADER_ERRORS[st][1]))
        self.__channels__ = info.channels
        self.__bits_per_sample__ = info.bits_per_sample
        self.__sample_rate__ = info.sample_rate
        # the decoder's mask is 0 without a wave or aiff header; the file
        # object then goes by the channel count (shn.py:82-88)
        mask = info.channel_mask or {1: 0x4, 2: 0x3}.get(info.channels, 0)
        self.__channel_mask__ = ChannelMask(mask)
        self.__total_frames__ = info.total_pcm_frames

    def bits_per_sample(self):
        return self.__bits_per_sample__

    def channels(self):
        return self.__channels__

    def channel_mask(self):
        return self.__channel_mask__

    def lossless(self):
        return True

    def total_frames(self):
        return self.__total_frames__

    def sample_rate(self):
        return self.__sample_rate__

    def to_pcm(self):
        from . import decoders
        try:
            with open(self.filename, "rb") as shn:
                return decoders.SHNDecoder(shn)
        except (IOError, ValueError) as msg:
            # the reference's fixed stand-in values (shn.py:201-209)
            return PCMReaderError(error_message=str(msg), sample_rate=44100, channels=2,
                                  channel_mask=0x3, bits_per_sample=16)

    @classmethod
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None,
                 block_size=256, encoding_function=None):
        """encode pcmreader to a new Shorten file (shn.py:211-272).  A
        Shorten file carries its wave header in front of the audio and every
        value in it is variable-sized, so the length has to be known first:
        either from total_pcm_frames, or by way of a temporary wave file."""
        from .wav import WaveAudio, wave_header
        if pcmreader.bits_per_sample not in (8, 16):
            raise UnsupportedBitsPerSample(filename, pcmreader.bits_per_sample)
        if total_pcm_frames is not None:
            header, footer = wave_parts(pcmreader.sample_rate, pcmreader.channels,
                                        pcmreader.channel_mask, pcmreader.bits_per_sample,
                                        total_pcm_frames)
            return cls.from_wave(filename, header, pcmreader, footer, compression, block_size,
                                 encoding_function)
        import tempfile
        f = tempfile.NamedTemporaryFile(suffix=".wav")
        try:
            w = WaveAudio.from_pcm(f.name, pcmreader)
            header, footer = w.wave_header_footer()
            return cls.from_wave(filename, header, w.to_pcm(), footer, compression, block_size,
                                 encoding_function)
        finally:
            if os.path.isfile(f.name):
                f.close()
            else:
                f.close_called = True

    def has_foreign_wave_chunks(self):
        """True if the VERBATIM commands hold RIFF chunks other than fmt and
        data (shn.py:274-316)"""
        from . import decoders
        try:
            with open(self.filename, "rb") as shn:
                head, tail = decoders.SHNDecoder(shn).pcm_split()
        except (IOError, ValueError):
            return False
        if len(head) < 12 or head[0:4] != b"RIFF" or head[8:12] != b"WAVE":
            return False
        if len(tail) >= 8:
            return True
        pos, total_size = 12, len(head) - 12
        while total_size >= 8:
            if pos + 8 > len(head):
                return False
            chunk_id, chunk_size = struct.unpack("<4sI", head[pos:pos + 8])
            pos += 8
            total_size -= 8
            if chunk_id not in (b"fmt ", b"data"):
                return True
            chunk_size += chunk_size % 2
            if pos + chunk_size > len(head):
                return False
            pos += chunk_size
            total_size -= chunk_size
        return False

    def wave_header_footer(self):
        """(bytes before the PCM data, bytes after it) from the VERBATIM
        commands; ValueError if they are no wave header, IOError if the
        stream cannot be walked (shn.py:318-338)"""
        from . import decoders
        with open(self.filename, "rb") as shn:
            head, tail = decoders.SHNDecoder(shn).pcm_split()
        if len(head) < 12:
            raise IOError("I/O error reading wave header")
        if head[0:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("invalid wave header")
        return head, tail

    @classmethod
    def from_wave(cls, filename, header, pcmreader, footer, compression=None, block_size=256,
                  encoding_function=None):
        """encode a new Shorten file from wave data: header + PCM + footer
        restore the wave file (shn.py:340-422)"""
        from .wav import (ERR_WAV_INVALID_SIZE, ERR_WAV_TRUNCATED_DATA_CHUNK, validate_footer,
                          validate_header)
        if encoding_function is None:
            from .encoders import encode_shn
        else:
            encode_shn = encoding_function
        if pcmreader.bits_per_sample not in (8, 16):
            raise UnsupportedBitsPerSample(filename, pcmreader.bits_per_sample)
        try:
            total_size, data_size = validate_header(header)
        except ValueError as err:
            raise EncodingError(str(err))
        counter = CounterPCMReader(pcmreader)
        try:
            kw = dict(filename=filename, pcmreader=BufferedPCMReader(counter),
                      is_big_endian=False, signed_samples=pcmreader.bits_per_sample == 16,
                      header_data=header, block_size=block_size)
            if len(footer):
                kw["footer_data"] = footer
            encode_shn(**kw)
            data_bytes_written = counter.bytes_written()
            if data_size != data_bytes_written:
                raise EncodingError(ERR_WAV_TRUNCATED_DATA_CHUNK)
            try:
                validate_footer(footer, data_bytes_written)
            except ValueError as err:
                raise EncodingError(str(err))
            if len(header) + data_size + len(footer) != total_size:
                raise EncodingError(ERR_WAV_INVALID_SIZE)
            return cls(filename)
        except EncodingError:
            cls.__unlink__(filename)
            raise
        except (IOError, ValueError) as err:
            cls.__unlink__(filename)
            raise EncodingError(str(err))
        except Exception:
            cls.__unlink__(filename)
            raise
