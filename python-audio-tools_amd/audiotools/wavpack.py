"""audiotools.wavpack — WavPack files on the MI355X engine.

Mirrors the slice of the reference's audiotools/wavpack.py that the transcode
path uses:

  WavPackAudio(filename)
    - the first block header gives sample rate, bits per sample, channels
      and total PCM frames; the sample-rate and channel-info sub-blocks of
      the first block where the header does not say (InvalidWavPack for a
      file the decoder would not open)
  .bits_per_sample() .channels() .channel_mask() .lossless()
  .total_frames() .sample_rate()
  .to_pcm() -> audiotools.decoders.WavPackDecoder (GPU), or a PCMReaderError
    when the decoder refuses the stream
  WavPackAudio.from_pcm(filename, pcmreader, compression, total_pcm_frames,
    encoding_function=audiotools.encoders.encode_wavpack) encodes on the GPU
    with the reference's five compression modes; with encoding_function left
    at None it still raises EncodingError (see from_pcm)
  convert / verify are AudioFile's.

Lossless integer streams only.  APEv2 tags, cuesheets and foreign RIFF
chunks (from_wave) are out of scope; the decoder steps over the RIFF header /
footer sub-blocks, the encoder writes the header the reference generates.
"""

from . import (AudioFile, BufferedPCMReader, ChannelMask, CounterPCMReader, EncodingError,
               InvalidFile, PCMReaderError)


class InvalidWavPack(InvalidFile):
    """reference audiotools/wavpack.py InvalidWavPack"""


class WavPackAudio(AudioFile):
    """the reference's WavPackAudio, transcode slice"""

    SUFFIX = "wv"
    NAME = SUFFIX
    DESCRIPTION = u"WavPack"
    DEFAULT_COMPRESSION = "standard"
    COMPRESSION_MODES = ("veryfast", "fast", "standard", "high", "veryhigh")
    COMPRESSION_DESCRIPTIONS = {"veryfast": u"fastest encode/decode, worst compression",
                                "veryhigh": u"slowest encode/decode, best compression"}
    BINARIES = ()
    __options__ = {mode: {"block_size": 44100, "joint_stereo": True, "false_stereo": True,
                          "wasted_bits": True, "correlation_passes": passes}
                   for mode, passes in zip(COMPRESSION_MODES, (1, 2, 5, 10, 16))}

    def __init__(self, filename):
        from . import _atgpu
        from .decoders import _wv_error
        AudioFile.__init__(self, filename)
        try:
            with open(filename, "rb") as f:
                data = f.read()
        except IOError as msg:
            raise InvalidWavPack(str(msg))
        st, info, _ = _atgpu.wv_read_info(data)
        if st:
            raise InvalidWavPack(str(_wv_error(st)))
        self.__sample_rate__ = info.sample_rate
        self.__bits_per_sample__ = info.bits_per_sample
        self.__channels__ = info.channels
        self.__channel_mask__ = info.channel_mask
        self.__total_pcm_frames__ = info.total_pcm_frames

    def bits_per_sample(self):
        return self.__bits_per_sample__

    def channels(self):
        return self.__channels__

    def channel_mask(self):
        return ChannelMask(self.__channel_mask__)

    def lossless(self):
        return True

    def total_frames(self):
        return self.__total_pcm_frames__

    def sample_rate(self):
        return self.__sample_rate__

    def to_pcm(self):
        from . import decoders
        try:
            with open(self.filename, "rb") as wv:
                return decoders.WavPackDecoder(wv)
        except (IOError, ValueError) as msg:
            return PCMReaderError(error_message=str(msg), sample_rate=self.sample_rate(),
                                  channels=self.channels(),
                                  channel_mask=int(self.channel_mask()),
                                  bits_per_sample=self.bits_per_sample())

    @classmethod
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None,
                 encoding_function=None):
        """encode pcmreader to a new WavPack file with encoding_function
        (audiotools.encoders.encode_wavpack), as the reference's from_pcm
        does (wavpack.py:443-490): an unknown compression is "standard", the
        frames are counted, ValueError / IOError and a total_pcm_frames
        mismatch unlink the file and raise EncodingError.

        With encoding_function left at None it raises EncodingError and
        creates no file, as before the engine had an encoder: making
        encode_wavpack the default is a one-line change here, together with
        the test that pins this behaviour, so convert(..., WavPackAudio)
        stays refused until then."""
        if encoding_function is None:
            raise EncodingError("WavPack encoding is not available")
        if compression is None or compression not in cls.COMPRESSION_MODES:
            compression = cls.DEFAULT_COMPRESSION
        counter = CounterPCMReader(pcmreader)
        try:
            encoding_function(filename, BufferedPCMReader(counter),
                              total_pcm_frames=(total_pcm_frames
                                                if total_pcm_frames is not None else 0),
                              **cls.__options__[compression])
        except (ValueError, IOError) as err:
            cls.__unlink__(filename)
            raise EncodingError(str(err))
        except Exception:
            cls.__unlink__(filename)
            raise
        if total_pcm_frames is not None and counter.frames_written != total_pcm_frames:
            cls.__unlink__(filename)
            raise EncodingError("total PCM frames mismatch")
        return cls(filename)
