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
  WavPackAudio.from_pcm(...) raises EncodingError: the engine has no WavPack
    encoder yet
  convert / verify are AudioFile's.

Lossless integer streams only.  APEv2 tags, cuesheets and the RIFF header /
footer sub-blocks are out of scope; the decoder steps over them.
"""

from . import AudioFile, ChannelMask, EncodingError, InvalidFile, PCMReaderError


class InvalidWavPack(InvalidFile):
    """reference audiotools/wavpack.py InvalidWavPack"""


class WavPackAudio(AudioFile):
    """the reference's WavPackAudio, decode slice"""

    SUFFIX = "wv"
    NAME = SUFFIX
    DESCRIPTION = u"WavPack"
    BINARIES = ()

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
    def from_pcm(cls, filename, pcmreader, compression=None, total_pcm_frames=None):
        raise EncodingError("WavPack encoding is not available")
