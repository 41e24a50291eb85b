"""audiotools._accuraterip — AccurateRip track checksums on the MI355X.

`ChecksumV1` and `ChecksumV2` keep the Python contract of the reference's C
types (src/accuraterip.c:64-326): Checksum(is_first, is_last, sample_rate,
total_pcm_frames), update(framelist), checksum().  update() buffers the
frames and sums them on the GPU (accuraterip.hip) a piece at a time; each
piece carries the running frame index, and the sums add modulo 2^32, so the
value does not depend on how the frames were split into FrameLists.  There
is no CPU path.
"""

import numpy as np

from . import _atgpu
from . import pcm

# frames buffered before a piece is summed on the GPU
FLUSH_FRAMES = 1 << 20


class _Checksum(object):
    _field = None  # the ArResult field this class reports

    def __init__(self, is_first, is_last, sample_rate, total_pcm_frames):
        for v in (is_first, is_last, sample_rate, total_pcm_frames):
            if isinstance(v, float) or not hasattr(v, "__index__"):
                raise TypeError("an integer is required")
        if sample_rate <= 0:
            raise ValueError("sample rate must be > 0")
        if total_pcm_frames <= 0:
            raise ValueError("total PCM frames must be > 0")
        self._first = bool(is_first)
        self._last = bool(is_last)
        self._rate = int(sample_rate)
        self._total = int(total_pcm_frames)
        self._index0 = 0  # frames summed so far
        self._sum = 0
        self._buf = np.empty(2 * FLUSH_FRAMES, dtype=np.int16)
        self._fill = 0    # samples in _buf

    def update(self, framelist):
        if not isinstance(framelist, pcm.FrameList):
            raise TypeError("objects must be of type FrameList")
        if framelist.channels != 2:
            raise ValueError("FrameList must be 2 channels")
        if framelist.bits_per_sample != 16:
            raise ValueError("FrameList must be 16 bits per sample")
        s = framelist.samples
        pos = 0
        while pos < len(s):
            n = min(len(s) - pos, len(self._buf) - self._fill)
            self._buf[self._fill:self._fill + n] = s[pos:pos + n]
            self._fill += n
            pos += n
            if self._fill == len(self._buf):
                self._flush()

    def _flush(self):
        frames = self._fill // 2
        if not frames:
            return
        track = _atgpu.ar_track(0, frames, self._rate, self._first, self._last,
                                index0=self._index0, total_pcm_frames=self._total)
        (res,), _ = _atgpu.accuraterip_host(self._buf[:self._fill], _atgpu.PCM_S16, [track])
        self._sum = (self._sum + getattr(res, self._field)) & 0xFFFFFFFF
        self._index0 += frames
        self._fill = 0

    def checksum(self):
        self._flush()
        return self._sum


class ChecksumV1(_Checksum):
    """sum of value * index modulo 2^32 (accuraterip.c:129-185)"""
    _field = "v1"


class ChecksumV2(_Checksum):
    """sum of the low and high words of the 64-bit products, modulo 2^32
    (accuraterip.c:263-326)"""
    _field = "v2"
