"""audiotools.pcmfiles — what the batch entry points share about the three
uncompressed containers (RIFF WAVE, AIFF, Sun AU): telling a file image's
kind by its magic, reading its header on the host, and laying a batch of
data chunks out for the device's byte-layout kernels (csrc/pcm_bytes.hip).

Used by decoders.decode_pcm_batch and encoders.encode_aiff_batch /
encode_au_batch / encode_flac_files_batch.  The single-file readers
(wav.WaveReader, aiff.AiffReader, au.AuReader) do not come through here.
"""

import io
from collections import namedtuple

import numpy as np

from . import _atgpu

# data_offset / data_bytes: the sample bytes present in the image; frames: the
# whole PCM frames among them, at most the header's total_pcm_frames
PcmImage = namedtuple("PcmImage", "kind channels bits_per_sample sample_rate channel_mask "
                      "total_pcm_frames data_offset data_bytes frames big_endian is_signed")

TRUNCATED = {"wav": u"premature end of data chunk", "aiff": u"premature end of SSND chunk",
             "au": u"truncated data block"}


def _finish(kind, channels, bits, rate, mask, total, offset, avail, big_endian, is_signed):
    per_frame = channels * (bits // 8)
    if bits not in (8, 16, 24) or per_frame == 0:
        raise ValueError("unsupported bits per sample or channel count")
    frames = min(total, max(0, avail) // per_frame)
    return PcmImage(kind, channels, bits, rate, mask, total, offset, frames * per_frame, frames,
                    big_endian, is_signed)


def image_info(image):
    """PcmImage of a WAV, AIFF or AU file image (bytes), told apart by its
    magic; the header errors of the single-file readers raise as theirs do"""
    image = bytes(image)
    if image[:4] == b"FORM":
        st, i = _atgpu.aiff_read_info(image)
        if st == _atgpu.ATG_ERR_UNSUPPORTED:
            raise ValueError("unsupported bits per sample or sample rate")
        if st == _atgpu.AIFF_IOERROR:
            raise IOError(_atgpu.AIFF_ERRORS[st])
        if st != _atgpu.AIFF_OK:
            raise ValueError(_atgpu.AIFF_ERRORS.get(st, "invalid AIFF file"))
        # the reader takes total_pcm_frames from COMM and reads on from the
        # sound data's first byte, whatever size SSND declares
        return _finish("aiff", i.channels, i.bits_per_sample, i.sample_rate, i.channel_mask,
                       i.total_pcm_frames, i.ssnd_data_offset, len(image) - i.ssnd_data_offset,
                       True, True)
    if image[:4] == b".snd":
        st, i = _atgpu.au_read_info(image)
        if st == _atgpu.AU_IOERROR:
            raise IOError(_atgpu.AU_ERRORS[st])
        if st != _atgpu.AU_OK:
            raise ValueError(_atgpu.AU_ERRORS.get(st, "unsupported Sun AU header"))
        return _finish("au", i.channels, i.bits_per_sample, i.sample_rate, i.channel_mask,
                       i.total_pcm_frames, i.data_offset, len(image) - i.data_offset, True, True)
    if image[:4] == b"RIFF":
        # wav.py's own parser, over the image
        from .wav import WaveReader
        r = WaveReader.__new__(WaveReader)
        r.file = io.BytesIO(image)
        r._open()
        return _finish("wav", r.channels, r.bits_per_sample, r.sample_rate, r.channel_mask,
                       r.total_pcm_frames, r.data_chunk_offset, len(image) - r.data_chunk_offset,
                       False, r.bits_per_sample != 8)
    raise ValueError("not a RIFF WAVE, AIFF or Sun AU file")


def layout_of(info):
    return _atgpu.pcm_layout(info.bits_per_sample // 8, info.big_endian, info.is_signed)


def plan(infos, group):
    """lay the images' data chunks back to back on the packed side and their
    samples in slots on a multiple of `group` samples.
    -> (runs [(byte_offset, samples, sample_offset)], packed bytes rounded up
    to 16, samples)"""
    runs, pos, slot = [], 0, 0
    for i in infos:
        n = i.frames * i.channels
        runs.append((pos, n, slot))
        pos += i.data_bytes
        slot += (n + group - 1) // group * group
    return runs, (pos + 15) // 16 * 16, slot


def gather(images, infos, cap):
    """the data chunks as one uint8 array of cap bytes"""
    buf = np.zeros(max(cap, 16), dtype=np.uint8)
    pos = 0
    for img, i in zip(images, infos):
        if i.data_bytes:
            buf[pos:pos + i.data_bytes] = np.frombuffer(img, dtype=np.uint8, count=i.data_bytes,
                                                        offset=i.data_offset)
        pos += i.data_bytes
    return buf


def unpack_groups(infos, runs, d_bytes, cap, d_pcm, fmt, n_samples):
    """one unpack launch per layout among the images"""
    groups = {}
    for i, r in zip(infos, runs):
        groups.setdefault((i.bits_per_sample // 8, i.big_endian, i.is_signed), []).append(r)
    for (b, be, sg), rs in sorted(groups.items()):
        _atgpu.pcm_unpack_device(d_bytes, cap, _atgpu.pcm_layout(b, be, sg), rs, d_pcm, fmt,
                                 n_samples)
