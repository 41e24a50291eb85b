"""audiotools.batchfiles — the files of one batch call, opened and decoded
for the device.  Shared by trackcmp's comparisons and convert_files_batch.

A file is a filename or a bytes image of any supported format (FLAC, Ogg
FLAC, ALAC, True Audio, WavPack, Shorten, WAV, AIFF, Sun AU), told apart by
magic.  _open gives what a caller needs of a file before any decode; _Batch
reads and opens every distinct file once and decodes those a caller wants,
all images of one format in one call of that format's decoder, the PCM left
in device memory as interleaved int32.  Everything runs on the default
device.
"""

import io
import sys
from collections import namedtuple

import numpy as np

from . import _atgpu
from . import pcmfiles
from .id3 import skip_id3v2_comment


# ------------------------------------------------------- opening the files
# what the comparison needs of a file before any decode; `info` is the
# format's own header struct, `image` the bytes its decoder takes
_Header = namedtuple("_Header", "kind sample_rate channels bits_per_sample channel_mask "
                     "total_frames info image")

_SIMPLE_MASKS = {1: 0x4, 2: 0x3}


def _open(image):
    """_Header of a file image, or None where the file's reader would refuse
    it (cmp_files then gives -2)"""
    try:
        f = io.BytesIO(image)
        skip = skip_id3v2_comment(f)
        magic = image[skip:skip + 4]
        if magic == b"fLaC":
            image = image[skip:]
            rc, si, _ = _atgpu.read_metadata(image)
            if rc:
                return None
            mask = _SIMPLE_MASKS.get(si.channels, si.channel_mask)
            return _Header("flac", si.sample_rate, si.channels, si.bits_per_sample, mask,
                           si.total_samples, si, image)
        if magic == b"TTA1":
            st, info, sizes = _atgpu.tta_read_info(image)
            if st:
                return None
            return _Header("tta", info.sample_rate, info.channels, info.bits_per_sample,
                           _SIMPLE_MASKS.get(info.channels, 0), info.total_pcm_frames,
                           (info, sizes), image)
        magic = image[:4]
        if magic == b"OggS":
            rc, info = _atgpu.oggflac_read_info(image)
            if rc:
                return None
            si = info.si
            return _Header("oggflac", si.sample_rate, si.channels, si.bits_per_sample,
                           _SIMPLE_MASKS.get(si.channels, si.channel_mask), si.total_samples,
                           info, image)
        if image[4:8] == b"ftyp":
            from .decoders import ALAC_CHANNEL_MASKS
            st, info, _, sizes = _atgpu.alac_read_info(image)
            if st:
                return None
            return _Header("alac", info.sample_rate, info.channels, info.bits_per_sample,
                           ALAC_CHANNEL_MASKS.get(info.channels, 0), info.total_frames,
                           (info, sizes), image)
        if magic == b"wvpk":
            st, info, blocks = _atgpu.wv_read_info(image)
            if st:
                return None
            return _Header("wavpack", info.sample_rate, info.channels, info.bits_per_sample,
                           info.channel_mask, info.total_pcm_frames, (info, blocks), image)
        if magic == b"ajkg":
            st, info = _atgpu.shn_read_info(image)
            if st:
                return None
            return _Header("shn", info.sample_rate, info.channels, info.bits_per_sample,
                           info.channel_mask, info.total_pcm_frames, info, image)
        if magic in (b"RIFF", b"FORM", b".snd"):
            i = pcmfiles.image_info(image)
            return _Header("pcm", i.sample_rate, i.channels, i.bits_per_sample, i.channel_mask,
                           i.total_pcm_frames, i, image)
    except (IOError, ValueError, IndexError, KeyError):
        return None
    return None


def _read(file):
    """a filename or a bytes image -> the image, or None if it cannot be read"""
    if isinstance(file, (bytes, bytearray, memoryview)):
        return bytes(file)
    try:
        with open(file, "rb") as f:
            return f.read()
    except (IOError, OSError):
        return None


# ------------------------------------------------------------ device decode
# Every helper decodes all images of its format in one call and leaves the
# PCM in device memory: -> (device pointer of int32 PCM, [_Pcm], device
# pointers to free after the comparison).
_Pcm = namedtuple("_Pcm", "ok sample_offset frames")


def _upload(images):
    """the images 4-byte aligned in one device buffer -> (pointer, bytes
    used, [offset])"""
    parts, offsets, pos = [], [], 0
    for img in images:
        offsets.append(pos)
        parts.append(img + b"\0" * ((-len(img)) % 4))
        pos += len(parts[-1])
    blob = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8)
    eng = _atgpu.engine()
    d = eng.device_alloc(len(blob))
    try:
        eng.copy_to_device(d, blob)
    except Exception:
        eng.device_free(d)
        raise
    return d, pos, offsets


def _decode_flac(headers):
    bodies = [h.image[h.info.frames_offset:] for h in headers]
    d, n, offs = _upload(bodies)
    tracks = [_atgpu.dec_track(o, len(b), h.info) for o, b, h in zip(offs, bodies, headers)]
    res, d_pcm, _ = _atgpu.decoder().decode_device(d, n, tracks)
    return d_pcm, [_Pcm(r.status == 0, r.pcm_offset * h.channels, r.pcm_frames)
                   for r, h in zip(res, headers)], [d]


def _decode_oggflac(headers):
    d, n, offs = _upload([h.image for h in headers])
    tracks = [_atgpu.oggflac_dec_track(o, len(h.image)) for o, h in zip(offs, headers)]
    res, d_pcm, _ = _atgpu.decoder().decode_oggflac_device(d, n, tracks)
    return d_pcm, [_Pcm(r.status == 0 and r.ogg_status == 0, r.sample_offset, r.pcm_frames)
                   for r in res], [d]


def _decode_alac(headers):
    d, n, offs = _upload([h.image for h in headers])
    tracks = [_atgpu.alac_dec_track(o, len(h.image), h.info[0], frameset_bytes=h.info[1])
              for o, h in zip(offs, headers)]
    res, d_pcm, _ = _atgpu.alac_decoder().decode_device(d, n, tracks)
    return d_pcm, [_Pcm(r.status == 0, r.sample_offset, r.pcm_frames) for r in res], [d]


def _decode_tta(headers):
    d, n, offs = _upload([h.image for h in headers])
    tracks = [_atgpu.tta_dec_track(o, len(h.image), h.info[0], h.info[1])
              for o, h in zip(offs, headers)]
    res, d_pcm, _ = _atgpu.tta_decoder().decode_device(d, n, tracks)
    return d_pcm, [_Pcm(r.status == 0, r.sample_offset, r.pcm_frames) for r in res], [d]


def _decode_wavpack(headers):
    d, n, offs = _upload([h.image for h in headers])
    tracks = [_atgpu.wv_dec_track(o, len(h.image), h.info[0], h.info[1], check_md5=2)
              for o, h in zip(offs, headers)]
    res, d_pcm, _ = _atgpu.wv_decoder().decode_device(d, n, tracks)
    return d_pcm, [_Pcm(r.status == 0, r.sample_offset, r.pcm_frames) for r in res], [d]


def _decode_shn(headers):
    d, n, offs = _upload([h.image for h in headers])
    tracks = [_atgpu.shn_dec_track(o, len(h.image), h.info) for o, h in zip(offs, headers)]
    res, d_pcm, _ = _atgpu.shn_decoder().decode_device(d, n, tracks)
    # a Shorten stream that ends with its QUIT command is a whole one
    return d_pcm, [_Pcm(r.status == _atgpu.SHN_END_OF_STREAM, r.pcm_offset, r.pcm_frames)
                   for r in res], [d]


def _decode_pcm(headers):
    """WAV, AIFF and AU: the data chunks go up as they lie in the files and
    one launch per sample layout unpacks them (pcm_bytes.hip)"""
    infos = [h.info for h in headers]
    runs, cap, n_samples = pcmfiles.plan(infos, 4)
    eng = _atgpu.engine()
    n_samples = max(n_samples, 4)
    d_bytes = eng.device_alloc(max(cap, 16))
    d_pcm = eng.device_alloc(4 * n_samples)
    try:
        eng.copy_to_device(d_bytes, pcmfiles.gather([h.image for h in headers], infos, cap))
        pcmfiles.unpack_groups(infos, runs, d_bytes, cap, d_pcm, _atgpu.PCM_S32, n_samples)
    except Exception:
        eng.device_free(d_bytes)
        eng.device_free(d_pcm)
        raise
    return d_pcm, [_Pcm(i.frames == i.total_pcm_frames, slot, i.frames)
                   for i, (_, _, slot) in zip(infos, runs)], [d_bytes, d_pcm]


# in this order; FLAC and Ogg FLAC share one decoder handle
_KINDS = ("flac", "oggflac", "alac", "tta", "wavpack", "shn", "pcm")


class _Batch(object):
    """the files of one call: read and opened once each, then those a
    comparison needs decoded, one decode per format"""

    def __init__(self, helpers=None):
        # the module whose _decode_<kind> functions decode (default: this one)
        self._helpers = sys.modules[__name__] if helpers is None else helpers
        self.headers = []   # _Header or None, per distinct file
        self._index = {}
        self.wanted = set()
        self.views = {}     # file index -> (d_pcm, _Pcm)
        self._free = []

    def add(self, file):
        """-> the file's index in the batch"""
        key = file if isinstance(file, str) else id(file)
        if key not in self._index:
            image = _read(file)
            self._index[key] = len(self.headers)
            self.headers.append(None if image is None else _open(image))
        return self._index[key]

    def want(self, i):
        self.wanted.add(i)

    def decode(self):
        eng = _atgpu.engine()
        for kind in _KINDS:
            idx = sorted(i for i in self.wanted if self.headers[i].kind == kind)
            if not idx:
                continue
            helper = getattr(self._helpers, "_decode_" + kind)
            d_pcm, pcms, free = helper([self.headers[i] for i in idx])
            self._free.extend(free)
            if kind == "flac" and any(self.headers[i].kind == "oggflac" for i in self.wanted):
                # the Ogg FLAC decode that follows runs on the same handle and
                # takes its output buffer: keep the FLAC PCM in a copy
                n = max([p.sample_offset + p.frames * self.headers[i].channels
                         for p, i in zip(pcms, idx)] + [1])
                keep = eng.device_alloc(4 * n)
                self._free.append(keep)
                eng.copy_device(keep, d_pcm, 4 * n)
                d_pcm = keep
            for i, p in zip(idx, pcms):
                self.views[i] = (d_pcm, p)

    def ok(self, i):
        return self.views[i][1].ok

    def frames(self, i):
        return self.views[i][1].frames

    def view(self, i, window_offset=0):
        d_pcm, p = self.views[i]
        return _atgpu.pcm_view(d_pcm, _atgpu.PCM_S32, p.frames, p.sample_offset, window_offset)

    def close(self):
        if not self._free:
            return
        eng = _atgpu.engine()
        for d in self._free:
            eng.device_free(d)
        self._free = []
