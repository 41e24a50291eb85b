"""audiotools.decoders — FLAC decoding on the MI355X.

`FlacDecoder` IS the compiled C-API type `audiotools._decoders_c.FlacDecoder`
(csrc/ext/decoders_c.c over libatgpu's C ABI), with the Python-visible
contract of the reference's C type audiotools.decoders.FlacDecoder
(src/decoders/flac.c, methods :145-166):

  FlacDecoder(file)        file object, filename or bytes positioned at
                           "fLaC"; ValueError / IOError from the metadata
                           reader (flacdec_read_metadata, flac.c:568-707)
  .sample_rate .bits_per_sample .channels .channel_mask
  .read(n)                 one FLAC frame per call as a pcm.FrameList; an
                           empty FrameList once the stream is done, after
                           the STREAMINFO MD5 check (flac.c:174-285, 479-493);
                           ValueError with the reference's message on a bad
                           frame, IOError "EOF reading frame" on truncation
  .seek(pcm_frame_offset)  last SEEKTABLE point at or before the offset
                           (flac.c:287-356)
  .offsets()               [(byte offset from the current position, block
                           size)] of the frames left, CRC-16 unchecked
                           (flac.c:365-443)
  .close()                 further reads raise ValueError

The stream is decoded by libatgpu (HIP kernels, flac_decode.hip) in bounded
segments as read() needs them (8 MiB of compressed data per GPU call, the
MD5 chained on the host); read() hands out the decoded frames in order and
raises the decode status at the frame where the reference would.
`decode_flac_batch` is the batch entry trackverify-style callers use.
`ALACDecoder` / `decode_alac_batch` do the same for ALAC in M4A
(reference src/decoders/alac.c; GPU kernels alac_decode.hip).
`TTADecoder` / `decode_tta_batch` do the same for True Audio (reference
src/decoders/tta.c; GPU kernels tta_decode.hip), `SHNDecoder` /
`decode_shn_batch` for Shorten (src/decoders/shn.c; shn_decode.hip),
`WavPackDecoder` /
`decode_wavpack_batch` for WavPack (reference src/decoders/wavpack.c; GPU
kernels wavpack_decode.hip), `OggFlacDecoder` / `decode_oggflac_batch` for
Ogg FLAC (src/ogg.c, src/decoders/oggflac.c; ogg_demux.hip and
flac_decode.hip).  `decode_pcm_batch` reads the uncompressed containers (RIFF
WAVE, AIFF, Sun AU) in a batch, their samples unpacked on the GPU
(pcm_bytes.hip).  `DVDA_Title` / `decode_dvda_batch` read DVD-Audio titles
(reference src/decoders/aob.c, aobpcm.c; GPU kernels aob_decode.hip).
There is no CPU decoding path.
"""

import hashlib

import numpy as np

from . import _atgpu
from . import pcm
# the drop-in decoder type: the compiled C-API FlacDecoder
# (csrc/ext/decoders_c.c over libatgpu), as the reference's is its C type
from ._decoders_c import FlacDecoder  # noqa: F401


def _metadata_error(rc):
    if rc == 1:
        return ValueError("not a FLAC file")
    return IOError("EOF while reading metadata")


def _file_bytes(file):
    """bytes as they are, a file object's from its position on"""
    if isinstance(file, (bytes, bytearray, memoryview)):
        return bytes(file)
    if hasattr(file, "read"):
        return file.read()
    raise TypeError("file must be a file object or bytes")


def _check_open(decoder, doing):
    if decoder._closed:
        raise ValueError("cannot %s closed stream" % doing)


def _seek_offset(decoder, pcm_frame_offset):
    """the offset of a seek() as an int, checked as every decoder checks it"""
    _check_open(decoder, "seek")
    pcm_frame_offset = int(pcm_frame_offset)
    if pcm_frame_offset < 0:
        raise ValueError("cannot seek to negative value")
    return pcm_frame_offset


def decode_flac_batch(images):
    """decode a list of .flac images (bytes) in one GPU batch.
    -> list of (status, streaminfo, int32 interleaved PCM); status is an
    ATG_FD_* code (0 = decoded and MD5-verified)."""
    infos, bodies = [], []
    for img in images:
        rc, si, _ = _atgpu.read_metadata(img)
        if rc:
            raise _metadata_error(rc)
        infos.append(si)
        bodies.append(bytes(img[si.frames_offset:]))
    # the streams sharded over the node's GPUs (_atgpu.batch_devices),
    # balanced by PCM frames
    devs = _atgpu.batch_devices()
    ranges = (_atgpu.shard_ranges([si.total_samples for si in infos], len(devs))
              if len(devs) > 1 else [(0, len(infos))])

    def shard(i):
        t0, t1 = ranges[i]
        data, spans = _atgpu.pack_images(bodies[t0:t1])
        tracks = [_atgpu.dec_track(offset, nbytes, si)
                  for (offset, nbytes), si in zip(spans, infos[t0:t1])]
        dec = (_atgpu.decoder() if len(ranges) == 1
               else _atgpu.shard_object("decoder", i, devs[i]))
        return dec.decode(data, tracks)

    out = []
    for (t0, t1), (pcm_i32, res, _, _) in zip(ranges, _atgpu.run_shards(shard, len(ranges))):
        for si, r in zip(infos[t0:t1], res):
            a = r.pcm_offset * si.channels
            out.append((r.status, si, pcm_i32[a:a + r.pcm_frames * si.channels]))
    return out


def flac_frame_index_batch(images):
    """the frame starts of a list of .flac images (bytes), found on the GPU
    in one call (flac_index.hip): a FLAC stream carries no per-frame table.
    -> per image [(byte offset from the first frame, first_sample,
    block_size)], ascending.  A start is listed when its header is sound,
    agrees with STREAMINFO, and the bytes up to a later header whose number
    follows (or up to the stream's end) pass CRC-16: starts are promised,
    lengths are not, and the samples themselves are not decoded."""
    infos, bodies = [], []
    for img in images:
        rc, si, _ = _atgpu.read_metadata(img)
        if rc:
            raise _metadata_error(rc)
        infos.append(si)
        bodies.append(bytes(img[si.frames_offset:]))
    data, spans = _atgpu.pack_images(bodies)
    ranges = [_atgpu.flac_index_range(offset, nbytes, si)
              for (offset, nbytes), si in zip(spans, infos)]
    out = [[] for _ in images]
    for r, offset, first_sample, block_size in _atgpu.flac_index_host(data, ranges):
        out[r].append((offset, first_sample, block_size))
    return out


def pcm_md5(samples, bits_per_sample):
    """MD5 of FrameList.to_bytes(False, True) for int32 samples (test aid)"""
    a = np.asarray(samples, dtype=np.int32)
    bb = (bits_per_sample + 7) // 8
    b = a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :bb]
    return hashlib.md5(b.tobytes()).digest()


# ------------------------------------------------------------------ ALAC
ALAC_CHANNEL_MASKS = {1: 0x0004, 2: 0x0003, 3: 0x0007, 4: 0x0107, 5: 0x0037, 6: 0x003F,
                      7: 0x013F, 8: 0x00FF}  # ALACDecoder_channel_mask (alac.c:157-180)


def _alac_init_error(status):
    msg = _atgpu.AD_INIT_MESSAGES.get(status, "no error")
    if status in (_atgpu.AD_IO_ERROR, _atgpu.AD_NO_MDAT):
        return IOError(msg)
    return ValueError(msg)


def _alac_read_error(status):
    msg = _atgpu.AD_READ_MESSAGES.get(status, "no error")
    return IOError(msg) if status == _atgpu.AD_IO_ERROR else ValueError(msg)


class ALACDecoder(object):
    """reference src/decoders/alac.c ALACDecoder(filename), decoded on the
    GPU (alac_decode.hip):

      .sample_rate .bits_per_sample .channels .channel_mask
      .read(n)       one ALAC frameset per call (wave channel order); an
                     empty FrameList once remaining_frames is 0 (:183-254)
      .seek(offset)  last seektable entry at or before offset (:256-301)
      .close()
    """

    def __init__(self, filename):
        with open(filename, "rb") as f:  # IOError with errno + filename
            data = f.read()
        self.filename = filename
        st, info, points, sizes = _atgpu.alac_read_info(data)
        if st:
            raise _alac_init_error(st)
        self._data = data
        self._info = info
        self._sizes = sizes
        # an empty seektable rewinds to the mdat start (alac.c:82-87)
        self._seektable = points if points else [(0, info.mdat_offset)]
        self.sample_rate = info.sample_rate
        self.bits_per_sample = info.bits_per_sample
        self.channels = info.channels
        self.channel_mask = ALAC_CHANNEL_MASKS.get(info.channels, 0)
        self.total_frames = info.total_frames
        self._pos = info.mdat_offset
        self._remaining = info.total_frames
        self._closed = False
        self._decoded = False

    def _hint(self):
        """the stsz sizes from the current position on (a decoding hint)"""
        if not len(self._sizes):
            return None
        starts = self._info.mdat_offset + np.concatenate(
            [[0], np.cumsum(self._sizes.astype(np.int64))])
        k = int(np.searchsorted(starts, self._pos))
        if k < len(self._sizes) and starts[k] == self._pos:
            return self._sizes[k:]
        return None

    def _decode(self):
        if self._decoded:
            return
        data, _ = _atgpu.pack_images([self._data])
        track = _atgpu.alac_dec_track(0, len(self._data), self._info, start=self._pos,
                                      remaining=self._remaining, frameset_bytes=self._hint())
        pcm_i32, res, ff, _ = _atgpu.alac_decoder().decode(data, [track])
        r = res[0]
        self._pcm = pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * self.channels]
        self._fs = [int(x) for x in ff[r.first_frameset:r.first_frameset + r.n_framesets]]
        self._starts = np.concatenate([[0], np.cumsum(self._fs, dtype=np.int64)])
        self._status = r.status
        self._next = 0
        self._decoded = True

    def read(self, pcm_frames):
        _check_open(self, "read")
        if self._remaining == 0:
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        self._decode()
        if self._next < len(self._fs):
            k = self._next
            self._next += 1
            n = self._fs[k]
            self._remaining -= min(self._remaining, n)
            a, b = int(self._starts[k]) * self.channels, int(self._starts[k + 1]) * self.channels
            return pcm.FrameList._wrap(self._pcm[a:b].copy(), self.channels,
                                       self.bits_per_sample)
        if self._status == _atgpu.AD_OK:  # remaining reached 0 with this walk
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        raise _alac_read_error(self._status)

    def seek(self, pcm_frame_offset):
        pcm_frame_offset = _seek_offset(self, pcm_frame_offset)
        best = None
        for entry in self._seektable:
            if entry[0] <= pcm_frame_offset:
                best = entry
            else:
                break
        if best is None:
            raise ValueError("no offset found in seektable")
        self._remaining = (self.total_frames - best[0]) % (1 << 32)
        self._pos = best[1]
        self._decoded = False
        return best[0]

    def close(self):
        self._closed = True


def decode_alac_batch(images):
    """decode a list of M4A/ALAC images (bytes) in one GPU batch
    -> list of (status, AlacInfo, int32 interleaved PCM); status is an
    ATG_AD_* code (0 = every frame up to total_frames decoded)"""
    images = list(images)
    data, spans = _atgpu.pack_images(images)
    tracks, infos = [], []
    for img, (offset, nbytes) in zip(images, spans):
        st, info, _, sizes = _atgpu.alac_read_info(img)
        if st:
            raise _alac_init_error(st)
        tracks.append(_atgpu.alac_dec_track(offset, nbytes, info, frameset_bytes=sizes))
        infos.append(info)
    pcm_i32, res, _, _ = _atgpu.alac_decoder().decode(data, tracks)
    out = []
    for info, r in zip(infos, res):
        out.append((r.status, info,
                    pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * info.channels]))
    return out


# ------------------------------------------------------------ True Audio
def _tta_init_error(status, stage):
    table = _atgpu.TD_HEADER_MESSAGES if stage == 0 else _atgpu.TD_SEEKTABLE_MESSAGES
    msg = table.get(status, "no error")
    return IOError(msg) if status == _atgpu.TD_IO_ERROR else ValueError(msg)


def _tta_read_error(status):
    msg = _atgpu.TD_READ_MESSAGES.get(status, "no error")
    return IOError(msg) if status == _atgpu.TD_IO_ERROR else ValueError(msg)


class TTADecoder(object):
    """reference src/decoders/tta.c TTADecoder(file), decoded on the GPU
    (tta_decode.hip):

      TTADecoder(file)   file object positioned at "TTA1" (or at an ID3v2
                         comment in front of it), or bytes; ValueError /
                         IOError from the header and seektable readers
                         (:79-122)
      .sample_rate .bits_per_sample .channels .channel_mask
      .read(n)           one TTA frame per call; an empty FrameList once
                         every PCM frame is out (:194-262)
      .seek(offset)      the frame boundary the reference's loop stops at
                         (:264-321)
      .close()
    """

    def __init__(self, file):
        data = _file_bytes(file)
        st, info, sizes = _atgpu.tta_read_info(data)
        if st:
            raise _tta_init_error(st, info.stage)
        self._data = data
        self._info = info
        self._sizes = sizes
        self.sample_rate = info.sample_rate
        self.bits_per_sample = info.bits_per_sample
        self.channels = info.channels
        self.channel_mask = {1: 0x4, 2: 0x3}.get(info.channels, 0)  # :181-192
        self.total_frames = info.total_pcm_frames
        self.block_size = info.block_size
        self._frame = 0          # current_tta_frame
        self._remaining = info.total_pcm_frames
        self._closed = False
        self._decoded_from = None

    def _decode(self):
        """the frames from the current one on, in one GPU call"""
        if self._decoded_from is not None and self._decoded_from <= self._frame:
            return
        data, _ = _atgpu.pack_images([self._data])
        track = _atgpu.tta_dec_track(0, len(self._data), self._info, self._sizes, self._frame)
        pcm_i32, res = _atgpu.tta_decoder().decode(data, [track])
        r = res[0]
        self._pcm = pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * self.channels]
        self._good = r.n_frames
        self._status = r.status
        self._decoded_from = self._frame

    def read(self, pcm_frames):
        _check_open(self, "read")
        if self._remaining == 0:
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        self._decode()
        k = self._frame - self._decoded_from
        if k >= self._good:
            raise _tta_read_error(self._status)
        n = min(self._remaining, self.block_size)
        a = k * self.block_size * self.channels
        self._frame += 1
        self._remaining -= n
        return pcm.FrameList._wrap(self._pcm[a:a + n * self.channels].copy(), self.channels,
                                   self.bits_per_sample)

    def seek(self, pcm_frame_offset):
        pcm_frame_offset = _seek_offset(self, pcm_frame_offset)
        # skip whole frames while the next boundary is still short of the
        # offset (the reference compares with <, so an offset on a boundary
        # stops one frame early)
        current, frame, remaining = 0, 0, self.total_frames
        while current + self.block_size < pcm_frame_offset:
            n = min(remaining, self.block_size)
            if n == 0:
                break
            current += n
            frame += 1
            remaining -= n
        self._frame = frame
        self._remaining = remaining
        if self._decoded_from is not None and frame < self._decoded_from:
            self._decoded_from = None
        return current

    def close(self):
        self._closed = True


def decode_tta_batch(images):
    """decode a list of .tta images (bytes) in one GPU batch
    -> list of (status, TtaInfo, int32 interleaved PCM, first bad frame or
    None); status is an ATG_TD_* code (0 = every frame decoded), the PCM ends
    before the first bad frame"""
    images = list(images)
    data, spans = _atgpu.pack_images(images)
    tracks, infos = [], []
    for img, (offset, nbytes) in zip(images, spans):
        st, info, sizes = _atgpu.tta_read_info(img)
        if st:
            raise _tta_init_error(st, info.stage)
        tracks.append(_atgpu.tta_dec_track(offset, nbytes, info, sizes))
        infos.append(info)
    pcm_i32, res = _atgpu.tta_decoder().decode(data, tracks)
    out = []
    for info, r in zip(infos, res):
        out.append((r.status, info,
                    pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * info.channels],
                    None if r.status == 0 else int(r.n_frames)))
    return out


# --------------------------------------------------------------- Shorten
def _shn_error(table, status):
    kind, msg = table.get(status, (ValueError, "unknown value from read_framelist()"))
    return kind(msg)


class SHNDecoder(object):
    """reference src/decoders/shn.c SHNDecoder(file), decoded on the GPU
    (shn_decode.hip):

      SHNDecoder(file)   file object or bytes; ValueError for a wrong magic
                         number, version or file type, IOError for a header
                         that ends early (:37-96)
      .sample_rate .bits_per_sample .channels .channel_mask
      .read(n)           one set of channels (one block) per call, an empty
                         FrameList after QUIT; ValueError for an unknown
                         command and IOError for a stream that ends early,
                         once the blocks before it are out (:153-191)
      .pcm_split()       (bytes in front of the audio, bytes after it) from
                         the VERBATIM commands (:193-294)
      .close()
    """

    def __init__(self, file):
        data = _file_bytes(file)
        st, info = _atgpu.shn_read_info(data)
        if st:
            raise _shn_error(_atgpu.SHN_HEADER_ERRORS, st)
        self._data = data
        self._info = info
        self.sample_rate = info.sample_rate
        self.bits_per_sample = info.bits_per_sample
        self.channels = info.channels
        self.channel_mask = info.channel_mask
        self._closed = False
        self._decoded = None
        self._frame = 0    # sets of channels handed out
        self._sample = 0   # and their samples

    def _decode(self):
        if self._decoded is None:
            self._decoded = decode_shn_batch([self._data], details=True)[0]
        return self._decoded

    def read(self, pcm_frames=None):
        _check_open(self, "read")
        status, _, samples, _, _, lengths = self._decode()
        if self._frame >= len(lengths):
            if status != _atgpu.SHN_END_OF_STREAM:
                raise _shn_error(_atgpu.SHN_READ_ERRORS, status)
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        a = self._sample
        n = lengths[self._frame]
        self._frame += 1
        self._sample += n * self.channels
        return pcm.FrameList._wrap(samples[a:a + n * self.channels].copy(), self.channels,
                                   self.bits_per_sample)

    def pcm_split(self):
        status, _, _, head, foot, _ = self._decode()
        if status != _atgpu.SHN_END_OF_STREAM:
            raise IOError("I/O error reading Shorten file")
        return head, foot

    def close(self):
        self._closed = True


def decode_shn_batch(images, details=False):
    """decode a list of .shn images (bytes) in one GPU batch
    -> list of (status, ShnInfo, int32 interleaved PCM, header bytes, footer
    bytes); status is an ATG_SHN_* code (1 = the stream ended with QUIT), the
    PCM ends before the first incomplete set of channels.  With details, each
    tuple ends with the frame counts of the stream's sets of channels."""
    images = list(images)
    data, spans = _atgpu.pack_images(images)
    tracks, infos = [], []
    for img, (offset, nbytes) in zip(images, spans):
        st, info = _atgpu.shn_read_info(img)
        if st:
            raise _shn_error(_atgpu.SHN_HEADER_ERRORS, st)
        tracks.append(_atgpu.shn_dec_track(offset, nbytes, info))
        infos.append(info)
    # the block lengths are read inside the decoder's locked decode-and-fetch
    pcm_i32, res, verb, *lengths = _atgpu.shn_decoder().decode(data, tracks, blocks=details)
    out = []
    for k, (info, r) in enumerate(zip(infos, res)):
        v = verb[r.verbatim_offset:r.verbatim_offset + r.header_bytes + r.footer_bytes].tobytes()
        one = (r.status, info, pcm_i32[r.pcm_offset:r.pcm_offset + r.pcm_frames * info.channels],
               v[:r.header_bytes], v[r.header_bytes:])
        if details:
            one += ([int(x) for x in lengths[0][k]],)
        out.append(one)
    return out


# --------------------------------------------------------------- WavPack
def _wv_error(status):
    msg = _atgpu.WVD_MESSAGES.get(status, "unspecified error")
    if status in (_atgpu.WVD_IO_ERROR, _atgpu.WVD_BLOCK_DATA_IO):
        return IOError(msg)
    return ValueError(msg)


class WavPackDecoder(object):
    """reference src/decoders/wavpack.c WavPackDecoder(file), decoded on the
    GPU (wavpack_decode.hip):

      WavPackDecoder(file)  file object positioned at the first "wvpk" block,
                            or bytes; ValueError / IOError as
                            WavPackDecoder_init raises them (:24-187)
      .sample_rate .bits_per_sample .channels .channel_mask
      .read(n)              one block set per call (a set: one block per
                            channel pair, all of the same PCM frames); an
                            empty FrameList once every PCM frame is out.  The
                            error of a bad set is raised by the call that
                            reaches it, an MD5 mismatch once, by the first
                            call after the last set (:261-361)
      .seek(offset)         the latest initial block with samples whose index
                            is not beyond the offset (:363-447); the MD5 is
                            checked again only after a seek to the start
      .close()
    """

    def __init__(self, file):
        data = _file_bytes(file)
        st, info, blocks = _atgpu.wv_read_info(data)
        if st:
            raise _wv_error(st)
        self._data = data
        self._info = info
        self._blocks = blocks
        self.sample_rate = info.sample_rate
        self.bits_per_sample = info.bits_per_sample
        self.channels = info.channels
        self.channel_mask = info.channel_mask
        self.total_frames = info.total_pcm_frames
        # the first block of every set: (block_index, block_samples, initial)
        self._sets = []
        for k in range(info.n_blocks - info.tail_blocks):
            b = blocks[k]
            if b.set == len(self._sets):
                self._sets.append((b.block_index, b.block_samples,
                                   bool(b.flags & _atgpu.WV_INITIAL)))
        self._set = 0
        self._remaining = info.total_pcm_frames
        self._check_md5 = True
        self._md5_failed = False
        self._closed = False
        self._decoded_from = None

    def _decode(self):
        """the sets from the current one on, in one GPU call"""
        if self._decoded_from is not None and self._decoded_from <= self._set:
            return
        data, _ = _atgpu.pack_images([self._data])
        # 8-bit samples are hashed as unsigned bytes (WavPackDecoder_update_md5sum)
        check = 2 if (self._check_md5 and self._set == 0) else 0
        track = _atgpu.wv_dec_track(0, len(self._data), self._info, self._blocks, self._set,
                                    check_md5=check)
        pcm_i32, res = _atgpu.wv_decoder().decode(data, [track])
        r = res[0]
        self._pcm = pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * self.channels]
        self._good = r.n_sets
        self._status = r.status
        self._decoded_from = self._set
        self._md5_failed = bool(check) and r.status == _atgpu.WVD_MD5_MISMATCH
        # sample index of every decoded set in self._pcm
        self._starts = [0]
        for k in range(self._set, self._set + r.n_sets):
            self._starts.append(self._starts[-1] + self._sets[k][1] * self.channels)

    def read(self, pcm_frames):
        _check_open(self, "read")
        if self._remaining == 0:
            if self._check_md5 and self._info.has_md5:
                self._check_md5 = False
                if self._decoded_from is None and self.total_frames == 0:
                    self._decode()
                if self._md5_failed:
                    raise _wv_error(_atgpu.WVD_MD5_MISMATCH)
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        self._decode()
        k = self._set - self._decoded_from
        if k >= self._good:
            raise _wv_error(self._status)
        a, b = self._starts[k], self._starts[k + 1]
        self._remaining -= min(self._remaining, self._sets[self._set][1])
        self._set += 1
        return pcm.FrameList._wrap(self._pcm[a:b].copy(), self.channels, self.bits_per_sample)

    def seek(self, pcm_frame_offset):
        pcm_frame_offset = _seek_offset(self, pcm_frame_offset)
        best, best_set = 0, 0
        for k, (index, samples, initial) in enumerate(self._sets):
            if initial and samples:
                if index > pcm_frame_offset:
                    break
                best, best_set = index, k
        self._set = best_set
        self._remaining = self.total_frames - min(best, self.total_frames)
        self._check_md5 = best == 0
        if self._decoded_from is not None and best_set < self._decoded_from:
            self._decoded_from = None
        return best

    def close(self):
        self._closed = True


def decode_wavpack_batch(images, md5_mode=1):
    """decode a list of .wv images (bytes) in one GPU batch; md5_mode 1 hashes
    signed bytes at every width, as the reference's standalone decoder does,
    2 hashes 8-bit samples unsigned, as WavPackDecoder does, 0 skips the MD5
    -> list of (status, WvInfo, int32 interleaved PCM, first bad set or
    None); status is an ATG_WVD_* code (0 = every set decoded and the MD5,
    where there is one, agrees), the PCM ends before the first bad set.  An
    image the reference's decoder would not open has its status, no info
    (None) and no PCM."""
    images = list(images)
    infos, tables = [], []
    for img in images:
        st, info, blocks = _atgpu.wv_read_info(img)
        infos.append((st, None if st else info))
        tables.append(blocks)
    good = [k for k, (st, _) in enumerate(infos) if not st]
    data, spans = _atgpu.pack_images([images[k] for k in good])
    tracks = [_atgpu.wv_dec_track(offset, nbytes, infos[k][1], tables[k], check_md5=md5_mode)
              for k, (offset, nbytes) in zip(good, spans)]
    pcm_i32, res = _atgpu.wv_decoder().decode(data, tracks)
    out, k = [], 0
    for st, info in infos:
        if info is None:
            out.append((st, None, np.zeros(0, dtype=np.int32), 0))
            continue
        r = res[k]
        k += 1
        bad = None if r.status in (0, _atgpu.WVD_MD5_MISMATCH) else int(r.n_sets)
        out.append((r.status, info,
                    pcm_i32[r.sample_offset:r.sample_offset + r.pcm_frames * info.channels],
                    bad))
    return out


# ------------------------------------------- uncompressed: WAV, AIFF, Sun AU
def decode_pcm_batch(images):
    """a list of RIFF WAVE, AIFF or Sun AU file images (bytes), told apart by
    magic and mixed freely, to integer PCM in one GPU batch: the headers are
    read on the host (wav.py's parser, atg_aiff_read_info, atg_au_read_info),
    the data chunks go up as they lie in the files, and one launch per sample
    layout unpacks them on the device (pcm_bytes.hip).
    -> list of (status, PcmImage, int32 interleaved PCM, frames); status is 0,
    or ATG_PCMF_TRUNCATED when the file holds fewer data bytes than its header
    says: the PCM is then the whole frames present.  A header error raises
    what the file's single-file reader raises."""
    from . import pcmfiles
    images = [bytes(i) for i in images]
    infos = [pcmfiles.image_info(i) for i in images]
    if not infos:
        return []
    runs, cap, n_samples = pcmfiles.plan(infos, 4)
    eng = _atgpu.engine()
    out = np.zeros(max(n_samples, 4), dtype=np.int32)
    d_bytes = eng.device_alloc(max(cap, 16))
    d_pcm = eng.device_alloc(out.nbytes)
    try:
        eng.copy_to_device(d_bytes, pcmfiles.gather(images, infos, cap))
        pcmfiles.unpack_groups(infos, runs, d_bytes, cap, d_pcm, _atgpu.PCM_S32, len(out))
        eng.copy_to_host(out, d_pcm)
    finally:
        eng.device_free(d_bytes)
        eng.device_free(d_pcm)
    return [(_atgpu.PCMF_TRUNCATED if i.frames < i.total_pcm_frames else 0, i,
             out[slot:slot + n], i.frames) for i, (_, n, slot) in zip(infos, runs)]


# -------------------------------------------------------------- Ogg FLAC
def _oggflac_error(r):
    """the exception the reference raises for a result: the frame's error
    first, then the container's, then the MD5's; None for success"""
    if r.status not in (_atgpu.FD_OK, _atgpu.FD_MD5):
        if r.status == _atgpu.FD_EOF:
            return IOError("I/O error decoding FLAC frame")
        return ValueError(_atgpu.FD_MESSAGES.get(r.status, "Error"))
    if r.ogg_status != _atgpu.OGG_OK:
        msg = _atgpu.OGG_MESSAGES.get(r.ogg_status, "unknown error")
        return IOError(msg) if r.ogg_status in _atgpu.OGG_IOERRORS else ValueError(msg)
    if r.status == _atgpu.FD_MD5:
        return ValueError(_atgpu.FD_MESSAGES[_atgpu.FD_MD5])
    return None


def _oggflac_in_headers(r):
    """the failure came before the first audio packet: the reference raises
    it from OggFlacDecoder's constructor (oggflac.c:86-107)"""
    if r.ogg_status == _atgpu.OGG_OK:
        return False
    return r.ogg_status >= _atgpu.OGG_PACKET_BYTE or r.packets < 1 + r.header_packets


def decode_oggflac_batch(images):
    """decode a list of Ogg FLAC (.oga) images (bytes) in one GPU batch: the
    container (pages, page checksums, packets) and the frames.
    -> list of (OggFlacDecResult, int32 interleaved PCM, frame block sizes);
    the result's status / ogg_status say what ended the stream (both 0 =
    decoded and MD5-verified), the PCM is what came before that."""
    images = [bytes(i) for i in images]
    devs = _atgpu.batch_devices()
    ranges = (_atgpu.shard_ranges([max(1, len(i)) for i in images], len(devs))
              if len(devs) > 1 else [(0, len(images))])

    def shard(i):
        t0, t1 = ranges[i]
        data, tracks = _atgpu.oggflac_pack(images[t0:t1])
        dec = (_atgpu.decoder() if len(ranges) == 1
               else _atgpu.shard_object("decoder", i, devs[i]))
        return dec.decode_oggflac(data, tracks)

    out = []
    for pcm_i32, res, bss in _atgpu.run_shards(shard, len(ranges)):
        frame = 0
        for r in res:
            a = r.sample_offset
            out.append((r, pcm_i32[a:a + r.pcm_frames * r.channels],
                        bss[frame:frame + r.n_frames]))
            frame += r.n_frames
    return out


class OggFlacDecoder(object):
    """reference src/decoders/oggflac.c OggFlacDecoder(filename, channel_mask),
    decoded on the GPU (ogg_demux.hip, flac_decode.hip):

      OggFlacDecoder(filename, channel_mask)
                     IOError if the file cannot be opened; the container's
                     and the first packet's errors up to the first audio
                     packet (ValueError, or IOError for a premature EOF, a
                     stream that finishes among its header packets and a short
                     STREAMINFO) (:53-123)
      .sample_rate .bits_per_sample .channels .channel_mask
      .read(n)       one FLAC frame per call; ValueError with the reference's
                     message for a bad frame or page, IOError "I/O error
                     decoding FLAC frame" for a frame cut by its packet,
                     IOError for a premature EOF; at the end of the stream the
                     MD5 check, then empty FrameLists (:145-273)
      .close()       further reads raise ValueError
    """

    def __init__(self, filename, channel_mask):
        if not isinstance(filename, str) or isinstance(channel_mask, bool) or \
                not isinstance(channel_mask, int):
            raise TypeError("OggFlacDecoder(filename: str, channel_mask: int)")
        if channel_mask < 0:
            raise ValueError("channel_mask must be >= 0")
        with open(filename, "rb") as f:  # IOError with errno + filename
            data = f.read()
        r, samples, sizes = decode_oggflac_batch([data])[0]
        if _oggflac_in_headers(r):
            raise _oggflac_error(r)
        self.sample_rate = r.sample_rate
        self.bits_per_sample = r.bits_per_sample
        self.channels = r.channels
        self.channel_mask = channel_mask
        self._samples = samples
        self._sizes = [int(x) for x in sizes]
        self._error = _oggflac_error(r)
        self._frame = 0
        self._at = 0
        self._finalized = False
        self._closed = False

    def read(self, pcm_frames=None):
        _check_open(self, "read")
        if self._finalized:
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        if self._frame < len(self._sizes):
            n = self._sizes[self._frame] * self.channels
            self._frame += 1
            a, self._at = self._at, self._at + n
            return pcm.FrameList._wrap(self._samples[a:a + n].copy(), self.channels,
                                       self.bits_per_sample)
        if self._error is not None:
            raise self._error
        self._finalized = True
        return pcm.empty_framelist(self.channels, self.bits_per_sample)

    def close(self):
        self._closed = True


# ------------------------------------------------------------------ DVD-Audio
class DvdaResult(object):
    """one title of decode_dvda_batch: the fields of the C ABI's
    atg_aob_result (status, stop_sector, sample_rate, bits_per_sample,
    channels, channel_mask, channel_assignment, good_frames, sample_offset)
    and, for a title whose status is DVDA_MLP, those of atg_mlp_result that
    it adds: mlp_status (ATG_MLP_*; None for a PCM title), stop_unit,
    access_units, substreams"""

    FIELDS = ("status", "stop_sector", "sample_rate", "bits_per_sample", "channels",
              "channel_mask", "channel_assignment", "good_frames", "sample_offset")

    def __init__(self, r, mlp=None, sample_base=0):
        src = r if mlp is None else mlp
        for f in self.FIELDS:
            setattr(self, f, int(getattr(src, f)))
        self.status = int(r.status)
        self.sample_offset += sample_base
        self.mlp_status = None if mlp is None else int(mlp.status)
        self.stop_unit = 0 if mlp is None else int(mlp.stop_unit)
        self.access_units = 0 if mlp is None else int(mlp.access_units)
        self.substreams = 0 if mlp is None else int(mlp.substreams)

    @property
    def decodes(self):
        """the title has stream attributes and may have frames"""
        return bool(self.sample_rate) and (
            self.status in (_atgpu.DVDA_OK, _atgpu.DVDA_BAD_SECTOR) or self.mlp_status is not None)


# the reference's mlp_python_exception / mlp_python_exception_msg per status
MLP_ERRORS = {
    _atgpu.MLP_IO_ERROR: (IOError, "I/O error reading MLP stream"),
    _atgpu.MLP_INVALID_MAJOR_SYNC: (ValueError, "invalid MLP major sync"),
    _atgpu.MLP_INVALID_EXTRAWORD: (ValueError,
                                   "invalid extraword present value in substream info"),
    _atgpu.MLP_INVALID_RESTART_HEADER: (ValueError, "invalid MLP restart header"),
    _atgpu.MLP_INVALID_DECODING_PARAMETERS: (ValueError, "invalid MLP decoding parameters"),
    _atgpu.MLP_INVALID_MATRIX_PARAMETERS: (ValueError, "invalid MLP matrix parameters"),
    _atgpu.MLP_INVALID_CHANNEL_PARAMETERS: (ValueError, "invalid MLP channel parameters"),
    _atgpu.MLP_INVALID_BLOCK_DATA: (ValueError, "invalid MLP block data"),
    _atgpu.MLP_INVALID_FILTER_PARAMETERS: (ValueError, "invalid MLP filter parameters"),
    _atgpu.MLP_PARITY_MISMATCH: (ValueError, "parity mismatch decoding MLP substream"),
    _atgpu.MLP_CRC8_MISMATCH: (ValueError, "CRC8 mismatch decoding MLP substream"),
    _atgpu.MLP_UNSUPPORTED: (ValueError, "MLP stream outside the decoder's limits"),
}


class DvdaBatch(object):
    """decode_dvda_batch's answer with the PCM left on the device: .results
    (one DvdaResult per title) and .d_pcm, interleaved int32 in device memory, title i's
    samples from index results[i].sample_offset; close() frees it"""

    def __init__(self, results, d_pcm, total_samples):
        self.results, self.d_pcm, self.total_samples = results, d_pcm, total_samples

    def close(self):
        if self.d_pcm:
            _atgpu.engine().device_free(self.d_pcm)
            self.d_pcm = None


def _dvda_range(title):
    """a DVDATitle, or (audio_ts, titleset, start_sector, end_sector) ->
    (AOB list, start sector)"""
    from . import dvda
    if isinstance(title, tuple):
        audio_ts, titleset, start, end = title
    else:
        audio_ts, titleset = title.dvdaudio.audio_ts_path, title.titleset
        start, end = title.tracks[0].first_sector, title.tracks[-1].last_sector
    if end < start:
        raise ValueError("end_sector is before start_sector")
    return dvda.find_aobs(audio_ts, titleset), start


def decode_dvda_batch(titles, on_device=False):
    """decode DVD-Audio titles in one GPU batch.  titles: audiotools.dvda
    DVDATitle objects, or (audio_ts, titleset, start_sector, end_sector)
    tuples.  As in the reference, end_sector does not bound the reads (aob.c
    reads on into the following sectors of the titleset): a title runs from
    start_sector to the last sector of the titleset's AOB files, and
    end_sector is taken for interface parity only.  The host reads that
    sector range alone, across the ATS_XX_1..9.AOB boundaries.
    Titles whose first sector is MLP (status DVDA_MLP) go through the MLP
    calls (mlp_decode.hip) in the same batch; their samples follow the PCM
    titles' in the one output buffer.
    -> per title (DvdaResult, int32 interleaved PCM of its good_frames), or
    with on_device a DvdaBatch that keeps the PCM in device memory."""
    from . import dvda
    parts, table, pos = [], [], 0
    for title in titles:
        aobs, start = _dvda_range(title)
        data = dvda.read_sectors(aobs, start)
        table.append((pos, len(data) // _atgpu.AOB_SECTOR_BYTES))
        parts.append(data)
        pos += len(data)
    data = np.frombuffer(b"".join(parts), dtype=np.uint8)
    eng = _atgpu.engine()
    d_bytes = eng.device_alloc(max(16, data.nbytes))
    d_pcm = None
    try:
        if data.nbytes:
            eng.copy_to_device(d_bytes, data)
        scan, n_pcm = _atgpu.aob_scan_device(d_bytes, data.nbytes, table, _atgpu.PCM_S32)
        mlp = [i for i, r in enumerate(scan) if r.status == _atgpu.DVDA_MLP]
        mlp_table = [table[i] for i in mlp]
        n_mlp = _atgpu.mlp_scan_device(d_bytes, data.nbytes, mlp_table, _atgpu.PCM_S32)[1] \
            if mlp else 0
        total = n_pcm + n_mlp       # n_pcm is a multiple of 4: 16-byte aligned
        d_pcm = eng.device_alloc(max(16, 4 * total))
        res = [DvdaResult(r) for r in _atgpu.aob_decode_device(
            d_bytes, data.nbytes, table, d_pcm, _atgpu.PCM_S32, n_pcm)]
        if mlp:
            for i, m in zip(mlp, _atgpu.mlp_decode_device(
                    d_bytes, data.nbytes, mlp_table, d_pcm + 4 * n_pcm, _atgpu.PCM_S32, n_mlp)):
                res[i] = DvdaResult(res[i], m, n_pcm)
        if on_device:
            batch, d_pcm = DvdaBatch(res, d_pcm, total), None
            return batch
        out = eng.copy_to_host(np.empty(max(1, total), dtype=np.int32), d_pcm)
        return [(r, out[r.sample_offset:r.sample_offset + r.good_frames * r.channels])
                for r in res]
    finally:
        eng.device_free(d_bytes)
        if d_pcm:
            eng.device_free(d_pcm)


class DVDA_Title(object):
    """reference src/decoders/aob.c DVDA_Title(audio_ts, titleset,
    start_sector, end_sector), decoded on the GPU (aob_decode.hip):

      .sample_rate .bits_per_sample .channels .channel_mask
                         0 until the first next_track(), as in the reference
      .pcm_frames        frames left in the current track
      .next_track(pts_ticks)
                         the next track holds round(pts_ticks * sample_rate /
                         90000) frames; ValueError "current track has not
                         been exhausted" before the current one is read out,
                         IOError for a bad first sector, ValueError for an
                         unknown codec ID, for an MLP stream that does not
                         start with a major sync and for stream attributes
                         the reference asserts on
      .read(n)           up to n frames of the track as a pcm.FrameList, an
                         empty one once it is exhausted; IOError "I/O reading
                         PCM packet" for a read that needs bytes of the
                         sector the title stops at, after the whole frames
                         before it have been delivered; for an MLP title
                         "I/O reading MLP packet", or the reference's own
                         message and exception type for the access unit that
                         fails (MLP_ERRORS)
      .close()           no effect, as in the reference

    PCM and MLP titles alike (aob_decode.hip, mlp_decode.hip).
    The title is decoded on the device once, at the first next_track();
    tracks are consecutive windows of it.  There is no read-ahead: an error
    surfaces at the read that needs the bad sector.  end_sector does not
    bound the reads (see decode_dvda_batch).  IOError when the titleset's
    AOB files cannot be found."""

    def __init__(self, audio_ts, titleset, start_sector, end_sector, cdrom=None):
        if cdrom is not None:
            raise ValueError("CPPM-protected discs are not supported: cdrom must be None")
        self._title = (audio_ts, int(titleset), int(start_sector), int(end_sector))
        _dvda_range(self._title)     # IOError now, as the reference's constructor
        self.sample_rate = self.bits_per_sample = self.channels = self.channel_mask = 0
        self.pcm_frames = 0
        self._result = self._pcm = None
        self._pos = 0

    def next_track(self, pts_ticks):
        if self.pcm_frames:
            raise ValueError("current track has not been exhausted")
        if self._result is None:
            r, samples = decode_dvda_batch([self._title])[0]
            if r.status == _atgpu.DVDA_BAD_SECTOR and r.stop_sector == 0:
                raise IOError("I/O error reading initialization packet")
            if r.status == _atgpu.DVDA_UNKNOWN_CODEC:
                raise ValueError("unknown codec ID")
            if r.mlp_status == _atgpu.MLP_NO_MAJOR_SYNC:
                raise ValueError("MLP stream does not start with a major sync")
            if not r.decodes:
                raise ValueError("unsupported DVD-Audio stream attributes")
            self._result, self._pcm = r, samples
            self.sample_rate, self.bits_per_sample = r.sample_rate, r.bits_per_sample
            self.channels, self.channel_mask = r.channels, r.channel_mask
        from .dvda import track_frames
        self.pcm_frames = track_frames(pts_ticks, self.sample_rate)

    def read(self, pcm_frames=4096):
        if not self.pcm_frames:
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        have = self._result.good_frames - self._pos
        if have <= 0:
            if self._result.mlp_status is None:
                raise IOError("I/O reading PCM packet")
            kind, text = MLP_ERRORS.get(self._result.mlp_status,
                                        (IOError, "I/O reading MLP packet"))
            raise kind(text)
        n = min(max(1, int(pcm_frames)), self.pcm_frames, have)
        a = self._pos * self.channels
        self._pos += n
        self.pcm_frames -= n
        return pcm.FrameList._wrap(self._pcm[a:a + n * self.channels].copy(), self.channels,
                                   self.bits_per_sample)

    def close(self):
        """does nothing, as in the reference: the tracks that follow stay
        readable after a caller closes the reader of one track"""
