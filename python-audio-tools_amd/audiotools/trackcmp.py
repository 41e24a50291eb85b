"""audiotools.trackcmp — are two files the same audio?  The comparison the
reference's trackcmp tool makes (its cmp_files and image_compare), for a
whole batch on the GPU, and the windowed readers it rests on.

Host side: PCMReaderHead / PCMReaderDeHead / PCMReaderWindow (reference
audiotools/__init__.py:4842-4975) and frame_cmp_value, the value pcm_frame_cmp
gives for two streams from their lengths and first differing frame.

Device side: compare_files_batch, compare_image_batch and find_offset_batch
take files of any supported format, mixed freely.  The files are told apart
by magic, every image of one format is decoded in one call of that format's
decoder, the PCM stays in the decoders' device buffers, and one launch of
csrc/pcm_compare.hip compares views into them.  compare_pcm_batch does the
same for numpy arrays.  Everything runs on the default device.
"""

import sys

import numpy as np

from . import FRAMELIST_SIZE
from . import _atgpu
from . import pcm
from . import batchfiles
from .batchfiles import (_open, _read, _decode_flac, _decode_oggflac,  # noqa: F401
                         _decode_alac, _decode_tta, _decode_wavpack, _decode_shn, _decode_pcm)

__all__ = ["PCMReaderHead", "PCMReaderDeHead", "PCMReaderWindow", "frame_cmp_value",
           "compare_files_batch", "compare_image_batch", "find_offset_batch",
           "compare_pcm_batch", "PARAMETER_MISMATCH", "READ_ERROR"]

PARAMETER_MISMATCH = -1  # sample rate, channel count or bits per sample differ
READ_ERROR = -2          # a file does not open or does not decode cleanly


# ------------------------------------------------------------ host readers
class PCMReaderHead(object):
    """the first pcm_frames frames of a reader's stream; a shorter stream is
    padded with silence to that length"""

    def __init__(self, pcmreader, pcm_frames):
        if pcm_frames < 0:
            raise ValueError("invalid pcm_frames value")
        self.pcmreader = pcmreader
        self.sample_rate = pcmreader.sample_rate
        self.channels = pcmreader.channels
        self.channel_mask = pcmreader.channel_mask
        self.bits_per_sample = pcmreader.bits_per_sample
        self.pcm_frames = pcm_frames  # still to hand out
        self._closed = False

    def read(self, pcm_frames):
        if self._closed:
            raise ValueError("cannot read closed stream")
        if self.pcm_frames <= 0:
            return pcm.empty_framelist(self.channels, self.bits_per_sample)
        frame = self.pcmreader.read(pcm_frames)
        if frame.frames == 0:
            # the stream is over: the rest of the window is silence
            frame = pcm.from_list([0] * (self.pcm_frames * self.channels), self.channels,
                                  self.bits_per_sample, True)
        elif frame.frames > self.pcm_frames:
            frame = frame.split(self.pcm_frames)[0]
        self.pcm_frames -= frame.frames
        return frame

    def close(self):
        self.pcmreader.close()
        self._closed = True


class PCMReaderDeHead(object):
    """a reader's stream without its first pcm_frames frames; a negative
    count puts that many frames of silence in front instead"""

    def __init__(self, pcmreader, pcm_frames):
        self.pcmreader = pcmreader
        self.sample_rate = pcmreader.sample_rate
        self.channels = pcmreader.channels
        self.channel_mask = pcmreader.channel_mask
        self.bits_per_sample = pcmreader.bits_per_sample
        self.pcm_frames = pcm_frames  # still to drop (> 0) or to pad (< 0)
        self._closed = False

    def read(self, pcm_frames):
        if self._closed:
            raise ValueError("cannot read closed stream")
        if self.pcm_frames < 0:
            pad, self.pcm_frames = -self.pcm_frames, 0
            return pcm.from_list([0] * (pad * self.channels), self.channels,
                                 self.bits_per_sample, True)
        while self.pcm_frames > 0:
            frame = self.pcmreader.read(pcm_frames)
            if frame.frames == 0:
                # more to drop than the stream holds
                self.pcm_frames = 0
                return frame
            if frame.frames > self.pcm_frames:
                tail = frame.split(self.pcm_frames)[1]
                self.pcm_frames = 0
                return tail
            self.pcm_frames -= frame.frames
        return self.pcmreader.read(pcm_frames)

    def close(self):
        self.pcmreader.close()
        self._closed = True


def PCMReaderWindow(pcmreader, initial_offset, pcm_frames):
    """pcm_frames frames of pcmreader's stream from frame initial_offset on,
    silence wherever the window lies outside the stream"""
    if initial_offset == 0:
        return PCMReaderHead(pcmreader, pcm_frames)
    return PCMReaderHead(PCMReaderDeHead(pcmreader, initial_offset), pcm_frames)


def frame_cmp_value(first_mismatch, frames_a, frames_b, chunk=FRAMELIST_SIZE):
    """what pcm_frame_cmp returns for streams of frames_a and frames_b frames
    whose common prefix first differs at frame first_mismatch (None: it does
    not).  Streams of different lengths differ where the shorter one ends:
    pcm_frame_cmp reads both in chunks, and reports the end itself when it
    falls on a chunk boundary, else the last common frame (the chunk that
    holds the end compares unequal, and no frame of it does)."""
    if first_mismatch is not None:
        return first_mismatch
    if frames_a == frames_b:
        return None
    s = min(frames_a, frames_b)
    return s if s % chunk == 0 else s - 1


def _Batch():
    """the files of one call (batchfiles._Batch), decoded by this module's
    _decode_<kind> names"""
    return batchfiles._Batch(sys.modules[__name__])


def _precheck(a, b):
    """what cmp_files answers from two headers alone, or "decode" """
    if a is None or b is None:
        return READ_ERROR
    if (a.sample_rate != b.sample_rate or a.channels != b.channels or
            a.bits_per_sample != b.bits_per_sample):
        return PARAMETER_MISMATCH
    if a.channel_mask != 0 and b.channel_mask != 0 and a.channel_mask != b.channel_mask:
        return 0  # pcm_frame_cmp's channel-mask rule
    return "decode"


def compare_files_batch(pairs):
    """trackcmp's cmp_files for a list of (file_a, file_b), each a filename
    or a bytes image of any supported format.
    -> per pair None when the PCM is equal, the first mismatching PCM frame
    (>= 0), -1 when sample rate, channel count or bits per sample differ
    (from the headers: nothing is decoded for that pair), -2 when a file
    does not open or decodes with an error status"""
    batch = _Batch()
    plans = []
    for fa, fb in pairs:
        i, j = batch.add(fa), batch.add(fb)
        verdict = _precheck(batch.headers[i], batch.headers[j])
        if verdict == "decode":
            batch.want(i)
            batch.want(j)
            verdict = ("decode", i, j)
        plans.append(verdict)
    try:
        batch.decode()
        out, table, where = [None] * len(plans), [], []
        for k, plan in enumerate(plans):
            if not isinstance(plan, tuple):
                out[k] = plan
                continue
            _, i, j = plan
            if not (batch.ok(i) and batch.ok(j)):
                out[k] = READ_ERROR
                continue
            frames = min(batch.frames(i), batch.frames(j))
            table.append(_atgpu.pcm_pair(batch.view(i), batch.view(j), frames,
                                         batch.headers[i].channels))
            where.append(k)
        for k, first in zip(where, _atgpu.pcm_compare_device(table)):
            _, i, j = plans[k]
            out[k] = frame_cmp_value(first, batch.frames(i), batch.frames(j))
        return out
    finally:
        batch.close()


def compare_image_batch(jobs):
    """trackcmp's image_compare for a list of (image_file, [track_file, ...]):
    track t against the window of the image that starts at the sum of the
    earlier tracks' total_frames() and has its own total_frames() length,
    silence where the window passes the image's end.  Every image and every
    track is decoded once.
    -> per job a list of None / first mismatching frame / -1 / -2 as
    compare_files_batch gives them"""
    batch = _Batch()
    plans = []
    for image, tracks in jobs:
        i = batch.add(image)
        row, start = [], 0
        for t in tracks:
            j = batch.add(t)
            verdict = _precheck(batch.headers[i], batch.headers[j])
            if verdict == "decode":
                batch.want(i)
                batch.want(j)
                verdict = ("decode", i, j, start, batch.headers[j].total_frames)
            if batch.headers[j] is not None:
                start += batch.headers[j].total_frames
            row.append(verdict)
        plans.append(row)
    try:
        batch.decode()
        out, table, where = [[None] * len(row) for row in plans], [], []
        for a, row in enumerate(plans):
            for t, plan in enumerate(row):
                if not isinstance(plan, tuple):
                    out[a][t] = plan
                    continue
                _, i, j, start, length = plan
                if not (batch.ok(i) and batch.ok(j)):
                    out[a][t] = READ_ERROR
                    continue
                frames = min(length, batch.frames(j))
                table.append(_atgpu.pcm_pair(batch.view(i, start), batch.view(j), frames,
                                             batch.headers[i].channels))
                where.append((a, t))
        for (a, t), first in zip(where, _atgpu.pcm_compare_device(table)):
            _, i, j, start, length = plans[a][t]
            out[a][t] = frame_cmp_value(first, length, batch.frames(j))
        return out
    finally:
        batch.close()


def find_offset_batch(pairs, max_offset):
    """do two files hold the same audio at some shift?  Per (file_a, file_b):
    A's whole length is the range, B is read with silence outside it, and
    the shift k of smallest |k| <= max_offset with A(i) == B(i + k) for every
    frame of A is looked for (+k before -k).
    -> per pair (offset or None, first mismatching frame at shift 0 or None),
    or -1 / -2 as compare_files_batch gives them"""
    batch = _Batch()
    plans = []
    for fa, fb in pairs:
        i, j = batch.add(fa), batch.add(fb)
        verdict = _precheck(batch.headers[i], batch.headers[j])
        if verdict == 0:
            verdict = (None, 0)  # the channel-mask rule: no shift is looked for
        elif verdict == "decode":
            batch.want(i)
            batch.want(j)
            verdict = ("decode", i, j)
        plans.append(verdict)
    try:
        batch.decode()
        out, table, where = [None] * len(plans), [], []
        for k, plan in enumerate(plans):
            if not (isinstance(plan, tuple) and plan[0] == "decode"):
                out[k] = plan
                continue
            _, i, j = plan
            if not (batch.ok(i) and batch.ok(j)):
                out[k] = READ_ERROR
                continue
            table.append(_atgpu.pcm_pair(batch.view(i), batch.view(j), batch.frames(i),
                                         batch.headers[i].channels))
            where.append(k)
        for k, found in zip(where, _atgpu.pcm_offset_search_device(table, max_offset)):
            out[k] = found
        return out
    finally:
        batch.close()


def compare_pcm_batch(a_list, b_list, channels):
    """pcm_frame_cmp's value for pairs of interleaved PCM held in numpy int16
    or int32 arrays: the arrays go up to the device, one launch compares
    every pair's common prefix, and frame_cmp_value settles the lengths"""
    if len(a_list) != len(b_list):
        raise ValueError("a_list and b_list differ in length")
    arrays = [np.ascontiguousarray(x) for x in list(a_list) + list(b_list)]
    for x in arrays:
        if x.dtype not in (np.int16, np.int32):
            raise ValueError("PCM arrays must be int16 or int32")
        if x.ndim != 1 or len(x) % channels:
            raise ValueError("PCM arrays must hold whole interleaved frames")
    if not arrays:
        return []
    # every array on a 16-byte boundary of one buffer
    starts, pos = [], 0
    for x in arrays:
        starts.append(pos)
        pos += (x.nbytes + 15) // 16 * 16
    host = np.zeros(max(pos, 16), dtype=np.uint8)
    for x, s in zip(arrays, starts):
        host[s:s + x.nbytes] = x.view(np.uint8)
    eng = _atgpu.engine()
    d = eng.device_alloc(len(host))
    try:
        eng.copy_to_device(d, host)
        views = [_atgpu.pcm_view(d + s, _atgpu.PCM_S16 if x.dtype == np.int16
                                 else _atgpu.PCM_S32, len(x) // channels)
                 for x, s in zip(arrays, starts)]
        n = len(a_list)
        table = [_atgpu.pcm_pair(views[k], views[n + k],
                                 min(views[k].src_frames, views[n + k].src_frames), channels)
                 for k in range(n)]
        firsts = _atgpu.pcm_compare_device(table)
        return [frame_cmp_value(f, views[k].src_frames, views[n + k].src_frames)
                for k, f in enumerate(firsts)]
    finally:
        eng.device_free(d)
