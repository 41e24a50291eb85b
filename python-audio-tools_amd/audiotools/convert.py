"""audiotools.convert — a batch of files transcoded to FLAC on the device.

convert_files_batch is track2track's job for many files at once: every
source is opened and told apart by magic (batchfiles), all sources of one
format are decoded in one call of that format's decoder, the converter chain
runs over the decoded PCM where it lies (pcmconverter.run_chain_device:
csrc/pcm_chain.hip on either side of the resampler), the tracks that share
output parameters are encoded in one encode_device call each, and every
image is finished as FlacAudio.from_pcm finishes it.  The PCM never comes
back to the host; the .flac images do.
"""

import numpy as np

from . import DecodingError, EncodingError
from . import _atgpu
from .batchfiles import _Batch
from .flac import (COMPRESSION_PRESETS, DEFAULT_COMPRESSION, FlacAudio, finish_image,
                   padding_for, target_layout, _unlink)
from .pcmconverter import DevicePcm, plan_target, run_chain_device


def _frame_offsets(image, total_frames, interval, block_size):
    """the encoder's (byte offset, pcm frames) list as far as the SEEKTABLE
    needs it: a track of one seek point needs its first frame alone; a longer
    one has its frames walked by the decoder"""
    if total_frames == 0:
        return []
    if total_frames <= interval:
        return [(0, min(block_size, total_frames))]
    rc, si, _ = _atgpu.read_metadata(image)
    if rc:
        raise ValueError("the encoder's image does not parse")
    body = image[si.frames_offset:]
    body += b"\0" * ((-len(body)) % 4)
    _, _, offs, sizes = _atgpu.decoder().decode(
        body, [_atgpu.dec_track(0, len(image) - si.frames_offset, si)], fetch_pcm=False)
    if int(sizes.sum()) != total_frames:
        raise ValueError("the encoder's image does not decode to its frame count")
    return [(int(o), int(n)) for o, n in zip(offs, sizes)]


def convert_files_batch(sources, targets, sample_rate=None, channels=None, channel_mask=None,
                        bits_per_sample=None, compression=None, dither=None):
    """sources[k] (a filename or a bytes image of any supported format) ->
    the FLAC file targets[k], converted to the target parameters as
    PCMConverter converts (None keeps each source's own value).  The file is
    the one FlacAudio.from_pcm(targets[k], PCMConverter(BufferedPCMReader(
    source.to_pcm()), ...), compression, total_pcm_frames=<converted frames>)
    writes, except for where the dither bits fall behind a resampler (DESIGN
    section 4o).  dither: n -> bytes (default os.urandom), drawn source by
    source in argument order.
    -> per source a FlacAudio, or the DecodingError / EncodingError instance
    of a file that could not be read or written (no target is left for it and
    the others go on).  ValueError, before any GPU work, for a target that
    PCMConverter refuses."""
    sources, targets = list(sources), list(targets)
    if len(sources) != len(targets):
        raise ValueError("sources and targets differ in length")
    if compression is None or compression not in FlacAudio.COMPRESSION_MODES:
        compression = DEFAULT_COMPRESSION
    preset = COMPRESSION_PRESETS[compression]
    batch = _Batch()
    results = [None] * len(sources)
    jobs = []  # (k, file index, ChainPlan, mask to write)
    for k, (source, target) in enumerate(zip(sources, targets)):
        i = batch.add(source)
        h = batch.headers[i]
        if h is None:
            results[k] = DecodingError("%s cannot be opened as audio" % _name(source))
            continue
        plan = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate),
                           sample_rate, channels, channel_mask, bits_per_sample)
        try:
            mask = target_layout(target, plan.channels, plan.channel_mask)
        except EncodingError as err:
            results[k] = err
            continue
        batch.want(i)
        jobs.append((k, i, plan, mask))
    eng = _atgpu.engine()
    free = []
    try:
        batch.decode()
        good = []
        for job in jobs:
            if batch.ok(job[1]):
                good.append(job)
            else:
                results[job[0]] = DecodingError("%s does not decode cleanly"
                                                % _name(sources[job[0]]))
        views = [batch.views[i] for _, i, _, _ in good]
        done, free = run_chain_device(
            [DevicePcm(d, _atgpu.PCM_S32, p.sample_offset, p.frames) for d, p in views],
            [plan for _, _, plan, _ in good], dither)
        # one encode per (buffer, channels, bits, rate, PADDING size)
        groups = {}
        for (k, _, plan, mask), d in zip(good, done):
            pad = padding_for(d.frames, plan.sample_rate * 10)
            key = (d.d_pcm, d.fmt, plan.channels, plan.bits_per_sample, plan.sample_rate, pad)
            groups.setdefault(key, []).append((k, plan, mask, d))
        for (d_pcm, fmt, ch, bits, rate, pad), members in groups.items():
            try:
                opts = _atgpu.make_options(padding_size=pad, **preset)
                tracks = [(d.sample_offset // ch, d.frames, None) for _, _, _, d in members]
                _, nb = eng.bounds(opts, tracks, ch, bits)
                d_out = eng.device_alloc(max(16, nb))
                free.append(d_out)
                encoded = eng.encode_device(opts, d_pcm, fmt, tracks, ch, bits, rate, d_out, nb)
                out = eng.copy_to_host(np.empty(max(1, nb), dtype=np.uint8), d_out)
            except _atgpu.ATGError as err:
                for k, _, _, _ in members:
                    results[k] = EncodingError(str(err))
                continue
            for (k, plan, mask, d), res in zip(members, encoded):
                results[k] = _finish(targets[k], out[res.out_offset:res.out_offset + res.bytes]
                                     .tobytes(), res.status, plan, mask, d.frames,
                                     preset["block_size"])
        return results
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()


def _finish(target, image, status, plan, mask, frames, block_size):
    """one encoded image -> its finished file; the FlacAudio, or the
    EncodingError with no file left"""
    try:
        if status != 0:
            raise ValueError("the encoder reports status %d" % status)
        interval = plan.sample_rate * 10
        data = finish_image(image, _frame_offsets(image, frames, interval, block_size),
                            plan.channels, plan.bits_per_sample, mask, interval)
        with open(target, "wb") as f:
            f.write(data)
        return FlacAudio(target)
    except (IOError, OSError, ValueError) as err:
        _unlink(target)
        return EncodingError(str(err))


def _name(source):
    return source if isinstance(source, str) else "<%d-byte image>" % len(source)
