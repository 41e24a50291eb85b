"""audiotools.cdimage — CD images split into tracks and tracks joined into
images, a batch at a time (the reference's tracksplit and trackcat).

split_image_batch decodes every distinct image whole, once, into device
memory (batchfiles._Batch, the stream's MD5 checked), takes the tracks a
Sheet names as views into that PCM, and sends them through the converter
chain (pcmconverter.run_chain_device) and the batch writers
(targets.write_tracks), grouped across all images of the call.
join_tracks_batch decodes the files of all albums in one _Batch, lays each
album's pieces end to end in device memory and writes it as one track.  The
PCM never comes to the host.  No kernel of its own: decode, chain, encoders
and the AccurateRip pass are the ones every other batch entry uses.

plan_split and plan_join are the arithmetic and the refusals alone, pure
Python.  This module imports no torch.  Everything runs on the default
device.
"""

from collections import namedtuple

from . import DecodingError, EncodingError
from . import _atgpu
from .batchfiles import _Batch
from .cue import ERR_CUE_INVALID_FORMAT
from .flac import CUESHEET, FlacAudio, _blocks, cuesheet_sheet
from .pcmconverter import DevicePcm, plan_target, run_chain_device
from .sheets import Sheet, SheetException, read_sheet
from .shn import ShortenAudio
from .targets import (Track, _group_key, _per_target, prepare, resolve_compression,
                      resolve_types, write_tracks)
from .wav import WaveAudio

__all__ = ["SplitResult", "plan_split", "plan_join", "split_image_batch", "join_tracks_batch"]

ERR_TRACKSPLIT_NO_CUESHEET = u"you must specify a cuesheet to split audio file"
ERR_TRACKSPLIT_OVERLONG_CUESHEET = u"cuesheet too long for track being split"
ERR_FILES_REQUIRED = u"you must specify at least 1 supported audio file"
ERR_SAMPLE_RATE_MISMATCH = u"all audio files must have the same sample rate"
ERR_CHANNEL_COUNT_MISMATCH = u"all audio files must have the same channel count"
ERR_CHANNEL_MASK_MISMATCH = u"all audio files must have the same channel assignment"
ERR_BPS_MISMATCH = u"all audio files must have the same bits per sample"

# one image of split_image_batch: tracks[j] the target class's instance or
# the exception of track j; checksums [(v1, v2)] per track or None; offsets
# the uint32 array [track][k + max_offset] of v1 at offset k, or None; stats
# uploaded_bytes and decoded_frames (the image's file as it went to its
# decoder and the frames that came out; 0 where an earlier image of the call
# named the same file, which is read and decoded once) and encode_calls (the
# encode calls the image's tracks were part of)
SplitResult = namedtuple("SplitResult", "tracks checksums offsets stats")


# ------------------------------------------------------------------ planning
def _lengths(sheet, total_pcm_frames, sample_rate):
    if any(not list(t.indexes()) for t in sheet.tracks()):
        raise SheetException("a track of the cuesheet has no index")
    if not sheet.image_formatted():
        raise SheetException(ERR_CUE_INVALID_FORMAT)
    try:
        return list(sheet.pcm_lengths(total_pcm_frames, sample_rate))
    except KeyError:
        raise SheetException("a track of the cuesheet has no index 1")


def plan_split(sheet, total_pcm_frames, sample_rate):
    """tracksplit's cuts of an image of total_pcm_frames frames -> [(offset,
    length)] per sheet track, in PCM frames.  The lengths are
    sheet.pcm_lengths (index 1 to index 1) and the offsets add them up from
    frame 0, as the reference does: a first track whose index 1 is not 0
    shifts every cut.  SheetException with tracksplit's words for no sheet,
    a sheet not formatted for an image, and one whose last track would have
    no frames; a track before the last with a negative length is refused as
    not image formatted."""
    if sheet is None or not list(sheet.tracks()):
        raise SheetException(ERR_TRACKSPLIT_NO_CUESHEET)
    lengths = _lengths(sheet, total_pcm_frames, sample_rate)
    if lengths[-1] <= 0:
        raise SheetException(ERR_TRACKSPLIT_OVERLONG_CUESHEET)
    if min(lengths) < 0:
        raise SheetException(ERR_CUE_INVALID_FORMAT)
    cuts, at = [], 0
    for n in lengths:
        cuts.append((at, n))
        at += n
    return cuts


def plan_join(params, frames, sheet=None):
    """trackcat's checks of one album.  params: per file (sample_rate,
    channels, channel_mask, bits_per_sample); frames: per file its PCM
    frames -> the image's total frames.  ValueError with trackcat's words
    for an empty album, files that differ in one of the four, and a sheet
    that is not image formatted or longer than the files together."""
    params = list(params)
    if not params:
        raise ValueError(ERR_FILES_REQUIRED)
    for column, message in enumerate((ERR_SAMPLE_RATE_MISMATCH, ERR_CHANNEL_COUNT_MISMATCH,
                                      ERR_CHANNEL_MASK_MISMATCH, ERR_BPS_MISMATCH)):
        if len(set(int(p[column]) for p in params)) != 1:
            raise ValueError(message)
    total = sum(frames)
    if sheet is not None:
        lengths = _lengths(sheet, total, params[0][0])
        if lengths and lengths[-1] < 0:
            raise SheetException(ERR_TRACKSPLIT_OVERLONG_CUESHEET)
    return total


# ------------------------------------------------------------ the arguments
def _per_image(value, n, what):
    """None, or a list with one entry per image -> the list"""
    if value is None:
        return [None] * n
    value = list(value)
    if len(value) != n:
        raise ValueError("%s has %d entries for %d images" % (what, len(value), n))
    return value


def _nested(value, targets, what):
    """one value for every track, or per image one value or one per track
    -> per image a list with one entry per track"""
    if not isinstance(value, (list, tuple)):
        return [[value] * len(t) for t in targets]
    if len(value) != len(targets):
        raise ValueError("%s has %d entries for %d images" % (what, len(value), len(targets)))
    return [_per_target(v, len(t), what) for v, t in zip(value, targets)]


def _load_sheet(sheet):
    """a Sheet, or the file name of one -> the Sheet; SheetException"""
    if sheet is None or isinstance(sheet, Sheet):
        return sheet
    if isinstance(sheet, str):
        return read_sheet(sheet)
    if callable(getattr(sheet, "tracks", None)) and callable(getattr(sheet, "catalog", None)):
        return sheet
    raise ValueError("a sheet is a Sheet, a .cue or .toc file name, or None")


def _embedded_sheet(header):
    """the Sheet in a FLAC image's CUESHEET block, None without one"""
    if header.kind != "flac":
        return None
    try:
        for t, body in _blocks(header.image)[0]:
            if t == CUESHEET:
                return cuesheet_sheet(body, header.sample_rate)
    except (ValueError, IndexError, KeyError):
        pass
    return None


def _name(source):
    return source if isinstance(source, str) else "<%d-byte image>" % len(source)


# -------------------------------------------------------------------- split
def split_image_batch(images, targets, sheets=None, target_types=None, compression=None,
                      sample_rate=None, channels=None, channel_mask=None, bits_per_sample=None,
                      dither=None, accuraterip=False, max_offset=0):
    """tracksplit for a batch: images[k] (a filename or a bytes image of any
    format the decoders read) cut by sheets[k] (a Sheet, the name of a .cue
    or .toc file, or None for the sheet a FLAC image carries) into the files
    targets[k][j], one per sheet track.  target_types and compression are
    convert_files_batch's, given as one value for every track or per image
    one value or one per track; sample_rate, channels, channel_mask,
    bits_per_sample and dither are convert_files_batch's too.  For the
    dither, a track's place is its place in the arguments: under a
    DeviceDither track j of image k reads stream len(targets[0]) + ... +
    len(targets[k-1]) + j, whether the images before it fail or not, so one
    image's bits do not depend on another's fate.  A callable is drawn from
    in that order too, but only for the tracks that are converted (those of
    an image that fails, or that keep their bits, draw nothing), so what a
    track gets from it depends on the tracks before it.

    The cuts are plan_split's.  Every distinct image is decoded whole, once,
    with its stream's MD5 checked; track j's file is the one cls.from_pcm(
    targets[k][j], PCMConverter(BufferedPCMReader(PCMReaderWindow(
    image.to_pcm(), offset, length)), ...), compression,
    total_pcm_frames=<converted length>) writes, under the exceptions
    convert_files_batch names.

    accuraterip: for an image of 44100 Hz, 2 channels and 16 bits, the
    AccurateRip v1 / v2 of every track, computed on the image's PCM where it
    lies (first and last by position, each track's own length, the whole
    image readable across the cuts); with max_offset, v1 at every offset of
    [-max_offset, max_offset] too.  Other images get None.

    -> per image a SplitResult, or that image's exception with nothing
    written for it and the other images going on: SheetException (no sheet,
    an unreadable one, not formatted for an image, too long), ValueError (a
    wrong number of targets), DecodingError (the image cannot be opened or
    does not decode cleanly).  A track whose converted parameters its type
    cannot hold gets that type's exception in .tracks, before any GPU work
    for it.  ValueError, before any GPU work, for lists of the wrong length,
    an unknown target type and a target PCMConverter refuses."""
    images = list(images)
    n = len(images)
    targets = [list(t) for t in _per_image(targets, n, "targets")]
    sheets = _per_image(sheets, n, "sheets")
    if target_types is None:
        classes = [[FlacAudio] * len(t) for t in targets]
    else:
        classes = [resolve_types(v, t) for v, t in
                   zip(_nested(target_types, targets, "target_types"), targets)]
    modes = [resolve_compression(v, c) for v, c in
             zip(_nested(compression, targets, "compression"), classes)]
    max_offset = int(max_offset)
    if max_offset < 0:
        raise ValueError("max_offset must not be negative")
    first_stream = [0] * n
    for k in range(1, n):
        first_stream[k] = first_stream[k - 1] + len(targets[k - 1])

    batch = _Batch()
    results = [None] * n
    files = [None] * n   # the image's index in the batch
    cuts = [None] * n
    jobs = {}            # (k, j) -> (ChainPlan, what prepare() returned)
    for k, image in enumerate(images):
        try:
            sheet = _load_sheet(sheets[k])
        except (SheetException, ValueError) as err:
            results[k] = err
            continue
        i = batch.add(image)
        h = batch.headers[i]
        if h is None:
            results[k] = DecodingError("%s cannot be opened as audio" % _name(image))
            continue
        if sheet is None:
            sheet = _embedded_sheet(h)
        try:
            cuts[k] = plan_split(sheet, h.total_frames, h.sample_rate)
        except SheetException as err:
            results[k] = err
            continue
        if len(targets[k]) != len(cuts[k]):
            results[k] = ValueError("%d targets for the %d tracks of the sheet"
                                    % (len(targets[k]), len(cuts[k])))
            continue
        plan = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate),
                           sample_rate, channels, channel_mask, bits_per_sample)
        tracks = [None] * len(cuts[k])
        for j, (_, length) in enumerate(cuts[k]):
            frames = length
            if plan.in_rate != plan.sample_rate and frames:
                frames = _atgpu.resample_output_frames(frames, plan.channels, plan.in_rate,
                                                       plan.sample_rate)
            try:
                jobs[(k, j)] = (plan, prepare(classes[k][j], targets[k][j], plan.channels,
                                              plan.channel_mask, plan.bits_per_sample,
                                              plan.sample_rate, frames))
            except (EncodingError, ValueError) as err:
                tracks[j] = err
        files[k] = i
        results[k] = SplitResult(tracks, None, None,
                                 dict(uploaded_bytes=0, decoded_frames=0, encode_calls=0))
        if accuraterip or any(t is None for t in tracks):
            batch.want(i)
    if not batch.wanted:
        return results
    free = []
    eng = _atgpu.engine()
    try:
        batch.decode()
        counted = set()
        for k in range(n):
            i = files[k]
            if i is None or i not in batch.wanted:
                continue
            # the cuts were made for the frames the header names
            if not batch.ok(i) or batch.frames(i) != batch.headers[i].total_frames:
                results[k] = DecodingError("%s does not decode cleanly" % _name(images[k]))
                files[k] = None
                continue
            if i not in counted:
                counted.add(i)
                results[k].stats["uploaded_bytes"] = len(batch.headers[i].image)
                results[k].stats["decoded_frames"] = int(batch.frames(i))
        if accuraterip:
            # now: the finishing of a long FLAC track decodes the encoder's
            # image on the same decoder handle, whose buffers the views are
            for k in range(n):
                if files[k] is not None:
                    results[k] = _checksums(eng, free, batch, files[k], cuts[k], results[k],
                                            max_offset)
        order = sorted(kj for kj in jobs if files[kj[0]] is not None)
        sources = []
        for k, j in order:
            d_pcm, p = batch.views[files[k]]
            offset, length = cuts[k][j]
            sources.append(DevicePcm(d_pcm, _atgpu.PCM_S32,
                                     p.sample_offset + offset * batch.headers[files[k]].channels,
                                     length))
        done, more = run_chain_device(sources, [jobs[kj][0] for kj in order], dither,
                                      streams=[first_stream[k] + j for k, j in order])
        free.extend(more)
        tracks = []
        for (k, j), d in zip(order, done):
            plan, ready = jobs[(k, j)]
            cls = classes[k][j]
            if cls in (ShortenAudio, WaveAudio):
                # their headers hold the length: made for the frames that came
                try:
                    ready = prepare(cls, targets[k][j], plan.channels, plan.channel_mask,
                                    plan.bits_per_sample, plan.sample_rate, d.frames)
                except (EncodingError, ValueError) as err:
                    results[k].tracks[j] = err
                    continue
            tracks.append(Track((k, j), targets[k][j], cls, modes[k][j], d, plan.channels,
                                plan.bits_per_sample, plan.sample_rate, plan.channel_mask, ready))
        calls = {}
        for t in tracks:
            calls.setdefault(t.k[0], set()).add(_group_key(t))
        for k, keys in calls.items():
            results[k].stats["encode_calls"] = len(keys)
        for (k, j), r in write_tracks(tracks).items():
            results[k].tracks[j] = r
        return results
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()


def _checksums(eng, free, batch, i, cuts, result, max_offset):
    """result with the AccurateRip values of the image's tracks, read from
    the image's PCM where the decoder left it"""
    h = batch.headers[i]
    if (h.sample_rate, h.channels, h.bits_per_sample) != (44100, 2, 16):
        return result
    d_pcm, p = batch.views[i]
    at = p.sample_offset
    if at % 2:
        # the pass takes whole frames from its buffer's start
        keep = eng.device_alloc(max(16, 8 * p.frames))
        free.append(keep)
        eng.copy_device(keep, d_pcm + 4 * at, 8 * p.frames)
        d_pcm, at = keep, 0
    first = at // 2
    live = [j for j, (_, length) in enumerate(cuts) if length > 0]
    tracks = [_atgpu.ar_track(first + cuts[j][0], cuts[j][1], 44100, is_first=(j == 0),
                              is_last=(j == len(cuts) - 1), lo_frame=first,
                              hi_frame=first + p.frames) for j in live]
    res, table = _atgpu.accuraterip_device(d_pcm, _atgpu.PCM_S32, tracks, max_offset)
    import numpy as np
    sums = [(0, 0)] * len(cuts)
    offsets = np.zeros((len(cuts), 2 * max_offset + 1), dtype=np.uint32)
    for j, r, row in zip(live, res, table):
        sums[j] = (int(r.v1), int(r.v2))
        offsets[j] = row
    return result._replace(checksums=sums, offsets=offsets if max_offset else None)


# --------------------------------------------------------------------- join
def join_tracks_batch(albums, targets, sheets=None, target_types=None, compression=None):
    """trackcat for a batch: the files of albums[k] (filenames or bytes
    images, of any formats the decoders read, mixed at will), in order, as
    the one file targets[k].  sheets[k]: a Sheet or the name of a .cue or
    .toc file to embed in a FLAC target (FlacAudio.set_cuesheet; other
    types carry no sheet and it is only checked), or None.  target_types and
    compression: one value or one per album, as convert_files_batch reads
    them.

    All files of all albums are decoded in one batch, a file named many
    times once.  An album's pieces are laid end to end in device memory:
    where they already follow each other in one decoder's output they are
    taken where they lie, otherwise runs of them are gathered with device
    copies.  The album is encoded as one track: the file is the one
    cls.from_pcm(targets[k], PCMCat([f.to_pcm() for f in files]),
    compression, total_pcm_frames=<sum>) writes.

    -> per album the target class's instance, or its exception with no file
    left and the other albums going on: ValueError with trackcat's words,
    before any GPU work, for an empty album, files that differ in sample
    rate, channel count, channel mask or bits per sample, and a sheet that is
    unreadable, not image formatted or too long; DecodingError for a file
    that cannot be opened or does not decode cleanly; the exception the
    target type's from_pcm raises for a stream it cannot hold.  ValueError
    for lists of the wrong length and an unknown target type."""
    albums = [list(a) for a in albums]
    n = len(albums)
    targets = _per_image(targets, n, "targets")
    sheets = _per_image(sheets, n, "sheets")
    classes = [FlacAudio] * n if target_types is None else resolve_types(target_types, targets)
    modes = resolve_compression(compression, classes)

    batch = _Batch()
    results = [None] * n
    jobs = {}  # k -> (file indexes, total frames, ChainPlan, ready, Sheet or None)
    for k, album in enumerate(albums):
        idx = [batch.add(f) for f in album]
        bad = [f for f, i in zip(album, idx) if batch.headers[i] is None]
        if bad:
            results[k] = DecodingError("%s cannot be opened as audio" % _name(bad[0]))
            continue
        heads = [batch.headers[i] for i in idx]
        try:
            sheet = _load_sheet(sheets[k])
            total = plan_join([(h.sample_rate, h.channels, h.channel_mask, h.bits_per_sample)
                               for h in heads], [h.total_frames for h in heads], sheet)
            h = heads[0]
            plan = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate))
            ready = prepare(classes[k], targets[k], plan.channels, plan.channel_mask,
                            plan.bits_per_sample, plan.sample_rate, total)
        except (EncodingError, ValueError) as err:
            results[k] = err
            continue
        for i in idx:
            batch.want(i)
        jobs[k] = (idx, total, plan, ready, sheet)
    if not jobs:
        return results
    free = []
    eng = _atgpu.engine()
    try:
        batch.decode()
        order, sources = [], []
        for k in sorted(jobs):
            idx, total = jobs[k][:2]
            bad = [f for f, i in zip(albums[k], idx) if not batch.ok(i)]
            if bad or sum(batch.frames(i) for i in idx) != total:
                results[k] = DecodingError("%s does not decode cleanly"
                                           % _name(bad[0] if bad else albums[k][0]))
                continue
            order.append(k)
            sources.append(_lay_out(eng, free, batch, idx, jobs[k][2].in_channels))
        done, more = run_chain_device(sources, [jobs[k][2] for k in order])
        free.extend(more)
        tracks = []
        for k, d in zip(order, done):
            plan, ready = jobs[k][2:4]
            tracks.append(Track(k, targets[k], classes[k], modes[k], d, plan.channels,
                                plan.bits_per_sample, plan.sample_rate, plan.channel_mask, ready))
        for k, r in write_tracks(tracks).items():
            sheet = jobs[k][4]
            if sheet is not None and isinstance(r, FlacAudio) and classes[k] is FlacAudio:
                try:
                    r.set_cuesheet(sheet)
                    r = FlacAudio(targets[k])
                except (IOError, OSError, ValueError) as err:
                    from .flac import _unlink
                    _unlink(targets[k])
                    r = EncodingError(str(err))
            results[k] = r
        return results
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()


def _runs(pieces):
    """[(d_pcm, sample offset, samples)] in order -> the same with pieces
    that follow each other in one buffer merged into one run"""
    runs = []
    for d_pcm, at, samples in pieces:
        if samples == 0:
            continue
        if runs and runs[-1][0] == d_pcm and runs[-1][1] + runs[-1][2] == at:
            runs[-1] = (d_pcm, runs[-1][1], runs[-1][2] + samples)
        else:
            runs.append((d_pcm, at, samples))
    return runs


def _lay_out(eng, free, batch, idx, channels):
    """the decoded files idx end to end -> DevicePcm: in place where they are
    one run of one decoder's output, else gathered run by run into a buffer
    of the album's own (appended to `free`)"""
    pieces = []
    for i in idx:
        d_pcm, p = batch.views[i]
        pieces.append((d_pcm, p.sample_offset, p.frames * channels))
    runs = _runs(pieces)
    samples = sum(r[2] for r in runs)
    if not runs:
        return DevicePcm(None, _atgpu.PCM_S32, 0, 0)
    if len(runs) == 1:
        return DevicePcm(runs[0][0], _atgpu.PCM_S32, runs[0][1], samples // channels)
    d_album = eng.device_alloc(max(16, 4 * samples))
    free.append(d_album)
    pos = 0
    for d_pcm, at, count in runs:
        eng.copy_device(d_album + 4 * pos, d_pcm + 4 * at, 4 * count)
        pos += count
    return DevicePcm(d_album, _atgpu.PCM_S32, 0, samples // channels)
