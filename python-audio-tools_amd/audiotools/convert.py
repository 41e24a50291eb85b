"""audiotools.convert — a batch of files transcoded on the device, to FLAC or
to any other format the engine writes.

convert_files_batch is track2track's job for many files at once: every
source is opened and told apart by magic (batchfiles), all sources of one
format are decoded in one call of that format's decoder, the converter chain
runs over the decoded PCM where it lies (pcmconverter.run_chain_device:
csrc/pcm_chain.hip on either side of the resampler), the tracks that share
output parameters and target type are encoded in one encode_device call each
(targets.write_tracks), and every image is finished as its class's from_pcm
finishes it.  The PCM never comes back to the host; the encoded images do.
"""

from . import DecodingError, EncodingError
from . import _atgpu
from .batchfiles import _Batch
from .flac import FlacAudio, finish_image, _unlink
from .pcmconverter import DevicePcm, plan_target, run_chain_device
from .shn import ShortenAudio
from .targets import Track, prepare, resolve_compression, resolve_types, write_tracks
from .wav import WaveAudio


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
                        bits_per_sample=None, compression=None, dither=None, target_types=None,
                        starts=None, lengths=None):
    """sources[k] (a filename or a bytes image of any supported format) ->
    the file targets[k], converted to the target parameters as PCMConverter
    converts (None keeps each source's own value).  target_types: None for
    FLAC, else one value for all targets or one per target -- one of the
    nine classes FlacAudio, OggFlacAudio, ALACAudio, TrueAudio, WavPackAudio,
    ShortenAudio, WaveAudio, AiffAudio, AuAudio, one of their SUFFIX strings,
    or "suffix" for the type each target's file name ends in.  compression:
    one value or one per target, read against the target class's
    COMPRESSION_MODES (None or an unknown value: that class's default).
    The file is the one cls.from_pcm(targets[k], PCMConverter(
    BufferedPCMReader(source.to_pcm()), ...), compression,
    total_pcm_frames=<converted frames>) writes (encode_oggflac /
    encode_wavpack being the encoding function of those two classes), except
    for where the dither bits fall behind a resampler,
    an Ogg FLAC stream's random serial number and an .m4a's creation time.
    dither: n -> bytes (default os.urandom), drawn source by
    source in argument order; or a DeviceDither, whose stream k makes the
    bits of sources[k] on the device.
    -> per source the target class's instance, or the DecodingError /
    EncodingError instance of a file that could not be read or written (no
    target is left for it and the others go on); a source whose converted
    parameters its target type cannot hold gets the exception that type's
    from_pcm raises, before any GPU work for it.  ValueError, before any GPU
    work, for a target that PCMConverter refuses, an unknown target type and
    lists of the wrong length.

    starts, lengths: with either given, row k converts only the window
    [starts[k], starts[k] + lengths[k]) of sources[k] -- each one value or
    one per source, in PCM frames at the source's rate, before conversion; a
    start of None is 0 and a length of None runs to the end.  The rows come
    from decode_windows_batch's planner and decoder (only the covering bytes
    of a source go up, once for all the rows that name it, and the stream's
    MD5 is not checked) and go into the chain as they are.  A window is cut
    to the stream as decode_windows_batch cuts it -- it is not padded with
    silence as PCMReaderWindow pads one, so the file is the one from_pcm
    writes over PCMReaderWindow of the cut window -- and a negative value
    raises ValueError before any GPU work.  With both None the whole files
    are converted as before, their MD5 checked."""
    sources, targets = list(sources), list(targets)
    if len(sources) != len(targets):
        raise ValueError("sources and targets differ in length")
    classes = ([FlacAudio] * len(targets) if target_types is None
               else resolve_types(target_types, targets))
    modes = resolve_compression(compression, classes)
    if starts is not None or lengths is not None:
        return _convert_windows(sources, targets, classes, modes, 0 if starts is None else starts,
                                lengths, (sample_rate, channels, channel_mask, bits_per_sample),
                                dither)
    batch = _Batch()
    results = [None] * len(sources)
    jobs = []  # (k, file index, ChainPlan, what prepare() returned)
    for k, (source, target) in enumerate(zip(sources, targets)):
        i = batch.add(source)
        h = batch.headers[i]
        if h is None:
            results[k] = DecodingError("%s cannot be opened as audio" % _name(source))
            continue
        plan = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate),
                           sample_rate, channels, channel_mask, bits_per_sample)
        frames = h.total_frames
        if plan.in_rate != plan.sample_rate and frames:
            frames = _atgpu.resample_output_frames(frames, plan.channels, plan.in_rate,
                                                   plan.sample_rate)
        try:
            ready = prepare(classes[k], target, plan.channels, plan.channel_mask,
                            plan.bits_per_sample, plan.sample_rate, frames)
        except (EncodingError, ValueError) as err:
            results[k] = err
            continue
        batch.want(i)
        jobs.append((k, i, plan, ready))
    if not jobs:
        return results
    free = []
    eng = _atgpu.engine()
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
            [plan for _, _, plan, _ in good], dither, streams=[k for k, _, _, _ in good])
        tracks = []
        for (k, _, plan, ready), d in zip(good, done):
            if classes[k] in (ShortenAudio, WaveAudio):
                # their headers hold the length: made for the frames that came
                try:
                    ready = prepare(classes[k], targets[k], plan.channels, plan.channel_mask,
                                    plan.bits_per_sample, plan.sample_rate, d.frames)
                except (EncodingError, ValueError) as err:
                    results[k] = err
                    continue
            tracks.append(Track(k, targets[k], classes[k], modes[k], d, plan.channels,
                                plan.bits_per_sample, plan.sample_rate, plan.channel_mask, ready))
        for k, r in write_tracks(tracks).items():
            results[k] = r
        return results
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()


def _convert_windows(sources, targets, classes, modes, starts, lengths, want, dither):
    """convert_files_batch over one window of each source"""
    from .windows import decode_rows, plan_rows
    batch, rows, headers = plan_rows(sources, starts, lengths)
    results = list(batch.errors)
    keep = dict((r.k, r.plan.keep) for r in rows)
    jobs = []  # (k, ChainPlan, what prepare() returned)
    for k, h in enumerate(headers):
        if h is None:
            continue
        plan = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate), *want)
        frames = keep.get(k, 0)
        if plan.in_rate != plan.sample_rate and frames:
            frames = _atgpu.resample_output_frames(frames, plan.channels, plan.in_rate,
                                                   plan.sample_rate)
        try:
            ready = prepare(classes[k], targets[k], plan.channels, plan.channel_mask,
                            plan.bits_per_sample, plan.sample_rate, frames)
        except (EncodingError, ValueError) as err:
            results[k] = err
            continue
        jobs.append((k, plan, ready))
    # rows whose target is refused are not decoded
    wanted = set(k for k, _, _ in jobs)
    if not jobs:
        return results
    free = []
    eng = _atgpu.engine()
    try:
        decode_rows(batch, [r for r in rows if r.k in wanted])
        good = []
        for job in jobs:
            if batch.errors[job[0]] is None:
                good.append(job)
            else:
                results[job[0]] = batch.errors[job[0]]
        done, more = run_chain_device([batch.rows[k] for k, _, _ in good],
                                      [plan for _, plan, _ in good], dither,
                                      streams=[k for k, _, _ in good])
        free.extend(more)
        tracks = []
        for (k, plan, ready), d in zip(good, done):
            if classes[k] in (ShortenAudio, WaveAudio):
                # their headers hold the length: made for the frames that came
                try:
                    ready = prepare(classes[k], targets[k], plan.channels, plan.channel_mask,
                                    plan.bits_per_sample, plan.sample_rate, d.frames)
                except (EncodingError, ValueError) as err:
                    results[k] = err
                    continue
            tracks.append(Track(k, targets[k], classes[k], modes[k], d, plan.channels,
                                plan.bits_per_sample, plan.sample_rate, plan.channel_mask, ready))
        for k, r in write_tracks(tracks).items():
            results[k] = r
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
