"""audiotools.tensors — decoded batches as PyTorch tensors, and back.

The decoders, the converter chain and the encoders keep a batch as ragged,
channel-interleaved int16 / int32 rows behind device pointers (DevicePcm).
This module turns such rows into what a PyTorch program consumes, a padded
planar [batch, channels, frames] tensor with samples in [-1, 1), and writes
such tensors out as FLAC files, without the PCM leaving device memory
(csrc/pcm_tensor.hip, one launch per call):

  pcm_to_tensor    [DevicePcm] -> (audio[B, C, T], lengths)
  tensor_to_pcm    audio, lengths -> [DevicePcm]
  load_batch       files of any supported format -> AudioBatch
  save_flac_batch  audio, lengths -> .flac files
  save_batch       audio, lengths -> files of any type the engine writes

The arithmetic is FrameList.to_float() one way (sample / 2^(bits-1)) and
FloatFrameList.to_int(bits) the other: truncation toward zero, clamped, NaN
and +inf giving the most negative sample as the reference's cast does.  No
dither on the way back, and no autograd: the tensors are plain data.

Order of initialisation: torch cannot bring its HIP runtime up once
libatgpu's has come up.  Import this module, or initialise torch.cuda, before
the first audiotools GPU call; importing it calls torch.cuda.init() when a
GPU is available.  torch is imported here only, so `import audiotools` stays
torch-free (the four names above are looked up lazily on the package).
Everything runs on the device the batch layer uses (_atgpu.default_device()).
"""

from collections import namedtuple

import torch

if torch.cuda.is_available():
    torch.cuda.init()

from . import DecodingError, EncodingError  # noqa: E402
from . import _atgpu  # noqa: E402
from .pcmconverter import DevicePcm, plan_target, run_chain_device, _round_up  # noqa: E402

__all__ = ["AudioBatch", "pcm_to_tensor", "tensor_to_pcm", "load_batch", "save_flac_batch",
           "save_batch"]

_DTYPES = {torch.float16: _atgpu.TENSOR_F16, torch.float32: _atgpu.TENSOR_F32,
           torch.float64: _atgpu.TENSOR_F64, torch.int32: _atgpu.TENSOR_I32}

AudioBatch = namedtuple("AudioBatch", "audio lengths sample_rates bits_per_sample "
                        "channel_masks errors")


def _dtype_code(dtype):
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise ValueError("dtype must be torch.float16, float32, float64 or int32")


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("audiotools.tensors needs a GPU: torch reports CUDA unavailable")
    return torch.device("cuda", _atgpu.default_device())


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def pcm_to_tensor(rows, dtype=torch.float32, frames=None):
    """rows: [(DevicePcm, channels, bits_per_sample)], every channel count
    the same.  -> (audio, lengths): audio is a [B, C, T] tensor of `dtype`
    on the PCM's device, row k's samples / 2^(bits-1) in audio[k, :, :n_k]
    and zeros behind them (dtype torch.int32: the samples unscaled); lengths
    is a CPU int64 tensor of the n_k.  T is the longest row, or `frames`.
    One kernel call on torch's current stream, synchronised before return.
    ValueError for differing channel counts and for `frames` below a row."""
    rows = list(rows)
    code = _dtype_code(dtype)
    counts = sorted(set(int(ch) for _, ch, _ in rows))
    if len(counts) > 1:
        raise ValueError("rows differ in channel count: %s" % counts)
    longest = max([int(p.frames) for p, _, _ in rows] + [0])
    if frames is None:
        frames = longest
    elif frames < longest:
        raise ValueError("frames=%d is shorter than a row of %d frames" % (frames, longest))
    device = _device()
    ch, t = (counts[0] if counts else 0), int(frames)
    audio = torch.empty((len(rows), ch, t), dtype=dtype, device=device)
    lengths = torch.tensor([int(p.frames) for p, _, _ in rows], dtype=torch.int64)
    if audio.numel():
        table = [_atgpu.pcm_to_tensor_row(
            _atgpu.pcm_view(p.d_pcm, p.fmt, p.frames, p.sample_offset), ch, bits, t, k * ch * t, t)
            for k, (p, _, bits) in enumerate(rows)]
        _atgpu.pcm_to_tensor_device(table, audio.data_ptr(), code, audio.numel(),
                                    _stream(device))
    return audio, lengths


def _per_row(value, n, what):
    """one value, or one per row -> a list of n"""
    if isinstance(value, (list, tuple)) or torch.is_tensor(value):
        values = [int(v) for v in value]
        if len(values) != n:
            raise ValueError("%s has %d entries for %d rows" % (what, len(values), n))
        return values
    return [int(value)] * n


def _check_batch(audio, lengths):
    """-> the lengths as a list, checked against audio[B, C, T]"""
    if not torch.is_tensor(audio) or audio.dim() != 3:
        raise ValueError("audio must be a [batch, channels, frames] tensor")
    _dtype_code(audio.dtype)
    lengths = _per_row(lengths, audio.size(0), "lengths")
    for n in lengths:
        if n < 0 or n > audio.size(2):
            raise ValueError("a length of %d does not fit %d frames" % (n, audio.size(2)))
    return lengths


def tensor_to_pcm(audio, lengths, bits_per_sample, int16_out=True):
    """audio[B, C, T] (float16, float32, float64 or int32, on the device) ->
    ([DevicePcm], owner): row k is audio[k, :, :lengths[k]] interleaved, as
    FloatFrameList.to_int(bits) gives it; an int32 tensor is clamped only.
    Rows of at most 16 bits land in int16 when int16_out is set, the others
    in int32; every row starts on a 16-byte boundary, whole frames from its
    buffer's start, as run_chain_device lays rows out.  `owner` is the torch
    tensor that owns the PCM: keep it for as long as the rows are in use.
    Any batch and channel strides are taken as they are; the tensor is made
    contiguous only if its last stride is not 1.  bits_per_sample: one value
    or one per row."""
    lengths = _check_batch(audio, lengths)
    n, ch, t = audio.shape
    bits = _per_row(bits_per_sample, n, "bits_per_sample")
    for b in bits:
        if b < 1 or b > 24:
            raise ValueError("bits per sample outside 1..24")
    if ch < 1 or ch > 8:
        raise ValueError("channel count outside 1..8")
    device = _device()
    if audio.device != device:
        raise ValueError("audio must be on %s" % device)
    code = _dtype_code(audio.dtype)
    if (t > 1 and audio.stride(2) != 1) or (ch > 1 and audio.stride(1) < t):
        audio = audio.contiguous()
    fmts = [_atgpu.PCM_S16 if int16_out and b <= 16 else _atgpu.PCM_S32 for b in bits]
    sizes, starts = {_atgpu.PCM_S16: 0, _atgpu.PCM_S32: 0}, []
    for f, frames in zip(fmts, lengths):
        starts.append(_round_up(sizes[f], 8 * ch))
        sizes[f] = starts[-1] + frames * ch
    # the int16 rows, then the int32 rows from the next 16-byte boundary
    at32 = _round_up(2 * sizes[_atgpu.PCM_S16], 16)
    owner = torch.empty(max(16, at32 + 4 * sizes[_atgpu.PCM_S32]), dtype=torch.uint8,
                        device=device)
    if owner.data_ptr() % 16:
        raise RuntimeError("torch returned a buffer off a 16-byte boundary")
    base = {_atgpu.PCM_S16: owner.data_ptr(), _atgpu.PCM_S32: owner.data_ptr() + at32}
    s0, s1 = audio.stride(0), audio.stride(1) if ch > 1 else t
    extent = (n - 1) * s0 + (ch - 1) * s1 + t if n and t else 0
    out = []
    for fmt in (_atgpu.PCM_S16, _atgpu.PCM_S32):
        table = [_atgpu.pcm_from_tensor_row(k * s0, s1, lengths[k], ch, bits[k], starts[k])
                 for k in range(n) if fmts[k] == fmt and lengths[k]]
        if table:
            _atgpu.pcm_from_tensor_device(table, audio.data_ptr(), code, extent, base[fmt], fmt,
                                          sizes[fmt], _stream(device))
    for k in range(n):
        out.append(DevicePcm(base[fmts[k]], fmts[k], starts[k], lengths[k]))
    return out, owner


def _name(source):
    return source if isinstance(source, str) else "<%d-byte image>" % len(source)


def load_batch(sources, sample_rate=None, channels=None, channel_mask=None,
               bits_per_sample=None, dtype=torch.float32, dither=None, frames=None,
               start=None, length=None):
    """sources (filenames or byte images of FLAC, Ogg FLAC, ALAC, True Audio,
    WavPack, Shorten, WAV, AIFF or Sun AU) -> AudioBatch(audio, lengths,
    sample_rates, bits_per_sample, channel_masks, errors).  Every format is
    decoded in one call of its decoder, the tracks are converted to the
    target parameters as PCMConverter converts them (None keeps each source's
    own value; `dither`: n -> bytes for the tracks that lose bits, or a
    DeviceDither, whose stream k serves sources[k] on the device) and
    audio[k, :, :lengths[k]] is FrameList.to_float() of track k, channel by
    channel; the PCM is never on the host.  sample_rates, bits_per_sample and
    channel_masks are lists with one entry per source: without a target the
    sources may differ in them.
    start, length (an int or one per row, in PCM frames at the source's rate,
    before any conversion): when either is given, row k is the window [start,
    start + length) of its source, decoded by decode_windows_batch -- only
    the bytes that cover it uploaded, only its units decoded, the stream's
    MD5 unchecked; a window that starts at or past the end is a row of zeros
    with length 0 and no error.
    A source that cannot be opened or decoded stops nothing: its row is all
    zeros, its length and its list entries are 0 and errors[k] is the
    DecodingError (None for a good row).
    ValueError, before any GPU work, for a target PCMConverter refuses and
    for sources whose channel counts differ after conversion."""
    from .batchfiles import _Batch
    sources = list(sources)
    n = len(sources)
    _dtype_code(dtype)
    if start is not None or length is not None:
        return _load_windows(sources, 0 if start is None else start, length, sample_rate,
                             channels, channel_mask, bits_per_sample, dtype, dither, frames)
    batch = _Batch()
    errors, plans, index = [None] * n, [None] * n, [None] * n
    for k, source in enumerate(sources):
        i = index[k] = batch.add(source)
        h = batch.headers[i]
        if h is None:
            errors[k] = DecodingError("%s cannot be opened as audio" % _name(source))
            continue
        plans[k] = plan_target((h.channels, h.channel_mask, h.bits_per_sample, h.sample_rate),
                               sample_rate, channels, channel_mask, bits_per_sample)
        batch.want(i)
    counts = sorted(set(p.channels for p in plans if p is not None))
    if len(counts) > 1:
        raise ValueError("the sources have %s channels after conversion: pass channels= "
                         "to give every row one count" % ", ".join(map(str, counts)))
    device = _device()
    eng = _atgpu.engine()
    free = []
    try:
        batch.decode()
        good = []
        for k in range(n):
            if plans[k] is None:
                continue
            if batch.ok(index[k]):
                good.append(k)
            else:
                errors[k] = DecodingError("%s does not decode cleanly" % _name(sources[k]))
                plans[k] = None
        views = [batch.views[index[k]] for k in good]
        done, free = run_chain_device(
            [DevicePcm(d, _atgpu.PCM_S32, p.sample_offset, p.frames) for d, p in views],
            [plans[k] for k in good], dither, streams=good)
        if good:
            ch = counts[0]
            rows = [(DevicePcm(None, _atgpu.PCM_S32, 0, 0), ch, 16)] * n
            for k, d in zip(good, done):
                rows[k] = (d, ch, plans[k].bits_per_sample)
            audio, lengths = pcm_to_tensor(rows, dtype, frames)
        else:
            audio = torch.zeros((n, counts[0] if counts else 0, frames or 0), dtype=dtype,
                                device=device)
            lengths = torch.zeros(n, dtype=torch.int64)
    finally:
        for d in free:
            eng.device_free(d)
        batch.close()
    return AudioBatch(audio, lengths,
                      [p.sample_rate if p else 0 for p in plans],
                      [p.bits_per_sample if p else 0 for p in plans],
                      [p.channel_mask if p else 0 for p in plans], errors)


def _load_windows(sources, start, length, sample_rate, channels, channel_mask, bits_per_sample,
                  dtype, dither, frames):
    """load_batch over one window per source: the rows of decode_windows_batch
    through the same chain and the same tensor kernel"""
    from .windows import decode_windows_batch
    n = len(sources)
    wins = decode_windows_batch(sources, start, length)
    eng = _atgpu.engine()
    free = []
    try:
        errors = list(wins.errors)
        plans = [None if errors[k] is not None else
                 plan_target((wins.channels[k], wins.channel_mask[k], wins.bits_per_sample[k],
                              wins.sample_rate[k]),
                             sample_rate, channels, channel_mask, bits_per_sample)
                 for k in range(n)]
        counts = sorted(set(p.channels for p in plans if p is not None))
        if len(counts) > 1:
            raise ValueError("the sources have %s channels after conversion: pass channels= "
                             "to give every row one count" % ", ".join(map(str, counts)))
        device = _device()
        good = [k for k in range(n) if plans[k] is not None]
        # an empty window has nothing to convert: it stays a row of length 0
        full = [k for k in good if wins.rows[k].frames]
        done, free = run_chain_device([wins.rows[k] for k in full], [plans[k] for k in full],
                                      dither, streams=full)
        if good:
            ch = counts[0]
            rows = [(DevicePcm(None, _atgpu.PCM_S32, 0, 0), ch, 16)] * n
            for k, d in zip(full, done):
                rows[k] = (d, ch, plans[k].bits_per_sample)
            audio, lengths = pcm_to_tensor(rows, dtype, frames)
        else:
            audio = torch.zeros((n, counts[0] if counts else 0, frames or 0), dtype=dtype,
                                device=device)
            lengths = torch.zeros(n, dtype=torch.int64)
    finally:
        for d in free:
            eng.device_free(d)
        wins.close()
    return AudioBatch(audio, lengths,
                      [p.sample_rate if p else 0 for p in plans],
                      [p.bits_per_sample if p else 0 for p in plans],
                      [p.channel_mask if p else 0 for p in plans], errors)


_Target = namedtuple("_Target", "channels bits_per_sample sample_rate")


def save_batch(audio, lengths, targets, sample_rate, bits_per_sample=16, channel_mask=None,
               target_types="suffix", compression=None):
    """audio[k, :, :lengths[k]] -> the file targets[k], of any type the
    engine writes: target_types and compression as convert_files_batch takes
    them, the type by default from each target's suffix.  The file is the one
    cls.from_pcm(targets[k], <a reader of FloatFrameList(row).to_int(bits)
    with channel mask `channel_mask or 0`>, compression,
    total_pcm_frames=lengths[k]) writes (an Ogg FLAC serial number and an
    .m4a's creation time apart).  sample_rate and bits_per_sample (8, 16 or
    24): one value or one per row.  tensor_to_pcm, then one encode call per
    group of rows that share what their encoder fixes per call
    (targets.write_tracks); the PCM is never on the host.
    -> per row the class's instance, or the exception its from_pcm raises
    for a row its type cannot hold / the EncodingError of a row that could
    not be written, with no file left for it.  ValueError, before any GPU
    work, for arguments that do not fit the tensor or the targets."""
    from .targets import Track, prepare, resolve_compression, resolve_types, write_tracks
    lengths = _check_batch(audio, lengths)
    targets = list(targets)
    n, ch, _ = audio.shape
    if len(targets) != n:
        raise ValueError("targets has %d entries for %d rows" % (len(targets), n))
    rates = _per_row(sample_rate, n, "sample_rate")
    bits = _per_row(bits_per_sample, n, "bits_per_sample")
    for r, b in zip(rates, bits):
        if r <= 0:
            raise ValueError("invalid sample rate")
        if b not in (8, 16, 24):
            raise ValueError("invalid bits-per-sample")
    classes = resolve_types(target_types, targets)
    modes = resolve_compression(compression, classes)
    mask = int(channel_mask or 0)
    results, ready = [None] * n, [None] * n
    for k, target in enumerate(targets):
        try:
            ready[k] = prepare(classes[k], target, ch, mask, bits[k], rates[k], lengths[k])
        except (EncodingError, ValueError) as err:
            results[k] = err
    rows, owner = tensor_to_pcm(audio, lengths, bits)
    try:
        written = write_tracks([Track(k, targets[k], classes[k], modes[k], rows[k], ch, bits[k],
                                      rates[k], mask, ready[k])
                                for k in range(n) if results[k] is None])
    finally:
        del owner
    for k, r in written.items():
        results[k] = r
    return results


def save_flac_batch(audio, lengths, targets, sample_rate, bits_per_sample=16,
                    channel_mask=None, compression=None):
    """audio[k, :, :lengths[k]] -> the FLAC file targets[k].  The file is
    the one FlacAudio.from_pcm(targets[k], <a reader of FloatFrameList(row)
    .to_int(bits)>, compression, total_pcm_frames=lengths[k]) writes,
    SEEKTABLE and MD5 included.  sample_rate and bits_per_sample (8, 16 or
    24): one value or one per row; channel_mask: None or 0 for the layout
    FLAC assumes for the channel count.  The rows that share channels, bits,
    rate and PADDING size are encoded in one encode_device call.
    -> per row a FlacAudio, or the EncodingError of a row that could not be
    written, with no file left for it.  ValueError, before any GPU work, for
    arguments that do not fit the tensor."""
    import numpy as np
    from .convert import _finish
    from .flac import (COMPRESSION_PRESETS, DEFAULT_COMPRESSION, FlacAudio, padding_for,
                       target_layout)
    lengths = _check_batch(audio, lengths)
    targets = list(targets)
    n, ch, _ = audio.shape
    if len(targets) != n:
        raise ValueError("targets has %d entries for %d rows" % (len(targets), n))
    rates = _per_row(sample_rate, n, "sample_rate")
    bits = _per_row(bits_per_sample, n, "bits_per_sample")
    for r, b in zip(rates, bits):
        if r <= 0:
            raise ValueError("invalid sample rate")
        if b not in (8, 16, 24):
            raise ValueError("invalid bits-per-sample")
    if compression is None or compression not in FlacAudio.COMPRESSION_MODES:
        compression = DEFAULT_COMPRESSION
    preset = COMPRESSION_PRESETS[compression]
    results, masks = [None] * n, [0] * n
    for k, target in enumerate(targets):
        try:
            masks[k] = target_layout(target, ch, channel_mask or 0)
        except EncodingError as err:
            results[k] = err
    rows, owner = tensor_to_pcm(audio, lengths, bits)
    eng = _atgpu.engine()
    groups = {}
    for k, d in enumerate(rows):
        if results[k] is None:
            pad = padding_for(d.frames, rates[k] * 10)
            groups.setdefault((d.d_pcm, d.fmt, bits[k], rates[k], pad), []).append(k)
    free = []
    try:
        for (d_pcm, fmt, b, rate, pad), members in groups.items():
            try:
                opts = _atgpu.make_options(padding_size=pad, **preset)
                tracks = [(rows[k].sample_offset // ch, rows[k].frames, None) for k in members]
                _, nb = eng.bounds(opts, tracks, ch, b)
                d_out = eng.device_alloc(max(16, nb))
                free.append(d_out)
                encoded = eng.encode_device(opts, d_pcm, fmt, tracks, ch, b, rate, d_out, nb)
                out = eng.copy_to_host(np.empty(max(1, nb), dtype=np.uint8), d_out)
            except _atgpu.ATGError as err:
                for k in members:
                    results[k] = EncodingError(str(err))
                continue
            for k, res in zip(members, encoded):
                results[k] = _finish(targets[k],
                                     out[res.out_offset:res.out_offset + res.bytes].tobytes(),
                                     res.status, _Target(ch, b, rate), masks[k], rows[k].frames,
                                     preset["block_size"])
    finally:
        for d in free:
            eng.device_free(d)
        del owner
    return results
